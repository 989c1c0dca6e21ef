/*
 * beta_cores_nnls.h -- C ABI of the device NNLS refit in libbeta_cores.
 *
 * An extension of include/beta_cores.h (same library, same conventions: int status, bc_last_error()); kept in a header of
 * its own so that the core ABI of beta_cores.h stays as it is.  Bound in Python by beta_cores_amd/_native.py
 * (_NNLS_SIGNATURES).
 *
 * OrthoPursuit's reweight (w[f] = 1; w[active] = nnls(A[:, active], b)) and SparseNNLS.optimize() are non-negative
 * least-squares solves on the at most M cached columns of the active list.  The entry points below run them on the device:
 * a Gram matrix of the cached fp64 columns is kept next to the list and a single thread block runs Lawson-Hanson's
 * active-set method on it, warm-started from the current weights (csrc/bc_nnls_dev.h).  The result is the NNLS minimiser --
 * the same support and the same weights to rounding as scipy.optimize.nnls on these columns, not SciPy's bits.
 *
 * Limits: single-rank solvers (world == 1), and a list of at most BC_NNLS_MAXP = 128 entries; both are refused with
 * BC_INVALID_ARGUMENT and a message.  The build calls, bc_snnls_optimize and a refit of a longer list refuse before anything
 * is enqueued; whether bc_snnls_refit(h, f) still finds a slot for f in a list of 128 (f listed already, or a slot of weight
 * 0) is decided by its kernel, which then leaves weights, list and selection state as they were.  Everything is opt-in: a solver on which none of these was
 * called behaves as before (bc_snnls_build* refuses BC_ALG_OMP, bc_snnls_reweight refuses it always).
 */
#ifndef BETA_CORES_NNLS_H
#define BETA_CORES_NNLS_H

#include "beta_cores.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Opt in (on != 0) or out (0).  On: bc_snnls_build, bc_snnls_build_begin / step_local / step_finish accept a BC_ALG_OMP
 * handle and run the guarded OrthoPursuit iteration with the refit on the device; a build call whose list could outgrow
 * the limit (listed entries + itrs > 128) is refused.  Refused for world != 1. */
int bc_snnls_device_refit(bc_snnls* h, int on);
/* orthopursuit.py:37-41 on the device, the step-wise twin of the fused step (same device functions, same bits): column f
 * -- the last selection, or any row of the local shard -- gets a list slot and the entries with a positive weight plus f
 * are refitted.  Works on any algorithm's list.  f < 0: NNLS over every cached column of the list, zero-weight entries
 * included.  Status like bc_snnls_reweight: BC_NUMERICAL_PRECISION (weights untouched) when the refit does not converge. */
int bc_snnls_refit(bc_snnls* h, int64_t f);
/* snnls.py:82-97: refit the entries with a positive weight; keep the result (*accepted = 1) unless the error grew beyond
 * (1 + tol) times the previous one, else restore the weights, set reached_numeric_limit and report *accepted = 0.  For
 * GIGA / FrankWolfe / OrthoPursuit handles alike. */
int bc_snnls_optimize(bc_snnls* h, int* accepted);
/* counters since the handle was created: refits, factor-and-solve rounds over all of them, columns rejected on entry
 * (Lawson-Hanson's rule: dependent on the passive set, or an own weight <= 0).  Any pointer may be NULL. */
int bc_snnls_refit_stats(const bc_snnls* h, int64_t* refits, int64_t* solves, int64_t* rejected);

#ifdef __cplusplus
}
#endif
#endif /* BETA_CORES_NNLS_H */
