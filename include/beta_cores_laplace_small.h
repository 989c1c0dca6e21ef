/*
 * beta_cores_laplace_small.h -- C ABI of the batched Laplace fit of libbeta_cores for MANY SMALL logistic posteriors at once:
 * the weighted coresets of an evaluation curve, each of at most a few hundred rows.
 *
 * An extension of include/beta_cores.h (same library, same conventions: int status, the last error's message, host pointers
 * borrowed for the call).  Bound in Python by beta_cores_amd/_native.py (_LAPLACE_SMALL_SIGNATURES).  beta_cores_laplace.h is the fit of
 * ONE problem of any size, pass by pass with the D x D algebra on the host; this header is the other end: one thread block per
 * problem does the whole fit (kernel k_laplace_many, csrc/bc_laplace_small.hip), P problems in the time of the slowest one, and
 * no mode, factor or draw crosses the host link before the end.
 *
 * Per problem, with rows z = y * x, weights w and the prior N(0, I):
 *
 *   mu    = argmax_th f(th),  f(th) = -sum_n w_n softplus(-z_n . th) - (D / 2) log(2 pi) - |th|^2 / 2
 *   H     = I + Z^T diag(w p (1 - p)) Z  at mu,  p_n = sigmoid(-z_n . mu)         hdiag = diag H
 *   C     = chol(H) (lower),  C^-1                                                (the Laplace posterior is N(mu, C^-T C^-1))
 *   theta = mu + E . C^-T          (diag: theta = mu + E / sqrt(hdiag), no factors)
 *
 * The mode search is the damped Newton iteration of csrc/bc_vi_laplace_dev.h, the device function the weight optimisation loop
 * runs for its logistic sampler (beta_cores_vilaplace.h): at most 200 steps of at most 34 halvings, the host's backtracking
 * constants and stopping rule.  A weight that is not positive contributes exactly nothing.  Newton only: the reference's BFGS
 * search is not offered here.
 *
 * Problems are host arrays, packed exactly as in beta_cores_hmc_small.h:  rows: (sum_p n_p) x D float64, problem p's rows at
 * row_ptr[p] .. row_ptr[p + 1] - 1;  w: one weight per row;  row_ptr: P + 1 entries, row_ptr[0] = 0, strictly increasing (every
 * n_p >= 1).  D is common to the batch.  The rows stay in device memory, so a problem need not fit a block's LDS: n_p <= 2^24.
 *
 * Limits: P >= 1, 1 <= D <= BC_LAPLACE_SMALL_MAX_DIM, 0 <= S <= BC_LAPLACE_SMALL_MAX_DRAWS; anything else, a NULL required
 * argument or held-out data of another context is refused with BC_INVALID_ARGUMENT before anything is enqueued, and no output
 * is written.  One device: no row shards, no communicator, no device random-number generator.
 *
 * Reproducibility: every loop has a fixed bound and every sum a fixed order.  The bits of a problem's results depend on its own
 * rows, weights, start and normals only -- not on P, on the problem's place in the batch or on the other problems.
 */
#ifndef BETA_CORES_LAPLACE_SMALL_H
#define BETA_CORES_LAPLACE_SMALL_H

#include "beta_cores_score.h"

#define BC_LAPLACE_SMALL_MAX_DIM 128      /* == BC_VI_MAX_DIM of beta_cores_viopt.h: the work space of a fit is one block's LDS */
#define BC_LAPLACE_SMALL_MAX_DRAWS 256

#ifdef __cplusplus
extern "C" {
#endif

/* Validates, stages the batch in one transfer, launches the fit (and the scorer), waits and copies.
 *   start: host, P x D, where each Newton iteration begins; NULL: zeros.    diag: 0, or 1 for the diagonal form.
 *   normals: host; NULL exactly when s == 0.
 *     problem_stride = 0: all problems read the same s x D block (common random numbers).
 *     problem_stride >= s D: problem p reads s x D numbers at normals + p * problem_stride.
 *   zt, yt: held-out rows and labels as beta_cores_score.h takes them, both NULL or both given.  Given: the draws are scored on
 *     the device where they lie -- T = P s parameter vectors, by that header's kernel -- which needs s >= 1 and zt of D columns.
 * Outputs (host):
 *   out_mu: P x D.   out_hdiag: P x D.   out_value: P, f(mu).
 *   out_counts: P x 3: Newton steps | halvings of the last line search | halvings of all line searches.
 *   out_status: P.   These five are required.
 *   out_chol, out_inv: P x D x D each, C and C^-1, dense, row-major, the upper triangle exactly 0.  Given together or both
 *     NULL; they must be NULL with diag.
 *   out_theta: P x s x D, or NULL: no draw is copied.
 *   out_correct, out_ll: P x s each; given exactly when zt and yt are.
 * A weight, start, value, decrement or pivot that is not finite (a pivot must also be positive) marks ITS PROBLEM on the
 * device: out_status[p] = BC_NUMERICAL_PRECISION and nothing is written or copied for p in any output; the other problems are
 * unaffected, with out_status = BC_OK.  The call returns BC_OK whenever the call itself worked.
 * Refused while a fused gradient is pending or a run of any kind (weight optimisation, beta_cores_hmc.h,
 * beta_cores_hmc_small.h) is open on the context; the call is synchronous and holds nothing after it returns.  (The whole
 * table is beside bc_ctx_refuse_busy in csrc/bc_core.hip.) */
int bc_laplace_small(bc_ctx* ctx, const double* rows, const double* w, const int64_t* row_ptr, int32_t n_problems, int32_t d,
                     const double* start, int32_t diag, const double* normals, int64_t problem_stride, int32_t s,
                     const bc_data* zt, const bc_data* yt, double* out_mu, double* out_hdiag, double* out_value,
                     int32_t* out_counts, int32_t* out_status, double* out_chol, double* out_inv, double* out_theta,
                     int32_t* out_correct, double* out_ll);
/* GPU milliseconds between HIP events around the launches of the last call (the transfer in and the copies out excluded). */
int bc_laplace_small_device_ms(bc_ctx* ctx, double* out_ms);

#ifdef __cplusplus
}
#endif
#endif /* BETA_CORES_LAPLACE_SMALL_H */
