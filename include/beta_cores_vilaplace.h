/*
 * beta_cores_vilaplace.h -- C ABI of the seam behind the logistic Laplace sampler of the on-device weight optimisation in
 * libbeta_cores.
 *
 * An extension of include/beta_cores_viopt.h (same library, same conventions: int status, bc_last_error(), host pointers
 * borrowed for the call); kept in a header of its own so that the ABI of the existing headers stays as it is.
 * Bound in Python by beta_cores_amd/_native.py (_VILAPLACE_SIGNATURES).
 *
 * A weight optimisation run with sampler kind BC_VI_SAMPLER_LOGISTIC draws Theta = mu_w + E . C_w^-T around the mode mu_w of
 *
 *   f(mu) = -sum_n w_n log(1 + exp(-z_n . mu)) - D/2 log(2 pi) - mu . mu / 2          (rows z = y * x, prior N(0, I))
 *
 * with C_w the Cholesky factor of H = I + Z^T diag(w p (1 - p)) Z at the mode (diag flag: Theta = mu_w + E / sqrt(diag H)).
 * One launch of k_vi_laplace per step finds the mode by damped Newton steps -- at most 200, each with at most 34 halvings of
 * the step, the stopping rule of samplers._lr_mode_newton -- starting where the step before it ended; the mode never leaves the
 * device between steps.
 */
#ifndef BETA_CORES_VILAPLACE_H
#define BETA_CORES_VILAPLACE_H

#include "beta_cores_viopt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What the last executed k_vi_laplace of the most recent run left in that run's own buffers -- a seam for tests of the mode
 * search; nothing is launched.  Valid under the rules of the last-draw seam of beta_cores_viopt.h: once a run has been begun
 * and no chunk is pending, until the next run is begun.  Refused with BC_INVALID_ARGUMENT when no run has ever been begun on the
 * context, while a chunk is pending, when d is not that run's D, and after a run of another sampler kind.
 *   out_mu: d, the mode the launch ended at (before the run's first chunk, and after a run that failed in its first step: the
 *     start point the run was given).
 *   out_counts: [3]: the Newton steps of that launch | the halvings of its last line search | the Newton steps of the whole
 *     run so far.  A launch that finds the gradient exactly 0 takes no step. */
int bc_vi_laplace_last_mode(bc_ctx* ctx, int32_t d, double* out_mu, int32_t* out_counts);

#ifdef __cplusplus
}
#endif
#endif /* BETA_CORES_VILAPLACE_H */
