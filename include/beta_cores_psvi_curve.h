/*
 * beta_cores_psvi_curve.h -- C ABI of libbeta_cores: the batched BatchPSVI run of beta_cores_psvi_many.h begun WITH A KIND, so
 * that the evaluation curve of a model other than logistic regression is one device run too.
 *
 * An extension of beta_cores_psvi_many.h (same library, same conventions, same run: what is begun here is continued with that
 * header's chunk, end, timing and seam entries, holds the context in the same way and obeys the same limits, reproducibility
 * contract and marking rules, all stated there).  Bound in Python by beta_cores_amd/_native.py (_PSVI_CURVE_SIGNATURES).
 *
 * Kinds served:
 *   logistic   BC_MODEL_LOGISTIC_LL with BC_VI_SAMPLER_LOGISTIC: model_params and sampler_params NULL, both counts 0 -- the run that
 *              beta_cores_psvi_many.h begins, bit for bit.
 *   Gaussian   BC_MODEL_GAUSS_LL (Gaussian location: rows x of D columns, known covariance) with BC_VI_SAMPLER_GAUSS.
 *              model_params {logdetSig, Siginv[D * D]} as the projection (beta_cores.h) takes them for this model;
 *              sampler_params mu0 | Sig0inv | Siginv as the weight-optimisation run (beta_cores_viopt.h) takes them.
 *              Per step: x^T Siginv x of the gathered rows and of every problem's points; per problem the closed-form weighted
 *              posterior A = Sig0inv + (sum w) Siginv, rhs = Sig0inv mu0 + Siginv sum_i w_i x_i, C = chol(A), L = C^-1,
 *              mu = L L^T rhs (the reference's expression), Theta = mu + E L^T, Theta' = (Siginv Theta^T)^T and
 *              theta^T Siginv theta; the tile's log-likelihood c0 - 1/2 ((ra + sa) - 2 x . Theta'), the projection's expression for
 *              this model with the x-only terms kept; residual, both gradients and ADAM as for the logistic kind.
 *              Full covariance only: diag must be 0.  start must be NULL.  D <= BC_VI_MAX_DIM.  out_modes of the run's end is mu.
 * Refused with BC_INVALID_ARGUMENT and a message, before anything is enqueued: diag != 0 or a start (Gaussian kind), a sampler
 * Siginv whose doubles are not the model's, parameter counts that do not fit D, parameters given to the logistic kind, every
 * other model or sampler kind (linear regression included), and everything beta_cores_psvi_many.h refuses.
 */
#ifndef BETA_CORES_PSVI_CURVE_H
#define BETA_CORES_PSVI_CURVE_H

#include "beta_cores_psvi_many.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Doubles of device work space of a run of the kind: the logistic figure of beta_cores_psvi_many.h, and for
 * BC_VI_SAMPLER_GAUSS, with R = sum m_p, P (S D + S) + n_sub + R more (the raw draws and theta^T Siginv theta, the row terms of
 * the gathered rows and of the points): four more pieces, each rounded up to an even count.  The Gaussian kind's constants
 * (2 D^2 + D doubles) are a buffer of their own, not part of this count.
 * Returns the count (not a status); -1 for arguments outside the limits or a sampler kind that is not served. */
int64_t bc_psvi_curve_work_doubles(int64_t total_points, int32_t n_problems, int32_t d, int32_t s, int64_t n_sub, int32_t opt_itrs,
                                   int sampler_kind);

/* Begins the batched run: the arguments of that header's begin entry, then the parameters of the kind (see above). */
int bc_psvi_curve_begin(bc_ctx* ctx, const bc_data* data, int model, int sampler_kind, int32_t diag, const double* pts,
                        const double* w0, const int64_t* row_ptr, int32_t n_problems, const double* start, int32_t s,
                        int32_t opt_itrs, const double* steps, const double* moments, int64_t n_sub, double sum_scaling,
                        const double* model_params, int32_t n_model_params, const double* sampler_params,
                        int32_t n_sampler_params);

#ifdef __cplusplus
}
#endif
#endif /* BETA_CORES_PSVI_CURVE_H */
