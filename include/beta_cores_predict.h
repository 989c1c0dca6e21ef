/*
 * beta_cores_predict.h -- C ABI of the held-out scorer of the linear-regression family of libbeta_cores: for T Gaussian
 * posteriors of a linear head at once, the summed Gaussian predictive log density and the summed squared error over held-out
 * rows that stay resident on the device (what the neural-linear driver's test() reports per coreset: the mean negative log
 * density of the Bayesian head's predictive and the RMSE), and on request the per-row predictive mean and variance.
 *
 * An extension of include/beta_cores.h (same library, same conventions: int status, the last-error string, host pointers
 * borrowed for the call).  Bound in Python by beta_cores_amd/_native.py (_PREDICT_SIGNATURES).
 *
 * Held-out data: zt, resident rows [phi_n, y_n] (Nt x (D + 1): the features, then the target; float64 or float32 storage,
 * float32 widened exactly).  For every posterior t with mean mu_t, covariance F_t F_t^T (F_t ANY D x D matrix: a Cholesky
 * factor, or a factor that is not triangular), noise_t and scale_t (kernel k_linreg_predict, csrc/bc_predict.hip):
 *
 *   m_nt   = phi_n . mu_t
 *   q_nt   = || F_t^T phi_n ||^2
 *   var_nt = noise_t + scale_t q_nt
 *   ll[t]  = sum_n -1/2 ( (y_n - m_nt)^2 / var_nt + log var_nt + log 2 pi )
 *   sse[t] = sum_n (y_n - m_nt)^2
 *
 * The covariance enters as a factor, so the variance is a sum of squares and cannot go negative.  noise = sigma^2, scale = 1 is
 * the reference's Gaussian head (BayesianRegressionDense); noise = scale = b / a gives the variance of its fully Bayesian head.
 * The density is Gaussian; the Student-t density of the fully Bayesian head is not offered.
 *
 * Limits: 1 <= D <= 512, Nt >= 1, T >= 1, one device; anything else is refused with BC_INVALID_ARGUMENT before a launch.
 *
 * Reproducibility: every sum has a fixed order (csrc/bc_predict_dev.h states each one); rows are split over blocks in chunks of a
 * compile-time length and a posterior's block partials are added in ascending chunk order by a second kernel; no floating-point
 * atomics.  The bits of one posterior's results do not depend on T, on its place in the batch, on the other posteriors or on
 * whether the per-row outputs were requested, and float32 rows give the bits of the same values stored as float64.  A
 * non-finite feature or target gives non-finite results, no error.
 */
#ifndef BETA_CORES_PREDICT_H
#define BETA_CORES_PREDICT_H

#include "beta_cores.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Uploads the posteriors, runs the kernels, waits and copies.
 *   zt: Nt x (D + 1), on this context.
 *   mu: host, T x D.   factor: host, T x D x D row-major, covariance = F F^T.   noise, scale: host, T each; noise > 0, scale >= 0.
 *   Every entry of the four must be finite (checked on the host).
 *   out_ll, out_sse: T each.   out_mean, out_var: T x Nt each, given together, or both NULL.
 * A refusal names the offending argument and writes to no output.  Refused while a sampler run of beta_cores_hmc.h or
 * beta_cores_hmc_small.h is open on the context (the table is in csrc/bc_core.hip). */
int bc_linreg_predict(bc_ctx* ctx, const bc_data* zt, const double* mu, const double* factor, const double* noise, const double* scale,
                      int64_t t, double* out_ll, double* out_sse, double* out_mean, double* out_var);

#ifdef __cplusplus
}
#endif
#endif /* BETA_CORES_PREDICT_H */
