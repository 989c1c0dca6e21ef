/*
 * beta_cores_diag.h -- C ABI of the chain summary of libbeta_cores: for P problems at once, the posterior mean and covariance,
 * split-R-hat and the effective sample size of HMC chains, computed on the device -- from host samples, or from the kept chunks
 * of an open run of the batched small-problem sampler (beta_cores_hmc_small.h), retained on the device as they are produced,
 * so that a run whose samples are never copied to the host can still be diagnosed.
 *
 * An extension of include/beta_cores.h (same library, same conventions: int status, bc_last_error(), host pointers borrowed
 * for the call).  Bound in Python by beta_cores_amd/_native.py (_DIAG_SIGNATURES).
 *
 * Samples: P problems x n kept iterations x C chains x D coordinates, D fastest.  Definitions, per problem and coordinate
 * (the arithmetic is csrc/bc_diag_dev.h, the kernels csrc/bc_diag.hip).  Let h = n / 2 (integer division), N = n C.  The 2 C
 * SEQUENCES are, for every chain c, its first h draws (sequence 2 c) and its last h draws (sequence 2 c + 1); when n is odd the
 * middle draw belongs to neither, but it counts in the mean and the covariance.
 *
 *   mean[j]       = (sum over all N draws of x[j]) / N
 *   cov[j][l]     = (sum over all N draws of (x[j] - mean[j]) (x[l] - mean[l])) / (N - 1)      two passes, no raw second moments
 *   m_s, v_s      = mean and variance (divisor h - 1) of sequence s
 *   W             = mean_s v_s          Bh = (sum_s (m_s - mean_s m_s)^2) / (2 C - 1)          varplus = (h - 1) / h * W + Bh
 *   rhat          = sqrt(varplus / W);  W = 0 gives NaN
 *   a_s(t)        = (1 / h) sum_{i < h - t} (x_i - m_s) (x_{i + t} - m_s),   abar(t) = mean_s a_s(t)
 *   rho_0 = 1,    rho_t = 1 - (W - abar(t)) / varplus   for 1 <= t <= L,   L = min(max_lag, h - 1)
 *   P_k           = rho_{2k} + rho_{2k + 1}   for k = 0 .. (L + 1) / 2 - 1 (integer division: the number of pairs)
 *   K             = the first k with P_k not > 0; if there is none, K = the number of pairs and ess_truncated = 1
 *   P'_0 = P_0,   P'_k = min(P_k, P'_{k - 1}),   tau = -1 + 2 sum_{k < K} P'_k,   ess = 2 C h / tau;   K = 0 gives ess = NaN
 *                 (a strongly antithetic chain is such a case).  Nothing else is guarded: with rho_1 < -1/2 the one pair
 *                 P_0 < 1/2 gives tau < 0 and a negative ess, as the formula has it -- a handful of draws can do that.
 *
 * How the sums are formed: on the draws less the coordinate's first draw, y = x - x_0.  mean = x_0 + mean(y); m_s, v_s, a_s(t)
 * and what follows from them are those of y (a common shift changes none of them).  A coordinate of mean 1e8 and unit spread
 * thus loses nothing to its mean, and a constant coordinate is all zeros: its mean is its value, its covariance row and column
 * are exact zeros, W = 0 and varplus = 0, rhat and ess are NaN.
 *
 * Limits: 1 <= C <= BC_HMC_MAX_CHAINS, 1 <= D <= BC_HMC_MAX_DIM, n >= 4 and n C < 2^31, P >= 1, max_lag >= 1 (a max_lag
 * above h - 1 is clipped, not refused), and a work space (bc_diag_work_doubles) of at most BC_DIAG_MAX_WORK_DOUBLES.  Anything
 * else is refused with BC_INVALID_ARGUMENT before anything is enqueued.
 *
 * Outputs, all host, row-major: out_mean P x D, out_cov P x D x D, out_rhat P x D, out_ess P x D, out_ess_truncated P x D
 * (int32: 0 or 1), out_status P (BC_OK or BC_NUMERICAL_PRECISION) -- these six are required -- and two test seams, each NULL or
 * given: out_rho P x D x (L + 1), the rho_t the device used (rho_0 = 1; a lag behind the pair at which the sum stopped was
 * never evaluated and reads NaN), and out_moments P x D x 2, the W and varplus it used.  A problem with a sample that is not
 * finite -- or one the sampler had marked -- gets BC_NUMERICAL_PRECISION in out_status and its slices of every other output are
 * left as they were; the other problems are not affected.
 *
 * Reproducibility: every sum has a fixed order (the mean: 256 interleaved partial sums, combined in a fixed tree; a sequence's
 * sums: 64 interleaved partial sums; sums over sequences: ascending; the covariance: the N draws in chunks of
 * BC_DIAG_COV_CHUNK, ascending within a chunk, the chunks' partial products added in chunk order; no floating-point atomics).
 * A problem's bits do not depend on P or on its place in the batch, and, for the attached form, not on how the kept iterations
 * were divided into chunks: the retained buffer is a copy.
 */
#ifndef BETA_CORES_DIAG_H
#define BETA_CORES_DIAG_H

#include "beta_cores_hmc_small.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BC_DIAG_MAX_WORK_DOUBLES ((int64_t)1 << 29) /* 4 GiB: the curve of 101 problems x 1000 x 16 x 128 needs 4.2e8 stand-alone */
#define BC_DIAG_COV_CHUNK 2048                      /* draws per partial product of the covariance */

/* The doubles of device work space the summary of P x n x C x D with max_lag needs, or -1 outside the limits above (the cap
 * included).  With e(x) = x rounded up to an even number, L = min(max_lag, n / 2 - 1), T = t (t + 1) / 2 for t = ceil(D / 16)
 * and G = ceil(n C / BC_DIAG_COV_CHUNK):
 *   2 e(P n C D)  [the uploaded samples and the retained layout]  +  e(256 P G T)  [partial covariance tiles]
 *   + 3 e(P D) [mean, rhat, ess] + e(P D D) [cov] + e(2 P D) [W, varplus] + e(P D (L + 1)) [rho]
 *   + e(ceil(P D / 2)) [truncation flags, ints] + e(ceil(P / 2)) [marks, ints] */
int64_t bc_diag_work_doubles(int64_t p, int64_t n, int32_t c, int32_t d, int64_t max_lag);

/* Uploads the samples, runs the summary and waits.   samples: host, P x n x C x D.
 * Refused while any run or gradient holds the context (the table is beside bc_ctx_refuse_busy in csrc/bc_core.hip). */
int bc_chain_summary(bc_ctx* ctx, const double* samples, int64_t p, int64_t n, int32_t c, int32_t d, int64_t max_lag, double* out_mean,
                     double* out_cov, double* out_rhat, double* out_ess, int32_t* out_ess_truncated, int32_t* out_status, double* out_rho,
                     double* out_moments);

/* Attaches a summary of n_keep kept iterations to the open run of the batched small-problem sampler: allocates the retained
 * buffer for that run's P, C and D.  Valid only while such a run is open; a second attach to the same run is refused. */
int bc_diag_attach(bc_ctx* ctx, int64_t n_keep, int64_t max_lag);

/* Folds the pending chunk of that run into the summary.  Valid only between the run's chunk begin and the chunk's end, once per
 * chunk.  Enqueues the transposing copy of the chunk's samples into the retained buffer on the library's stream and does not
 * wait.  Chunks for which it is not called (warm-up) are not part of the summary; more than n_keep iterations in total are
 * refused, and the refused chunk is not folded. */
int bc_diag_chunk(bc_ctx* ctx);

/* Runs the summary of the n_keep retained iterations, waits and copies; the outputs are those of bc_chain_summary.  Valid once
 * the last kept chunk has been ended, before or after the run itself has been ended; it detaches the summary.  Fewer than
 * n_keep folded iterations, or a chunk still pending, are refused (and the summary stays attached).  Problems the sampler had
 * marked stay marked. */
int bc_diag_end(bc_ctx* ctx, double* out_mean, double* out_cov, double* out_rhat, double* out_ess, int32_t* out_ess_truncated,
                int32_t* out_status, double* out_rho, double* out_moments);

#ifdef __cplusplus
}
#endif
#endif /* BETA_CORES_DIAG_H */
