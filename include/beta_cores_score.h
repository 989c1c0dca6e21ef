/*
 * beta_cores_score.h -- C ABI of the held-out scorer of libbeta_cores: for T logistic parameter vectors at once, the number of
 * held-out rows each predicts correctly and its summed held-out log-likelihood (the drivers' compute_accuracy and
 * log_likelihood(...).sum() of model_lr.py), computed on the device -- from host thetas, or straight from the sample buffer a
 * chunk of the batched small-problem sampler (beta_cores_hmc_small.h) has just filled, so that the samples need not be copied
 * to the host at all.
 *
 * An extension of include/beta_cores.h (same library, same conventions: int status, bc_last_error(), host pointers borrowed
 * for the call).  Bound in Python by beta_cores_amd/_native.py (_SCORE_SIGNATURES).
 *
 * Held-out data: zt, resident rows z_n = y_n x_n (Nt x D, float64 or float32 storage), and yt, their labels (Nt x 1, float64,
 * every entry +1 or -1; the caller guarantees that).  For every theta_t (kernel k_lr_score, csrc/bc_score.hip):
 *
 *   s_n = z_n . theta_t     ll[t] = sum_n ll(-s_n)     correct[t] = #{n : (y_n = +1 and s_n >= 0) or (y_n = -1 and s_n > 0)}
 *
 * ll(m) = -(max(m, 0) + log1p(exp(-|m|))) for m < 100 and -m from there on, as everywhere in the library.  The prediction rule
 * is the reference's "predict -1 iff log_likelihood(-x, theta) > log_likelihood(x, theta), +1 on a tie": it gives the
 * reference's prediction for every margin with |x . theta| >= 1.5e-16, exact zeros (ties: +1) included.  For 0 < |x . theta| <
 * about 2.2e-16 the reference's two log-likelihoods can round to a tie where the sign is negative; that is not emulated.
 *
 * Limits: 1 <= D <= BC_HMC_MAX_DIM, Nt >= 1, T >= 1 (T is tiled: no cap besides memory and the grid's 2^37); anything else is refused with
 * BC_INVALID_ARGUMENT before a launch.
 *
 * Reproducibility: every sum has a fixed order (over D one ascending chain; over rows the tiles of 16 in ascending order, four
 * interleaved partial sums per theta combined as (a0 + a1) + (a2 + a3); rows are never split over blocks; no floating-point
 * atomics).  The bits of one theta's scores do not depend on T, on its place in the batch or on the other thetas, and float32
 * rows give the bits of the same values stored as float64.
 */
#ifndef BETA_CORES_SCORE_H
#define BETA_CORES_SCORE_H

#include "beta_cores_hmc_small.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Uploads the thetas, runs the kernel and waits.
 *   theta: host, T x D, all finite (checked on the host: T D numbers).   out_correct: T.   out_ll: T.
 * Refused while a sampler run of beta_cores_hmc.h or beta_cores_hmc_small.h is open on the context (the table is beside
 * bc_ctx_refuse_busy in csrc/bc_core.hip). */
int bc_lr_score(bc_ctx* ctx, const bc_data* zt, const bc_data* yt, const double* theta, int64_t t, int32_t* out_correct, double* out_ll);

/* Scores the pending chunk of the open batched small-problem run where it lies.  Valid only between that run's chunk begin and
 * the chunk's end.  Enqueues k_lr_score on the library's stream over the chunk's sample buffer -- P x k x C x D, that is
 * T = P k C thetas -- and does not wait.  zt must have the run's D columns; zt and yt must stay alive until the chunk has been
 * ended.  The score buffers belong to the run. */
int bc_score_chunk(bc_ctx* ctx, const bc_data* zt, const bc_data* yt);

/* The chunk end of beta_cores_hmc_small.h plus the two score arrays: waits and copies.
 *   out_samples: P x k x C x D, or NULL: the sample copy -- the largest transfer of a chunk -- is skipped.
 *   out_logjoint, out_accept: P x k x C.   out_status: P.   These three are required.
 *   out_correct, out_ll: P x k x C, given together.  With them the call is refused, and the chunk left pending, unless
 *   bc_score_chunk was called for this chunk.  Both NULL: nothing is fetched from the scorer and none is needed (a warm-up
 *   chunk, of which only the accept flags are wanted).
 * A marked problem gets BC_NUMERICAL_PRECISION in out_status and nothing is copied for it, as in the plain chunk end.  The plain
 * chunk end still serves a scored chunk; it fetches no scores. */
int bc_score_chunk_end(bc_ctx* ctx, double* out_samples, double* out_logjoint, int32_t* out_accept, int32_t* out_status,
                       int32_t* out_correct, double* out_ll);

#ifdef __cplusplus
}
#endif
#endif /* BETA_CORES_SCORE_H */
