/*
 * beta_cores_psvi_many.h -- C ABI of the batched BatchPSVI run of libbeta_cores: the pseudo-coresets of MANY sizes (the
 * evaluation curve m = 1 .. M of bayesiancoresets/coreset/bpsvi.py) optimised in lock-step in one device run.
 *
 * An extension of include/beta_cores.h (same library, same conventions: int status, the last error's message, host pointers
 * borrowed for the call).  Bound in Python by beta_cores_amd/_native.py (_PSVI_MANY_SIGNATURES).  A chunked run like
 * beta_cores_viopt.h's: the HOST draws the random numbers (NumPy's legacy stream, in the reference's order) and uploads them per
 * chunk of steps; the steps are enqueued with plain stream launches and the host waits once per chunk.
 *
 * P problems; problem p has m_p points of width D (packed as in beta_cores_hmc_small.h: row_ptr of P + 1 entries, row_ptr[0] = 0,
 * strictly increasing) and m_p weights.  All problems share each step's draws -- common random numbers, which is what
 * size-m builds started from one stream state see: one S x D block of normals E and one set of n_sub row numbers.  One step, for
 * every problem, stream-ordered:
 *
 *   1. gather    the step's n_sub rows of the resident data (float64 or float32), once for the whole batch
 *   2. fit, draw the Laplace fit of (points_p, w_p) by the damped Newton search of csrc/bc_vi_laplace_dev.h (beta_cores_vilaplace.h),
 *                started at the problem's previous mode, which stays on the device, and one full Newton step from
 *                where that search ends; Theta_p = mu_p + E . C_p^-T, or with diag
 *                mu_p + E / sqrt(diag H_p)
 *   3. target    target_p = sum_scaling * sum over the gathered rows of their row-centred log-likelihoods under Theta_p: a batched
 *                contraction on the fp64 matrix cores over a grid of problems x row tiles, the partial sums added in tile order
 *   4. residual  corevecs_p (m_p x S, row-centred), resid_p = target_p - w_p . corevecs_p, g_w = -corevecs_p . resid_p / S, and the
 *                point-gradient of beta_cores_psvi.h (the m x S x D tensor is never formed)
 *   5. ADAM      one step of util/opt.py's partial_nn_opt on x_p = (w_p, points_p): b1 = 0.9, b2 = 0.999, eps = 1e-8, max(., 0) on
 *                the m_p weights only
 *
 * Scope: two kinds of run.
 *   logistic   model BC_MODEL_LOGISTIC_LL with sampler kind BC_VI_SAMPLER_LOGISTIC (Newton search), diag 0 or 1, rows z = y * x of
 *              exactly D columns, prior N(0, I): the steps above (bc_psvi_many_begin, or bc_psvi_curve_begin without parameters).
 *   Gaussian   model BC_MODEL_GAUSS_LL (Gaussian location, rows x of D columns, known covariance) with sampler kind
 *              BC_VI_SAMPLER_GAUSS, through bc_psvi_curve_begin.  Step 2 is a closed form instead of a search:
 *                2a. row aux    ra_r = x_r^T Siginv x_r of the gathered rows, once for the whole batch, and of every problem's points
 *                               (the expression of the projection's row quadratic form; float32 rows widened as they are read)
 *                2b. posterior  A = Sig0inv + (sum w) Siginv, rhs = Sig0inv mu0 + Siginv sum_i w_i x_i, C = chol(A), L = C^-1,
 *                               mu_p = L L^T rhs (the reference's expression), Theta_p = mu_p + E L^T,
 *                               Theta'_p = (Siginv Theta_p^T)^T, sa_q = theta_q^T Siginv theta_q (A, C, L and mu by the
 *                               block of k_vi_sampler, beta_cores_viopt.h, bit for bit; the three products on the fp64
 *                               matrix cores in a fixed order of their own)
 *              and step 3's log-likelihood is c0 - 1/2 ((ra + sa_q) - 2 x . Theta'_q), K1's expression for this model, x-only terms
 *              kept.  Steps 4-5 are the same code; the point-gradient takes Theta'_p and Siginv.  out_modes is mu_p.  Full
 *              covariance only (diag = 0), start = NULL, and the sampler's Siginv must be the model's, double for double.
 * The two entries that take a kind, bc_psvi_curve_begin and bc_psvi_curve_work_doubles, are declared in beta_cores_psvi_curve.h;
 * a run begun there continues with this header's chunk, end, timing and seam entries.
 * Refused with BC_INVALID_ARGUMENT and a message: every other model or sampler kind (linear regression included), n_sub = 0
 * (all rows every step), data of another context.  Not offered at all: encoders, row shards or communicators, the reference's BFGS
 * search, a device random-number generator, per-problem independent draws.
 *
 * Limits, refused with BC_INVALID_ARGUMENT before anything is enqueued:
 *   1 <= D <= BC_VI_MAX_DIM, 1 <= S <= BC_PSVI_MANY_MAX_SAMPLES, 1 <= n_sub <= BC_PSVI_MANY_MAX_SUB, 1 <= opt_itrs,
 *   1 <= P <= BC_PSVI_MANY_MAX_PROBLEMS, 1 <= m_p <= BC_PSVI_MANY_MAX_POINTS, and the run's device work space
 *   (bc_psvi_many_work_doubles / bc_psvi_curve_work_doubles) at most BC_PSVI_MANY_MAX_WORK_DOUBLES.  The Gaussian kind's
 *   posterior block takes 2 D (D + 1) / 2 + 3 D + 2 doubles of LDS (132 KiB at D = 128: one block per compute unit).
 *
 * Reproducibility: every loop has a fixed bound and every sum a fixed order.  The bits of a problem's results depend on its own
 * points, weights, start, steps and the shared draws only -- not on P, on its place in the batch or on the other problems.  Float32
 * data rows give the bits of their widened float64 copy.
 *
 * A weight, value of the log-joint, gradient component or pivot that is not finite (a pivot must also be positive) marks THAT
 * PROBLEM on the device: its later steps return at once, out_status[p] = BC_NUMERICAL_PRECISION and nothing is copied for it.
 * The other problems are unaffected.
 */
#ifndef BETA_CORES_PSVI_MANY_H
#define BETA_CORES_PSVI_MANY_H

#include "beta_cores_viopt.h"

#define BC_PSVI_MANY_MAX_SAMPLES 256
#define BC_PSVI_MANY_MAX_SUB 262144                 /* rows per sub-sample: 16 384 row tiles of 16 in the target's grid */
#define BC_PSVI_MANY_MAX_PROBLEMS 4096
#define BC_PSVI_MANY_MAX_POINTS 4096                /* per problem: 256 point tiles of 16 beside the row tiles */
#define BC_PSVI_MANY_MAX_WORK_DOUBLES (1ll << 27)   /* 1 GiB of device work space */

#ifdef __cplusplus
extern "C" {
#endif

/* Doubles of device work space of a run: with R = sum m_p and T = ceil(n_sub / 16),
 *   R (5 D + 8 + S) + R / 2 + P (S D + D + T S + 2 S + opt_itrs + 2) + P / 2 + 2 opt_itrs + 1      (state, moments, gradients, the
 *   last step's snapshot, Theta, corevecs, partial sums, row scratch, step arrays, row_ptr and the ints), rounded up piece by
 *   piece to even counts.
 * The Gaussian kind (sampler_kind BC_VI_SAMPLER_GAUSS) adds P (S D + S) + n_sub + R: the raw draws Theta_p and sa, and the row aux
 *   of the gathered rows and of the points -- four more pieces, rounded up the same way.  Its constants (Sig0inv, Sig0inv mu0,
 *   Siginv: 2 D^2 + D doubles) and, for both kinds, the gathered rows are small buffers of their own, not part of this count.
 * Returns the count (not a status); -1 for arguments outside the limits above or a sampler kind that is not served.
 * bc_psvi_many_work_doubles is the logistic kind's count. */
int64_t bc_psvi_many_work_doubles(int64_t total_points, int32_t n_problems, int32_t d, int32_t s, int64_t n_sub, int32_t opt_itrs);

/* Steps per chunk that keep a chunk's staged draws (normals + indices) under BC_VI_STAGE_BYTES (at least 1): a count, not a status. */
int bc_psvi_many_auto_chunk(int32_t s, int32_t d, int64_t n_sub);

/* Validates everything but the indices and stages what is constant over the run; zeroes both moments; nothing runs yet.
 *   data: the resident rows, D columns, float64 or float32.
 *   model: BC_MODEL_LOGISTIC_LL.   sampler_kind: BC_VI_SAMPLER_LOGISTIC.   diag: 0 or 1.   (the Gaussian kind: beta_cores_psvi_curve.h)
 *   pts: host, (sum m_p) x D, the initial points.   w0: host, sum m_p.   row_ptr: host, P + 1.
 *   start: host, P x D, where each problem's first mode search begins; NULL: zeros.
 *   steps: host, [P][opt_itrs]: step_sched(m_p)(i).   moments: host, [2][opt_itrs]: 1 - b1^(i+1) | 1 - b2^(i+1).
 *   sum_scaling: N / n_sub.
 * Refused while a fused gradient is pending or a run of any kind is open on the context; while this run is open every gradient
 * and every other run is refused (the table is beside bc_ctx_refuse_busy in csrc/bc_core.hip). */
int bc_psvi_many_begin(bc_ctx* ctx, const bc_data* data, int model, int sampler_kind, int32_t diag, const double* pts,
                       const double* w0, const int64_t* row_ptr, int32_t n_problems, const double* start, int32_t s,
                       int32_t opt_itrs, const double* steps, const double* moments, int64_t n_sub, double sum_scaling);
/* normals: host, k x S x D.   sub_idx: host, k x n_sub, local row numbers of `data`: one that is negative or >= the row count is
 * refused with BC_INVALID_ARGUMENT before anything of the chunk is enqueued, and fails the run: every later chunk is refused and
 * _end (all outputs NULL) closes it.  The host arrays have been read on return. */
int bc_psvi_many_chunk_begin(bc_ctx* ctx, const double* normals, const int64_t* sub_idx, int32_t k);
/* Waits for the chunk.  out_marked (or NULL): how many problems are marked so far.  Marked problems do not fail the run. */
int bc_psvi_many_chunk_end(bc_ctx* ctx, int32_t* out_marked);
/* Hands out the results and closes the run.  Callable after a failure with every output NULL (nothing is copied).
 *   out_w: sum m_p.   out_pts: (sum m_p) x D.   out_modes: P x D, the last step's modes.   out_status: P.
 * All four or none.  A marked problem's slices are left alone. */
int bc_psvi_many_end(bc_ctx* ctx, double* out_w, double* out_pts, double* out_modes, int32_t* out_status);
/* GPU milliseconds of the chunks of the last run, between HIP events around each chunk's steps (upload excluded). */
int bc_psvi_many_device_ms(bc_ctx* ctx, double* out_ms);

/* What the LAST EXECUTED STEP of the most recent run left in that run's own buffers -- a seam for tests; nothing is launched.
 * Valid once a chunk has been waited for: after _chunk_end and after _end, until the next _begin.  The snapshot of the state
 * before a step is taken by the last step of each chunk.  Refused with BC_INVALID_ARGUMENT when no run has been begun on the
 * context, while a chunk is pending, and when the shape arguments are not that run's.  Every output may be NULL.
 *   out_w_before: R.  out_pts_before: R x D.  out_mode: P x D.  out_theta: P x S x D.  out_target, out_resid: P x S.
 *   out_gw: R.  out_gp: R x D.  out_w, out_mom1_w, out_mom2_w: R.  out_pts, out_mom1_p, out_mom2_p: R x D.
 *   out_newton: P x 2: Newton steps of the last fit | of all fits of the run.   out_flag: P: 0, or 1 + the step that marked it.
 * Gaussian kind: out_theta is the draw Theta_p (not Theta'_p), out_mode is mu_p, out_newton is zero.
 * A marked problem's slices hold what its last executed stage left. */
int bc_psvi_many_last_step(bc_ctx* ctx, int64_t total_points, int32_t n_problems, int32_t d, int32_t s, double* out_w_before,
                           double* out_pts_before, double* out_mode, double* out_theta, double* out_target, double* out_resid,
                           double* out_gw, double* out_gp, double* out_w, double* out_pts, double* out_mom1_w, double* out_mom1_p,
                           double* out_mom2_w, double* out_mom2_p, int32_t* out_newton, int32_t* out_flag);

#ifdef __cplusplus
}
#endif
#endif /* BETA_CORES_PSVI_MANY_H */
