/*
 * beta_cores_viopt.h -- C ABI of the on-device weight optimisation of the greedy variational coresets in libbeta_cores.
 *
 * An extension of include/beta_cores.h (same library, same conventions: int status, bc_last_error(), host pointers
 * borrowed for the call); kept in a header of its own so that the ABI of the existing headers stays as it is.
 * Bound in Python by beta_cores_amd/_native.py (_VIOPT_SIGNATURES).
 *
 * beta-Cores and SparseVI run `opt_itrs` projected-ADAM steps on the coreset weights after every selected point
 * (bcores.py:141-150, sparsevi.py:129-136).  With bc_vi_gradient every step returns to the host three times: for the
 * posterior draw, for the gradient, for the ADAM arithmetic.  The entry points below enqueue whole runs of steps and wait once
 * per run.  One step is, on the context's stream, in order:
 *
 *   1. k_vi_sampler    Theta = mu_w + E . L_w^T from the coreset rows and the CURRENT weights (one block; Cholesky in LDS)
 *      k_vi_laplace    (logistic kind) the same draw around the mode of the weighted log-joint: a damped Newton solve in the
 *                      block, started at the previous step's mode, which stays on the device (beta_cores_vilaplace.h)
 *   2. K1              of the coreset rows, materialised
 *   3. k_take_rows     the step's sub-sample of the resident rows (when sub-sampled)
 *   4. K1, store-free  of the data rows
 *   5. the column-sum reduction
 *   6. k_vi_gradient   the M x S algebra
 *   7. k_vi_adam       w, mom1, mom2 <- one step of util/opt.py's nn_opt
 *
 * The normals E and the sub-sample indices are drawn by the HOST (NumPy's legacy stream, in the reference's order) and
 * uploaded per chunk of steps.  Results equal the host loop's to rounding (the Cholesky and E . L^T have neither LAPACK's nor
 * BLAS's bits), not bit for bit.
 *
 * Out of scope (the host loop serves them): the reference's BFGS mode search of the logistic sampler, feature encoders, groups,
 * row shards (communicators), learn_beta = True, and a device-side random number generator (it would leave the reference's
 * stream).
 */
#ifndef BETA_CORES_VIOPT_H
#define BETA_CORES_VIOPT_H

#include "beta_cores.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BC_VI_SAMPLER_LINREG 0      /* sampler_params = th0 [D] | Sig0inv [D][D] | sigsq;   rows [x (D), y] */
#define BC_VI_SAMPLER_GAUSS 1       /* sampler_params = mu0 [d] | Sig0inv [d][d] | Siginv [d][d];   rows x (d) */
#define BC_VI_SAMPLER_LOGISTIC 2    /* sampler_params = start [D] | diag flag (0.0 or 1.0);   rows z = y * x (D); prior N(0, I).
                                     * The Laplace approximation by damped Newton steps (samplers.logistic_laplace, solver='newton');
                                     * start: where the first step's search begins, every later step begins at the mode before it. */
#define BC_VI_MAX_DIM 128           /* largest D: the factor and its inverse share one work-group's LDS */
#define BC_VI_STAGE_BYTES (32u << 20)      /* automatic chunks keep the staged draws (normals + indices) of a chunk under this */

/* Steps per chunk that keep a chunk's draws under BC_VI_STAGE_BYTES (at least 1): returns a count, not a status. */
int bc_vi_optimize_auto_chunk(int32_t s, int32_t d, int64_t n_sub);

/* A run in pieces.  _begin validates everything but the indices and stages what is constant over the run (coreset rows, w0,
 * the step arrays, the sampler's parameters); nothing runs yet.  Per chunk: _chunk_begin checks the chunk's indices (one that is
 * negative or >= the row count is refused with BC_INVALID_ARGUMENT before anything of the chunk is enqueued), uploads its
 * draws in one transfer and enqueues its steps with plain stream launches; the host arrays have been read when it returns.
 * _chunk_end waits for them.  Between the two the host is free -- Python draws the next chunk there.  _end hands out the
 * weights (and the trace) and closes the run; call it after a failure too (out_w = NULL: nothing is copied).
 *   core_rows: host, m x dz doubles (dz = the data's column count).     w0: host, m.
 *   model / params: as bc_vi_gradient takes them (a value model: LINREG_LL/_BETA with the linreg sampler, GAUSS_LL/_BETA with
 *     the Gaussian one, LOGISTIC_LL (no params) / LOGISTIC_BETA ({beta, value at zero}) with the logistic one; any other pair
 *     is refused with BC_INVALID_ARGUMENT).  s <= 256, D <= BC_VI_MAX_DIM, m (dz + 1) <= 60000.
 *   step: host, [3][opt_itrs]: step_sched(i) | 1 - b1^(i+1) | 1 - b2^(i+1) with b1 = 0.9, b2 = 0.999, eps = 1e-8 (nn_opt).
 *   n_sub: rows per sub-sample, 0 = every step projects all rows of `data` (sum_scaling is then usually 1).
 *   normals: host, k x S x D.    sub_idx: host, k x n_sub (NULL iff n_sub == 0), local row numbers of `data`.
 * A pivot of the Cholesky that is not finite and positive marks the run on the device: the sampler and the ADAM kernel of
 * every later step return at once (the projections between them run on the previous Theta and their result is dropped),
 * _chunk_end returns BC_NUMERICAL_PRECISION and _end copies nothing.  The logistic kind marks the run the same way on a weight,
 * a value of the log-joint, a component of its gradient or a pivot that is not finite. */
int bc_vi_optimize_begin(bc_ctx* ctx, const bc_data* data, const double* core_rows, int64_t m, int model, const double* params,
                         int32_t n_params, int sampler_kind, const double* sampler_params, int32_t s, const double* w0,
                         int32_t opt_itrs, const double* step, int64_t n_sub, double sum_scaling, int want_trace);
int bc_vi_optimize_chunk_begin(bc_ctx* ctx, const double* normals, const int64_t* sub_idx, int32_t k);
int bc_vi_optimize_chunk_end(bc_ctx* ctx);
int bc_vi_optimize_end(bc_ctx* ctx, double* out_w, double* out_trace);
/* GPU milliseconds of the chunks of the last run, between HIP events around each chunk's steps (upload excluded). */
int bc_vi_optimize_device_ms(bc_ctx* ctx, double* out_ms);

/* What the last executed k_vi_sampler of the most recent run left in that run's own buffers -- a seam for tests of the draw;
 * nothing is launched.  Valid once a run has been begun and no chunk is pending: after _chunk_end and after _end, until the next
 * _begin (before the run's first chunk everything reads 0).  Refused with BC_INVALID_ARGUMENT when no run has ever been begun on
 * the context, while a chunk is pending, and when s / d are not that run's S / D.
 *   out_theta: s x d, rows < S and columns < D of the zero-padded Theta block K1 reads (Gaussian kind: Theta' = Theta . Siginv^T).
 *   out_saux: s, or NULL (Gaussian kind: theta^T Siginv theta per sample; else 0).
 *   out_raw: s x d, or NULL (Gaussian kind: the draw before Siginv is applied; else 0).
 *   out_pad_max: the largest |value| of every OTHER element of that block and of the rows >= S of saux (NaN if one of them is
 *     NaN).  _begin zero-fills them, the kernel never writes there and K1 relies on it: anything but 0 is a defect.
 * After a run that failed in its first step (BC_NUMERICAL_PRECISION) all of it reads 0: the sampler writes nothing then. */
int bc_vi_optimize_last_draw(bc_ctx* ctx, int32_t s, int32_t d, double* out_theta, double* out_saux, double* out_raw,
                             double* out_pad_max);

/* The whole run in one call: the four above, chunk after chunk.  chunk_steps: 0 = bc_vi_optimize_auto_chunk.
 *   out_w: m (left alone unless the call returns BC_OK).   out_trace: opt_itrs x m, the weights after every step, or NULL. */
int bc_vi_optimize(bc_ctx* ctx, const bc_data* data, const double* core_rows, int64_t m, int model, const double* params,
                   int32_t n_params, int sampler_kind, const double* sampler_params, int32_t s, const double* w0,
                   int32_t opt_itrs, const double* step, const double* normals, const int64_t* sub_idx, int64_t n_sub,
                   double sum_scaling, int32_t chunk_steps, double* out_w, double* out_trace);

#ifdef __cplusplus
}
#endif
#endif /* BETA_CORES_VIOPT_H */
