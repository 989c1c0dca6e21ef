/*
 * beta_cores_hmc.h -- C ABI of the exact-posterior sampler of libbeta_cores: multi-chain HMC of the logistic posterior of
 * resident rows, and the multi-chain rows pass under it.
 *
 * An extension of include/beta_cores.h (same library, same conventions: int status, bc_last_error(), host pointers
 * borrowed for the call), modelled on beta_cores_viopt.h.  Bound in Python by beta_cores_amd/_native.py (_HMC_SIGNATURES).
 *
 * The target is the reference's weighted log-joint with the N(0, I) prior (model_lr.py:88-93) of rows z = y * x (no y
 * column, the intercept a column of the rows):
 *
 *   logjoint(theta) = sum_n w_n ll(-z_n . theta) - (D / 2) log(2 pi) - |theta|^2 / 2
 *
 * The sampler is plain HMC -- not NUTS, no dual averaging -- with a diagonal inverse mass, a step and a leapfrog count the
 * caller chooses; C chains advance in lock-step.  One leapfrog step is, on the context's stream: the multi-chain rows pass
 * k_lr_rows_mc (value and gradient of the likelihood for all C chains from ONE read of the rows, on the fp64 matrix cores),
 * the block-order reduction of its partials, and one small update kernel (csrc/bc_hmc_dev.h).  The normals and the log-uniforms
 * are drawn by the HOST (NumPy's stream) and uploaded per chunk of iterations; between a chunk's upload and its single wait
 * nothing returns to the host.
 *
 * Limits of this version: 1 <= C <= BC_HMC_MAX_CHAINS, 1 <= D <= BC_HMC_MAX_DIM; anything else is refused with
 * BC_INVALID_ARGUMENT before a launch.  No row shards, no communicator, no device random-number generator.
 *
 * Reproducibility: every reduction has a fixed order (no floating-point atomics).  A repeated call returns the same bits, and
 * the bits of chain c depend neither on which other chains share the batch nor on how many.
 */
#ifndef BETA_CORES_HMC_H
#define BETA_CORES_HMC_H

#include "beta_cores.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BC_HMC_MAX_CHAINS 64
#define BC_HMC_MAX_DIM 256
#define BC_HMC_STAGE_BYTES (32u << 20)     /* automatic chunks keep a chunk's staged draws under this (= BC_VI_STAGE_BYTES) */

/* The rows pass on its own, prior included: out_value[c] = logjoint(theta_c), out_grad[c] = its gradient, c < C.
 *   data: rows z = y * x, float64 or float32.   w: n x 1 float64 rows, or NULL (all ones).   theta: host, C x D.
 *   out_value: C, or NULL: the gradient-only pass the inner leapfrog steps run (no log1p per element).
 * Refused while a run of this header or of beta_cores_hmc_small.h is open on the context; a pending fused gradient and an open
 * weight-optimisation run do not refuse it. */
int bc_logistic_logjoint_batch(bc_ctx* ctx, const bc_data* data, const bc_data* w, const double* theta, int32_t c,
                               double* out_value, double* out_grad);

/* Iterations per chunk that keep a chunk's draws (normals C x D and log-uniforms C per iteration) under BC_HMC_STAGE_BYTES
 * (at least 1): returns a count, not a status. */
int bc_hmc_auto_chunk(int32_t c, int32_t d);

/* A run in pieces.  _begin validates, stages the start points and the inverse mass, and enqueues the pass that gives every
 * chain its log-joint and gradient at the start; it does not wait.
 *   start: host, C x D.    inv_mass: host, D, finite and positive.    n_leapfrog >= 1.    n_iter: iterations of the whole run.
 * Per chunk: _chunk_begin uploads the chunk's draws in one transfer and enqueues its k iterations (the step may differ from
 * chunk to chunk: the host's warm-up rule lives between chunks); the host arrays have been read when it returns.  _chunk_end
 * waits and copies the chunk's results:
 *   normals: host, k x C x D.    log_u: host, k x C, logarithms of uniforms.
 *   out_samples: k x C x D, the position of every chain after every iteration.    out_logjoint: k x C.    out_accept: k x C (0 / 1).
 *   All three are required: a call without one is refused and leaves the chunk pending.
 * Per iteration and chain: momentum r = E / sqrt(inv_mass); H0 = -logjoint + sum inv_mass r^2 / 2; n_leapfrog leapfrog steps;
 * H1 likewise; accept iff H1 is finite and log_u < H0 - H1.  An accepted chain takes the proposal with the value and gradient
 * computed at it; a rejected chain keeps its position, value and gradient bit for bit.  A non-finite H1 is a rejection, not an
 * error.  A start whose log-joint or gradient is not finite -- a non-finite weight shows there -- marks the run on the device:
 * every later kernel of the run returns at once, _chunk_end returns BC_NUMERICAL_PRECISION and copies nothing.
 * _end closes the run; call it after a failure too.
 * A run cannot begin while a fused gradient (any kind: the _gradient_begin / _end pairs) is pending or a weight-optimisation run
 * (beta_cores_viopt.h), another run of this header or a run of beta_cores_hmc_small.h is open on the context, and none of those
 * can begin while an HMC run is open: BC_INVALID_ARGUMENT.  (The whole table -- who is refused while what is held -- is beside
 * bc_ctx_refuse_busy in csrc/bc_core.hip.) */
int bc_hmc_begin(bc_ctx* ctx, const bc_data* data, const bc_data* w, const double* start, int32_t c, const double* inv_mass,
                 int32_t n_leapfrog, int64_t n_iter);
int bc_hmc_chunk_begin(bc_ctx* ctx, const double* normals, const double* log_u, int32_t k, double step_size);
int bc_hmc_chunk_end(bc_ctx* ctx, double* out_samples, double* out_logjoint, int32_t* out_accept);
int bc_hmc_end(bc_ctx* ctx);
/* GPU milliseconds of the chunks of the last run, between HIP events around each chunk's iterations (upload excluded). */
int bc_hmc_device_ms(bc_ctx* ctx, double* out_ms);

/* The whole run in one call with one step size: the four above, chunk after chunk.  chunk_steps: 0 = bc_hmc_auto_chunk.
 *   normals: n_iter x C x D.   log_u: n_iter x C.   Outputs as _chunk_end's with k = n_iter; on a failure what they hold is
 *   unspecified (nothing of the failing chunk is copied). */
int bc_hmc_logistic(bc_ctx* ctx, const bc_data* data, const bc_data* w, const double* start, int32_t c, const double* inv_mass,
                    int32_t n_leapfrog, double step_size, int64_t n_iter, const double* normals, const double* log_u,
                    int32_t chunk_steps, double* out_samples, double* out_logjoint, int32_t* out_accept);

#ifdef __cplusplus
}
#endif
#endif /* BETA_CORES_HMC_H */
