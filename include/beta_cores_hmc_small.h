/*
 * beta_cores_hmc_small.h -- C ABI of the batched sampler of libbeta_cores for MANY SMALL logistic posteriors at once: the
 * weighted coresets of an evaluation curve, each of at most a few hundred rows.
 *
 * An extension of include/beta_cores.h (same library, same conventions: int status, bc_last_error(), host pointers borrowed
 * for the call), modelled on beta_cores_hmc.h, whose target, sampler and limits it shares: plain HMC of
 *
 *   logjoint(theta) = sum_n w_n ll(-z_n . theta) - (D / 2) log(2 pi) - |theta|^2 / 2
 *
 * with a diagonal inverse mass, a step and a leapfrog count the caller chooses, on draws the HOST makes.  Bound in Python by
 * beta_cores_amd/_native.py (_HMC_SMALL_SIGNATURES).
 *
 * What differs is the shape of the work.  beta_cores_hmc.h serves ONE problem of any size with three launches per leapfrog
 * step; here one thread block serves one problem and one, two or four of its chains: it copies the problem's rows into the
 * LDS of its CU once per launch and runs a whole chunk of iterations there, every leapfrog step included (k_hmc_small,
 * csrc/bc_hmc_small.hip).  A chunk is ONE launch for all problems and chains; blocks never wait for each other, blocks beyond
 * the resident capacity queue.  How many chains share a block is the library's choice and changes no result.
 *
 * Problems are host arrays, packed:  rows: (sum_p n_p) x D float64, problem p's rows at row_ptr[p] .. row_ptr[p + 1] - 1;
 * w: one weight per row;  row_ptr: P + 1 entries, row_ptr[0] = 0, strictly increasing (every n_p >= 1).  D and the chain
 * count C are common to the batch.  A problem must fit one block's LDS: bc_hmc_small_fits is the capacity rule.
 *
 * Limits: 1 <= C <= BC_HMC_MAX_CHAINS, 1 <= D <= BC_HMC_MAX_DIM, every problem fits; anything else is refused with
 * BC_INVALID_ARGUMENT before a launch.  No row shards, no communicator, no device random-number generator.
 *
 * Reproducibility: every sum has a fixed order (over D: one ascending fma chain; over rows: segments of 64 rows, combined in
 * ascending order; no floating-point atomics).  The bits of a chain depend on its own problem, start, mass, step and draws
 * only -- not on P, on the problem's place in the batch, on the other problems, on the other chains or on how chains are
 * grouped into blocks.
 */
#ifndef BETA_CORES_HMC_SMALL_H
#define BETA_CORES_HMC_SMALL_H

#include "beta_cores_hmc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 when a problem of n rows and d columns fits one block's LDS (with one chain in the block) on the context's device (and
 * 1 <= n, 1 <= d <= BC_HMC_MAX_DIM), 0 otherwise: a flag, not a status.  On a device with 160 KiB of LDS per block:
 * (128, 128), (1000, 16) and (60, 256) fit. */
int bc_hmc_small_fits(bc_ctx* ctx, int64_t n, int32_t d);

/* The in-LDS pass on its own, prior included: out_value[p][c] = logjoint_p(theta[p][c]), out_grad[p][c] = its gradient.
 *   theta: host, P x C x D.   out_value: P x C, or NULL: the gradient-only pass of the inner leapfrog steps (no log1p).
 *   out_grad: P x C x D.   Refused, as _begin is, while a fused gradient is pending or a run of any
 *   kind (weight optimisation, beta_cores_hmc.h, this header) is open on the context. */
int bc_hmc_small_logjoint(bc_ctx* ctx, const double* rows, const double* w, const int64_t* row_ptr, int32_t n_problems, int32_t d,
                          const double* theta, int32_t c, double* out_value, double* out_grad);

/* A run in pieces.  _begin validates, uploads the problems, the start points and the inverse masses once, and enqueues the pass
 * that gives every chain its log-joint and gradient at the start; it does not wait.
 *   start: host, P x C x D.    inv_mass: host, P x D, finite and positive.    n_leapfrog >= 1.    n_iter: iterations of the run.
 * _chunk_begin uploads a chunk's draws in one transfer and enqueues its k iterations as one launch; the host arrays have been
 * read when it returns.
 *   step: host, P finite positive steps, one per problem (they may change from chunk to chunk).
 *   problem_stride = 0: all problems read the same normals (k x C x D) and log-uniforms (k x C): common random numbers.
 *   problem_stride >= k C D: problem p's normals begin at normals + p * problem_stride, its log-uniforms at log_u + p * k * C.
 * _chunk_end waits and copies the chunk's results:
 *   out_samples: P x k x C x D, the position of every chain after every iteration.   out_logjoint: P x k x C.
 *   out_accept: P x k x C (0 / 1).   out_status: P.   All four are required: a call without one leaves the chunk pending.
 * Per iteration and chain the arithmetic is that of beta_cores_hmc.h (csrc/bc_hmc_dev.h): accept iff H1 is finite and
 * log_u < H0 - H1; a rejected chain keeps its position, value and gradient bit for bit; a non-finite H1 is a rejection.  A start
 * whose log-joint or gradient is not finite marks ITS PROBLEM on the device: that problem's blocks return at once in every
 * later launch, out_status[p] = BC_NUMERICAL_PRECISION and nothing is copied for p; the other problems run on unaffected, with
 * out_status = BC_OK.  _chunk_end returns BC_OK whenever the call itself worked.
 * _end closes the run; call it after a failure too.
 * A run cannot begin while a fused gradient is pending, or a weight-optimisation run (beta_cores_viopt.h) or a run of
 * beta_cores_hmc.h or of this header is open on the context, and none of those (nor bc_logistic_logjoint_batch) can begin while
 * a run of this header is open.  (The whole table is beside bc_ctx_refuse_busy in csrc/bc_core.hip.) */
int bc_hmc_small_begin(bc_ctx* ctx, const double* rows, const double* w, const int64_t* row_ptr, int32_t n_problems, int32_t d,
                       const double* start, int32_t c, const double* inv_mass, int32_t n_leapfrog, int64_t n_iter);
int bc_hmc_small_chunk_begin(bc_ctx* ctx, const double* normals, const double* log_u, int64_t problem_stride, int32_t k,
                             const double* step);
int bc_hmc_small_chunk_end(bc_ctx* ctx, double* out_samples, double* out_logjoint, int32_t* out_accept, int32_t* out_status);
int bc_hmc_small_end(bc_ctx* ctx);
/* GPU milliseconds of the chunk launches of the last run, between HIP events around each (upload excluded). */
int bc_hmc_small_device_ms(bc_ctx* ctx, double* out_ms);

#ifdef __cplusplus
}
#endif
#endif /* BETA_CORES_HMC_SMALL_H */
