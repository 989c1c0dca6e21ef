/*
 * beta_cores_hmc_adapt.h -- C ABI of the per-chain warm-up of the batched small-problem sampler (beta_cores_hmc_small.h):
 * every chain adapts its own step by dual averaging and its own diagonal inverse mass in windows, as Stan's warm-up does,
 * inside the block that runs it.  No NUTS, no step-size search at a restart, no step jitter.
 *
 * An extension of include/beta_cores.h (same library, same conventions: int status, bc_last_error(), host pointers borrowed
 * for the call).  Bound in Python by beta_cores_amd/_native.py (_HMC_ADAPT_SIGNATURES).  These are entry points ON AN OPEN RUN
 * of beta_cores_hmc_small.h: that header's _begin opens it and its _end closes it; there is no new kind of run.
 *
 * Per chain the state is x = log(step), its average xbar, hbar, mu, a counter t, the inverse mass im[D] and the running mean and
 * M2 of the positions of the current window.  A warm-up iteration runs with step exp(x) and im; then, with dh = H0 - H1,
 *   alpha = 0 where H1 is not finite, 1 where dh >= 0, exp(dh) otherwise (exactly 0 below -700)
 *   t += 1;  hbar = (1 - 1/(t + t0)) hbar + (delta - alpha) / (t + t0);  x = mu - hbar sqrt(t) / gamma;
 *   xbar = (1 - t^-kappa) xbar + t^-kappa x
 * An iteration of a slow window folds the chain's position after it (accepted or kept) into mean and M2; a window's last
 * iteration sets, with nw >= 2 folded positions, im_k = (nw / (nw + 5)) M2_k / (nw - 1) + 1e-3 * 5 / (nw + 5) (with fewer the
 * mass stays), empties the sums and restarts the averaging: mu = log 10 + x, hbar = xbar = 0, t = 0.  Kept iterations run at
 * exp(xbar) -- exp(x) where t = 0 -- and the adapted im, both frozen.  The windows are Stan's (csrc/bc_hmc_adapt_plan.h).
 *
 * The leapfrog and accept arithmetic is that of beta_cores_hmc_small.h, and so are the draws, the marking of problems and the
 * reproducibility: a chain's bits depend on its own problem, start, mass, step and draws only, and not on how the warm-up is
 * cut into chunks.  The adaptation uses no communication between blocks.
 */
#ifndef BETA_CORES_HMC_ADAPT_H
#define BETA_CORES_HMC_ADAPT_H

#include "beta_cores_hmc_small.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The plan of a warm-up of n_warmup iterations: out_flags[i] (bit 0: iteration i folds its position, bit 1: it ends a window) and
 * out_coef[i] = 1 / (t + t0) | sqrt(t) / gamma | t^-kappa with t the iterations since the last window end, i counted.  Needs no
 * context.  n_warmup >= 0, the buffers >= 0, base_window >= 1, gamma > 0, t0 >= 0, kappa > 0; out_flags: n_warmup, out_coef:
 * n_warmup x 3 (both may be NULL only with n_warmup = 0).  With n_warmup < 20 no iteration folds or ends a window. */
int bc_hmc_adapt_plan(int32_t n_warmup, int32_t init_buffer, int32_t term_buffer, int32_t base_window, double gamma, double t0,
                      double kappa, int32_t* out_flags, double* out_coef);

/* Starts the warm-up of the open run, before its first chunk: every chain of problem p begins with x = log_step[p] (host, P finite
 * numbers), mu = log 10 + x, and the inverse mass the run was begun with.  0 < delta < 1: the target of the mean alpha.
 * Stan's constants: gamma 0.05, t0 10, kappa 0.75, delta 0.8, buffers 75 / 50 / 25.  1 <= n_warmup <= the run's iterations. */
int bc_hmc_adapt_begin(bc_ctx* ctx, const double* log_step, double delta, double gamma, double t0, double kappa, int32_t n_warmup,
                       int32_t init_buffer, int32_t term_buffer, int32_t base_window);
/* The next k warm-up iterations in ONE launch; draws and problem_stride as the _chunk_begin of beta_cores_hmc_small.h has them.
 * The chunks of a warm-up may be cut anywhere: no bit depends on it.  More iterations than n_warmup are refused. */
int bc_hmc_adapt_chunk_begin(bc_ctx* ctx, const double* normals, const double* log_u, int64_t problem_stride, int32_t k);
/* Waits for that chunk.  out_samples: P x k x C x D or NULL (not copied); out_logjoint, out_accept: P x k x C; out_status: P;
 * out_step: P x k x C, the step every iteration ran with; out_alpha: P x k x C.  All but out_samples are required: a call
 * without one leaves the chunk pending.  Marked problems as in that header's _chunk_end: nothing is copied for them. */
int bc_hmc_adapt_chunk_end(bc_ctx* ctx, double* out_samples, double* out_logjoint, int32_t* out_accept, int32_t* out_status,
                           double* out_step, double* out_alpha);
/* A chunk of k kept iterations at every chain's frozen step and inverse mass.  It is pending like a chunk of
 * beta_cores_hmc_small.h: that header's _chunk_end, the chunk scores of beta_cores_score.h and the chunk fold of beta_cores_diag.h
 * serve it unchanged.  Refused before bc_hmc_adapt_begin. */
int bc_hmc_adapted_chunk_begin(bc_ctx* ctx, const double* normals, const double* log_u, int64_t problem_stride, int32_t k);
/* The chains' frozen steps (P x C) and inverse masses (P x C x D) as they stand; no chunk may be pending.  Waits.  The entries of
 * a marked problem are those it began with. */
int bc_hmc_adapt_state(bc_ctx* ctx, double* out_step, double* out_inv_mass);

#ifdef __cplusplus
}
#endif
#endif /* BETA_CORES_HMC_ADAPT_H */
