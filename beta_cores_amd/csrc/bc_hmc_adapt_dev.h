// The per-chain warm-up arithmetic of the batched small-problem HMC run (include/beta_cores_hmc_adapt.h): Stan's dual averaging
// of the step and its windowed estimate of a diagonal metric, for ONE chain, applied after bc_hmc_last_chain.  Written as
// bc_hmc_dev.h is written: element k = tid, tid + nt, ...; every scalar recurrence is thread 0's; the same text compiles for the
// host with tid = 0 (tests/hmc_adapt_harness.cpp, against the long-double restatement of tests/hmc_adapt_cases.py).
//
// A chain's state: the scalars x (= log eps) | xbar | hbar | mu | t | nw (bc_hmc_adapt_scalars), its inverse mass im [d], and the running
// mean [d] and M2 [d] of the positions of the current window (Welford).  One warm-up iteration runs with eps = exp(x) and im; then
//
//   dh = H0 - H1;   alpha = 0 if dh is not finite (a non-finite H1), 1 if dh >= 0, 0 if dh < -700, else exp(dh)
//   t += 1;   hbar = (1 - eta) hbar + eta (delta - alpha);   x = mu - hbar sg;   xbar = (1 - zeta) xbar + zeta x
//   fold (BC_HMC_ADAPT_FOLD):   nw += 1;  dk = th_k - mean_k;  mean_k += dk / nw;  M2_k += dk (th_k - mean_k)      (the position AFTER the
//                               iteration, accepted or kept)
//   window end (BC_HMC_ADAPT_WEND):   if nw >= 2:  im_k = (nw / (nw + 5)) (M2_k / (nw - 1)) + 1e-3 (5 / (nw + 5))
//                               mean = M2 = 0, nw = 0;   mu = log 10 + x;   hbar = xbar = 0;   t = 0
//
// with eta, sg = sqrt(t) / gamma, zeta = t^-kappa and the flags from the plan (bc_hmc_adapt_plan.h) and log 10 from the host: no
// transcendental is evaluated here but exp, and that is ONE plain-C text on the device and on the host (bc_np_exp.h's main
// path), so the harness and the kernel evaluate the same operations.  Kept iterations run at exp(xbar) -- exp(x) where t = 0 --
// and the adapted im, both frozen (bc_hmc_adapt_frozen_log_step).
//
// t and nw follow the plan alone, so they are the same numbers in every thread of a slot and every chain of a run: each thread
// keeps its own copy in a register, and the branches below that hold no barrier may as well be per thread.
#pragma once
#include "bc_np_exp.h"
#include "bc_hmc_adapt_plan.h"      // BC_HMC_ADAPT_FOLD, BC_HMC_ADAPT_WEND: the flags of an iteration

#define BC_HMC_ADAPT_STATE 8      // doubles per chain in memory: x | xbar | hbar | mu | t | nw | - | -
// the same in registers: members, not an array -- `t == 0 ? x : xbar` on an array becomes a select of addresses, and the array
// then lives in scratch memory
struct bc_hmc_adapt_scalars {
  double x, xbar, hbar, mu, t, nw;
};

#ifndef BC_HMC_FN
#define BC_HMC_FN __device__
#define BC_HMC_TID ((int)threadIdx.x)
#define BC_HMC_NT ((int)blockDim.x)
#define BC_HMC_SYNC() do { __threadfence_block(); __syncthreads(); } while (0)
#endif

// exp(x) for |x| < 707.7: bc_np_exp's main path.  Beyond it: 0 or +inf by the sign (NaN stays NaN).  (BC_HD: the library's host
// side evaluates the frozen step with the same text, bc_hmc_adapt_state.)
BC_HD double bc_hmc_adapt_exp(double x) {
  int covered;
  const double e = bc_np_exp(x, &covered);
  if (covered) return e;
  return x > 0. ? INFINITY : (x < 0. ? 0. : x);
}

// the acceptance statistic of a proposal from dh = H0 - H1
BC_HD double bc_hmc_adapt_alpha(double dh) {
  if (!(fabs(dh) <= 1.7976931348623157e308)) return 0.;      // (H1 is not finite; NaN too)
  if (dh >= 0.) return 1.;
  if (dh < -700.) return 0.;
  return bc_hmc_adapt_exp(dh);
}

// the dual-averaging update of one chain's scalars: thread 0's
BC_HMC_FN inline void bc_hmc_adapt_step_size(double alpha, double delta, double eta, double sg, double zeta, bc_hmc_adapt_scalars* st) {
  const double hbar = (1. - eta) * st->hbar + eta * (delta - alpha);
  const double x = st->mu - hbar * sg;
  st->hbar = hbar;
  st->x = x;
  st->xbar = (1. - zeta) * st->xbar + zeta * x;
}

// the restart of the step's averaging at a window end: thread 0's
BC_HMC_FN inline void bc_hmc_adapt_restart(double log10, bc_hmc_adapt_scalars* st) {
  st->mu = log10 + st->x;
  st->xbar = st->hbar = 0.;
}

// the position th [d] folded into mean [d], m2 [d] as sample number nw (>= 1, this one counted): element k by its thread
BC_HMC_FN inline void bc_hmc_adapt_fold(const double* th, int d, double nw, double* mean, double* m2) {
  const int tid = BC_HMC_TID, nt = BC_HMC_NT;
  for (int k = tid; k < d; k += nt) {
    const double q = th[k], dk = q - mean[k], m = mean[k] + dk / nw;
    mean[k] = m;
    m2[k] = m2[k] + dk * (q - m);
  }
}

// a window's end for the vectors: the regularised variance of nw samples becomes the inverse mass (nw < 2: it stays), and the
// running sums restart.  Element k by its thread; im is read by the other threads after the caller's barrier.
BC_HMC_FN inline void bc_hmc_adapt_window_end(int d, double nw, double* mean, double* m2, double* im) {
  const int tid = BC_HMC_TID, nt = BC_HMC_NT;
  const double a = nw / (nw + 5.), b = 1e-3 * (5. / (nw + 5.));
  for (int k = tid; k < d; k += nt) {
    if (nw >= 2.) im[k] = a * (m2[k] / (nw - 1.)) + b;
    mean[k] = 0.;
    m2[k] = 0.;
  }
}

// log of the step of the kept iterations: the averaged iterate, or the last one where none has been averaged since a restart
BC_HD double bc_hmc_adapt_frozen_log_step(double x, double xbar, double t) { return t == 0. ? x : xbar; }
