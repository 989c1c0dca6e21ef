// The leapfrog and accept arithmetic of the multi-chain HMC run (include/beta_cores_hmc.h), for ONE chain and one thread block.
//
// Target: the reference's weighted logistic log-joint with the N(0, I) prior (model_lr.py:88-93),
//
//   logjoint(theta) = sum_n w_n ll(-z_n . theta) - (D / 2) log(2 pi) - |theta|^2 / 2
//   gradient        = sum_n w_n p(-z_n . theta) z_n - theta
//
// whose sums over the rows come from the rows pass (`red`: value | grad [D] of one chain).  One HMC iteration with a diagonal
// inverse mass im[D], step eps and L leapfrog steps is
//
//   bc_hmc_start_chain     r = E / sqrt(im);  H0 = -logjoint(theta) + sum im r^2 / 2;  r += eps/2 g;  theta' = theta + eps im r
//   bc_hmc_inner_chain     (L - 1 times, after a rows pass at theta')   g' = grad(theta');  r += eps g';  theta' += eps im r
//   bc_hmc_last_chain      (after the L-th rows pass, with value)       r += eps/2 g';  H1;  accept iff H1 is finite and
//                                                                       logU < H0 - H1;  an accepted chain takes theta', its
//                                                                       log-joint and its gradient, a rejected one keeps its own
//
// Written the way bc_vi_sampler_dev.h is: every loop over the D coordinates is "element k = tid, tid + nt, ...", barriers between
// phases, and every sum over the coordinates is ONE fixed-order fma chain of thread 0 over terms the other threads left in the
// work space (LDS on the device) -- so a chain's bits depend on nothing but its own inputs, and the same text compiles for the
// host with tid = 0, nt = 1 and an empty barrier (tests/hmc_harness.cpp, against the long-double restatement of
// tests/hmc_cases.py).
#pragma once
#include <math.h>

#define BC_HMC_MAX_CHAINS 64
#define BC_HMC_MAX_DIM 256
#define BC_HMC_WS_DOUBLES(d) (2 * (d) + 2)             // the work space of the functions below

#ifndef BC_HMC_FN
#define BC_HMC_FN __device__
#define BC_HMC_TID ((int)threadIdx.x)
#define BC_HMC_NT ((int)blockDim.x)
// (values one thread of the block wrote to device memory are read by the others after a barrier)
#define BC_HMC_SYNC() do { __threadfence_block(); __syncthreads(); } while (0)
#endif

BC_HMC_FN inline int bc_hmc_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }      // (false for NaN)

// lj = logjoint, g = its gradient at th from the rows' sums red = value | grad [d].  half_d_log_2pi: (d / 2) log(2 pi), evaluated
// once by the host.  Returns 1 (block-uniform) when the log-joint or a component of the gradient is not finite.
BC_HMC_FN inline int bc_hmc_logjoint_chain(const double* red, const double* th, int d, double half_d_log_2pi, double* lj, double* g,
                                           double* ws) {
  const int tid = BC_HMC_TID, nt = BC_HMC_NT;
  for (int k = tid; k < d; k += nt) {
    const double t = th[k], gk = red[1 + k] - t;
    g[k] = gk;
    ws[k] = t;
    ws[d + k] = bc_hmc_finite(gk) ? 0. : 1.;
  }
  BC_HMC_SYNC();
  if (tid == 0) {
    double ss = 0., bad = 0.;
    for (int k = 0; k < d; ++k) {
      ss = fma(ws[k], ws[k], ss);
      bad += ws[d + k];
    }
    const double v = (red[0] - half_d_log_2pi) - 0.5 * ss;
    *lj = v;
    ws[2 * d] = (bad != 0. || !bc_hmc_finite(v)) ? 1. : 0.;
  }
  BC_HMC_SYNC();
  const int r = ws[2 * d] != 0.;
  BC_HMC_SYNC();
  return r;
}

// The momentum draw, H0, the first half step of the momentum and the first position step.
BC_HMC_FN inline void bc_hmc_start_chain(const double* th, const double* lj, const double* g, const double* e, const double* im,
                                         double eps, int d, double* r, double* thp, double* h0, double* ws) {
  const int tid = BC_HMC_TID, nt = BC_HMC_NT;
  const double he = 0.5 * eps;
  for (int k = tid; k < d; k += nt) {
    const double r0 = e[k] / sqrt(im[k]);
    ws[k] = im[k] * r0;
    ws[d + k] = r0;
    const double r1 = fma(he, g[k], r0);
    r[k] = r1;
    thp[k] = fma(eps, im[k] * r1, th[k]);
  }
  BC_HMC_SYNC();
  if (tid == 0) {
    double kin = 0.;
    for (int k = 0; k < d; ++k) kin = fma(ws[k], ws[d + k], kin);
    *h0 = -*lj + 0.5 * kin;
  }
  BC_HMC_SYNC();
}

// A full step of the momentum with the gradient at thp, then the next position step.
BC_HMC_FN inline void bc_hmc_inner_chain(const double* red, double eps, const double* im, int d, double* r, double* thp) {
  const int tid = BC_HMC_TID, nt = BC_HMC_NT;
  for (int k = tid; k < d; k += nt) {
    const double gk = red[1 + k] - thp[k];
    const double r1 = fma(eps, gk, r[k]);
    r[k] = r1;
    thp[k] = fma(eps, im[k] * r1, thp[k]);
  }
}

// The trajectory's end: the last half step of the momentum, H1 and the decision.  Returns 1 (block-uniform) when the proposal
// is accepted (th, lj, g then hold the proposal's), 0 when it is rejected (they are not written at all).  gp [d], ljp [1]: scratch.
// ws[2 d + 1] holds H0 - H1 on return (not finite where H1 is not).
BC_HMC_FN inline int bc_hmc_last_chain(const double* red, double eps, const double* im, int d, double half_d_log_2pi, const double* h0,
                                       double logu, const double* r, const double* thp, double* gp, double* ljp, double* th,
                                       double* lj, double* g, double* ws) {
  const int tid = BC_HMC_TID, nt = BC_HMC_NT;
  const double he = 0.5 * eps;
  (void)bc_hmc_logjoint_chain(red, thp, d, half_d_log_2pi, ljp, gp, ws);
  for (int k = tid; k < d; k += nt) {
    const double r1 = fma(he, gp[k], r[k]);
    ws[k] = im[k] * r1;
    ws[d + k] = r1;
  }
  BC_HMC_SYNC();
  if (tid == 0) {
    double kin = 0.;
    for (int k = 0; k < d; ++k) kin = fma(ws[k], ws[d + k], kin);
    const double h1 = -*ljp + 0.5 * kin;
    ws[2 * d] = (bc_hmc_finite(h1) && logu < *h0 - h1) ? 1. : 0.;
    ws[2 * d + 1] = *h0 - h1;      // (handed out in addition, for the warm-up of bc_hmc_adapt_dev.h; thread 0 reads it back)
  }
  BC_HMC_SYNC();
  const int acc = ws[2 * d] != 0.;
  if (acc) {
    for (int k = tid; k < d; k += nt) {
      th[k] = thp[k];
      g[k] = gp[k];
    }
    if (tid == 0) *lj = *ljp;
  }
  BC_HMC_SYNC();
  return acc;
}
