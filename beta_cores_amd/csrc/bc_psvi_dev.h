// The point-gradient of BatchPSVICoreset (bayesiancoresets/coreset/bpsvi.py:47-57) for ONE pseudo-point, for one thread block:
//
//   g_p[i, c] = -(1/S) sum_s w_i * r_s * G[i, s, c],      G = the x-gradient tensor of the log-likelihood, centred over c
//
// without the M x S x W tensor.  Centring over the coordinate axis (projector.py:31) commutes with the sum over the samples:
//
//   g_p[i, c] = -(w_i / S) * ( V[i, c] - mean_c V[i, :] ),     V[i, c] = sum_s r_s * Gu[i, s, c]      (Gu: un-centred)
//
//   linear regression  (model_linreg.py:12-17, rows [x, y], W = D + 1):  Gu[i,s,:] = fac_is [th_s, 1],  fac = 1/sigsq (y - x.th_s)
//   logistic regression (model_lr.py:107-114, rows z = y*x, W = D):       Gu[i,s,:] = fac_is th_s,       m = -z.th_s,
//                                                                         fac = (m < 100) ? e^m / (1 + e^m) : 1
//   Gaussian location   (gaussian.py:17-20, rows x, W = d):               Gu[i,s,:] = th_s.Siginv - x_i.Siginv
//
// so with coef_s = r_s fac_is (Gaussian: coef_s = r_s) every model is  V[i, c] = sum_s coef_s T[s, c]  (c < D) for the Theta T
// that K1's staging already holds -- row pitch dk, for the Gaussian model T = Theta' = (Siginv . Theta^T)^T, which is Theta . Siginv
// for the symmetric Siginv a precision matrix is --, plus  V[i, D] = sum_s coef_s  (linear regression's last coordinate)  and
// V[i, c] -= (sum_s r_s) (x_i . Siginv)[c]  (Gaussian).  sum_s r_s Theta'_s is the same for every point; each block forms it
// itself in the chain the other two models run anyway: S D fmas beside the other blocks, no launch in front of the M groups.
//
// fac_is is k_grad_x's expression operation for operation (csrc/bc_gradx.hip), the branch at 100 included.
//
// Written the way bc_vi_sampler_dev.h / bc_nnls_dev.h are: "element = tid, tid + nt, ...", barriers between phases, every sum a
// fixed-order fma chain of one thread or a fixed-order wave / block reduction, so a run is bit-reproducible and the same text
// compiles for the host with one thread, one lane and empty barriers (tests/psvi_grad_harness.cpp).
#pragma once
#include <math.h>
#include <stddef.h>

#define BC_PSVI_LINREG 0
#define BC_PSVI_LOGISTIC 1
#define BC_PSVI_GAUSS 2
#define BC_PSVI_MAX_DZ 3840                                  // widest row: the work space stays within 64 KiB of LDS
#define BC_PSVI_RED 17                                       // doubles of the block reduction's scratch (bc_block_sum)
#define BC_PSVI_WS_DOUBLES(dz, s) (2 * (size_t)(dz) + (size_t)(s) + BC_PSVI_RED)

#ifndef BC_PSVI_FN
#define BC_PSVI_FN __device__
#define BC_PSVI_TID ((int)threadIdx.x)
#define BC_PSVI_NT ((int)blockDim.x)
#define BC_PSVI_LANES 64                                     // a sample's dot product is spread over one wave
#define BC_PSVI_SYNC() __syncthreads()
#define BC_PSVI_WAVE_SUM(v) bc_wave_sum_all(v)               // the total in every lane, fixed order
#define BC_PSVI_BLOCK_SUM(v, red) bc_block_sum(v, red)       // the total in every thread, fixed order
#endif

struct PsviArgs {
  int kind;               // BC_PSVI_LINREG / _LOGISTIC / _GAUSS
  int m, s, d, dz, dk;    // points, samples, dimension of theta, row width (= W, the coordinates of g_p), row pitch of theta
  const double* pts;      // [m][dz]
  const double* w;        // [m]
  const double* theta;    // [.][dk], rows q < s, columns a < d: Theta (Gaussian: Theta')
  const double* siginv;   // [d][d] (Gaussian)
  const double* resid;    // [s]
  double sigsq;           // (linear regression)
  double* out;            // [m][dz]
};

// ws: BC_PSVI_WS_DOUBLES(dz, s) doubles.
BC_PSVI_FN inline void bc_psvi_point_grad(const PsviArgs& a, int i, double* ws) {
  const int tid = BC_PSVI_TID, nt = BC_PSVI_NT;
  const int lane = tid % BC_PSVI_LANES, wave = tid / BC_PSVI_LANES, nw = nt / BC_PSVI_LANES;
  const int d = a.d, dz = a.dz, s = a.s, dk = a.dk;
  double* x = ws;                   // [dz] this point's row
  double* coef = x + dz;            // [s]
  double* v = coef + s;             // [dz] V[i, :]
  double* red = v + dz;             // [BC_PSVI_RED]
  for (int k = tid; k < dz; k += nt) x[k] = a.pts[(size_t)i * dz + k];
  BC_PSVI_SYNC();
  // ---- phase 1: coef_s = r_s fac_is, one wave per sample in turn
  if (a.kind == BC_PSVI_GAUSS) {
    for (int q = tid; q < s; q += nt) coef[q] = a.resid[q];
  } else {
    for (int q = wave; q < s; q += nw) {
      const double* th = a.theta + (size_t)q * dk;
      double p = 0.;
      for (int k = lane; k < d; k += BC_PSVI_LANES) p = fma(x[k], th[k], p);
      p = BC_PSVI_WAVE_SUM(p);
      double fac;
      if (a.kind == BC_PSVI_LINREG) {
        fac = 1. / a.sigsq * (x[d] - p);
      } else {
        const double mm = -p;
        fac = (mm < 100.) ? exp(mm) / (1. + exp(mm)) : 1.;
      }
      if (lane == 0) coef[q] = a.resid[q] * fac;
    }
  }
  BC_PSVI_SYNC();
  // ---- phase 2: thread t owns the coordinates t, t + nt, ...: the S-term chain in ascending s over row-major Theta
  double part = 0.;
  for (int c = tid; c < dz; c += nt) {
    double acc = 0.;
    if (c < d) {
      int q = 0;
      for (; q + 8 <= s; q += 8) {          // same chain, eight loads in flight
        double t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = a.theta[(size_t)(q + u) * dk + c];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = fma(coef[q + u], t[u], acc);
      }
      for (; q < s; ++q) acc = fma(coef[q], a.theta[(size_t)q * dk + c], acc);
      if (a.kind == BC_PSVI_GAUSS) {
        double cs = 0., xs = 0.;
        for (int q2 = 0; q2 < s; ++q2) cs += coef[q2];
        for (int k = 0; k < d; ++k) xs = fma(x[k], a.siginv[(size_t)k * d + c], xs);      // (x_i . Siginv)[c]
        acc -= cs * xs;
      }
    } else {
      for (int q = 0; q < s; ++q) acc += coef[q];      // linear regression's last coordinate
    }
    v[c] = acc;
    part += acc;
  }
  // ---- phase 3: the mean over the W coordinates (fixed-order block reduction), the centred and scaled row
  const double mean = BC_PSVI_BLOCK_SUM(part, red) / (double)dz;
  const double scale = -(a.w[i] / (double)s);
  for (int c = tid; c < dz; c += nt) a.out[(size_t)i * dz + c] = scale * (v[c] - mean);
}
