// The posterior draw and the ADAM update of the greedy-VI weight optimisation, for one thread block.
//
//   Theta = mu + E . L^T      with  A = chol-factorable D x D,  C = chol(A) (lower),  L = C^-1,  mu = (L . L^T) . rhs
//
// is what the samplers of beta_cores_amd/samplers.py hand to K1 once per gradient (posterior.weighted_post /
// gaussian_weighted_post, then `muw + randn(S, D).dot(LSigw.T)`):
//
//   linear regression (model_linreg.py:25-34), rows [x, y]:  A = Sig0inv + X^T diag(w) X / sigsq,  rhs = Sig0inv.th0 + X^T (w*y) / sigsq
//   Gaussian location (gaussian.py:28-32), rows x:           A = Sig0inv + (sum w) Siginv,         rhs = Sig0inv.mu0 + Siginv . sum_i w_i x_i
//
// L . L^T (= C^-1 C^-T) is the REFERENCE's expression, kept on purpose; the true covariance is C^-T C^-1.
// The result is the reference's to rounding, not LAPACK's or BLAS's bits: the forward error is that of a Cholesky solve,
// O(D eps kappa(A)).
//
// C and L are kept as packed lower triangles in the work space (LDS on the device): 2 . D (D + 1) / 2 doubles, 129 KiB at
// D = 128, next to three D-vectors -- within the 160 KiB one work-group of gfx950 may take.
//
// Written the way bc_nnls_dev.h is: every loop is "element i = tid, tid + nt, ...", barriers between phases, every sum a
// fixed-order fma chain of one thread, so a run is bit-reproducible and the same text compiles for the host with tid = 0,
// nt = 1 and an empty barrier (tests/vi_sampler_harness.cpp checks it against the oracle without a GPU).
#pragma once
#include <math.h>

#define BC_VIS_MAXD 128                                   // largest D the work space is sized for
#define BC_VIS_LINREG 0                                   // sampler kinds (include/beta_cores_viopt.h)
#define BC_VIS_GAUSS 1
#define BC_VIS_TRI(d) ((d) * ((d) + 1) / 2)
#define BC_VIS_WS_DOUBLES(d) (2 * BC_VIS_TRI(d) + 3 * (d) + 2)

#ifndef BC_VIS_FN
#define BC_VIS_FN __device__
#define BC_VIS_TID ((int)threadIdx.x)
#define BC_VIS_NT ((int)blockDim.x)
// (the Gaussian kind re-reads, after a barrier, values other threads of the block wrote to device memory)
#define BC_VIS_SYNC() do { __threadfence_block(); __syncthreads(); } while (0)
#endif

struct VisArgs {
  int kind;                // BC_VIS_LINREG / BC_VIS_GAUSS
  int d, m, dz, s, dk;     // dimension, coreset rows, their width, samples, row pitch of the zero-padded Theta K1 reads
  const double* core;      // [m][dz] the coreset rows
  const double* w;         // [m]
  const double* sig0inv;   // [d][d]
  const double* b0;        // [d]  Sig0inv . th0 (constant over the loop: evaluated once by the host)
  const double* siginv;    // [d][d] (Gaussian kind)
  double sigsq;            // (linear regression)
  const double* E;         // [s][d] this step's normals
  double* theta;           // out: [.][dk], rows q < s, columns a < d (the padding is never touched)
  double* saux;            // out, Gaussian kind: [s] theta^T Siginv theta
  double* raw;             // scratch in device memory, Gaussian kind: [s][d] the samples before Siginv is applied
};

BC_VIS_FN inline int bc_vis_tri(int i, int k) { return i * (i + 1) / 2 + k; }

// b0 = Sig0inv . th0 for VisArgs::b0, on the HOST (bc_vi_optimize_begin, once per run): the full matrix row by row -- both
// triangles, where the factorisation reads the lower one only -- each entry one fixed-order fma chain.
inline void bc_vi_prior_rhs(const double* sig0inv, const double* th0, int d, double* b0) {
  for (int i = 0; i < d; ++i) {
    double acc = 0.;
    for (int j = 0; j < d; ++j) acc = fma(sig0inv[(size_t)i * d + j], th0[j], acc);
    b0[i] = acc;
  }
}

// Returns 1 (block-uniform) when a pivot of the factorisation is not finite and positive; nothing has been written to
// theta / saux then.  ws: BC_VIS_WS_DOUBLES(d) doubles.
BC_VIS_FN inline int bc_vi_sampler(const VisArgs& a, double* ws) {
  const int tid = BC_VIS_TID, nt = BC_VIS_NT;
  const int d = a.d, m = a.m, dz = a.dz, ntri = BC_VIS_TRI(d);
  double* Cf = ws;                  // A, then its factor C, packed: (i, k) at i (i + 1) / 2 + k
  double* Li = Cf + ntri;           // L = C^-1, packed
  double* rhs = Li + ntri;
  double* t = rhs + d;
  double* mu = t + d;
  double* sc = mu + d;              // [2] block-wide scalars
  // ---- A (lower triangle) and the right-hand side
  if (a.kind == BC_VIS_GAUSS) {
    if (tid == 0) {
      double ws_ = 0.;
      for (int r = 0; r < m; ++r) ws_ += a.w[r];
      sc[0] = ws_;
    }
    for (int j = tid; j < d; j += nt) {
      double acc = 0.;
      for (int r = 0; r < m; ++r) acc = fma(a.w[r], a.core[(size_t)r * dz + j], acc);
      t[j] = acc;                   // sum_i w_i x_i
    }
    BC_VIS_SYNC();
  }
  for (int e = tid; e < ntri; e += nt) {
    int i = (int)((sqrt(8. * (double)e + 1.) - 1.) * .5);
    while (bc_vis_tri(i + 1, 0) <= e) ++i;
    while (bc_vis_tri(i, 0) > e) --i;
    const int j = e - bc_vis_tri(i, 0);
    if (a.kind == BC_VIS_GAUSS) {
      Cf[e] = a.sig0inv[i * d + j] + sc[0] * a.siginv[i * d + j];
    } else {
      double acc = 0.;
      for (int r = 0; r < m; ++r) {
        const double* x = a.core + (size_t)r * dz;
        acc = fma(a.w[r] * x[i], x[j], acc);
      }
      Cf[e] = a.sig0inv[i * d + j] + acc / a.sigsq;
    }
  }
  for (int j = tid; j < d; j += nt) {
    double acc = 0.;
    if (a.kind == BC_VIS_GAUSS) {
      for (int b = 0; b < d; ++b) acc = fma(a.siginv[j * d + b], t[b], acc);
      rhs[j] = a.b0[j] + acc;
    } else {
      for (int r = 0; r < m; ++r) {
        const double* x = a.core + (size_t)r * dz;
        acc = fma(a.w[r] * x[d], x[j], acc);
      }
      rhs[j] = a.b0[j] + acc / a.sigsq;
    }
  }
  BC_VIS_SYNC();
  // ---- C = chol(A) in place, left-looking: thread i finishes element (i, k) from the finished columns < k
  for (int k = 0; k < d; ++k) {
    for (int i = k + tid; i < d; i += nt) {
      double sum = Cf[bc_vis_tri(i, k)];
      const double* ri = Cf + bc_vis_tri(i, 0);
      const double* rk = Cf + bc_vis_tri(k, 0);
      for (int q = 0; q < k; ++q) sum = fma(-ri[q], rk[q], sum);
      t[i] = sum;
    }
    BC_VIS_SYNC();
    const double piv = t[k];
    if (!(piv > 0. && piv < INFINITY)) return 1;      // (NaN fails the first comparison)
    const double dd = sqrt(piv);
    for (int i = k + tid; i < d; i += nt) Cf[bc_vis_tri(i, k)] = (i == k) ? dd : t[i] / dd;
    BC_VIS_SYNC();
  }
  // ---- L = C^-1 by forward substitution on the identity: column j is one thread's, top to bottom (it reads what it wrote)
  for (int j = tid; j < d; j += nt) {
    Li[bc_vis_tri(j, j)] = 1. / Cf[bc_vis_tri(j, j)];
    for (int i = j + 1; i < d; ++i) {
      double sum = 0.;
      const double* ci = Cf + bc_vis_tri(i, 0);
      for (int k = j; k < i; ++k) sum = fma(ci[k], Li[bc_vis_tri(k, j)], sum);
      Li[bc_vis_tri(i, j)] = -sum / ci[i];
    }
  }
  BC_VIS_SYNC();
  // ---- mu = L . (L^T . rhs)
  for (int k = tid; k < d; k += nt) {
    double acc = 0.;
    for (int i = k; i < d; ++i) acc = fma(Li[bc_vis_tri(i, k)], rhs[i], acc);
    t[k] = acc;
  }
  BC_VIS_SYNC();
  for (int i = tid; i < d; i += nt) {
    double acc = 0.;
    const double* li = Li + bc_vis_tri(i, 0);
    for (int k = 0; k <= i; ++k) acc = fma(li[k], t[k], acc);
    mu[i] = acc;
  }
  BC_VIS_SYNC();
  // ---- Theta = mu + E . L^T
  const int total = a.s * d;
  for (int e = tid; e < total; e += nt) {
    const int q = e / d, c = e - q * d;
    const double* eq = a.E + (size_t)q * d;
    const double* lc = Li + bc_vis_tri(c, 0);
    double acc = 0.;
    for (int k = 0; k <= c; ++k) acc = fma(eq[k], lc[k], acc);
    const double th = mu[c] + acc;
    if (a.kind == BC_VIS_GAUSS) a.raw[e] = th;
    else a.theta[(size_t)q * a.dk + c] = th;
  }
  if (a.kind != BC_VIS_GAUSS) return 0;
  BC_VIS_SYNC();
  // Gaussian location: K1 contracts the rows against Theta' = (Siginv . Theta^T)^T and takes theta^T Siginv theta per sample
  // (gaussian.py:11-12; the expressions of the host staging in bc_project.hip, one rounding per operation)
  for (int e = tid; e < total; e += nt) {
    const int q = e / d, c = e - q * d;
    const double* th = a.raw + (size_t)q * d;
    double m1 = 0.;
    for (int b = 0; b < d; ++b) m1 += a.siginv[(size_t)c * d + b] * th[b];
    a.theta[(size_t)q * a.dk + c] = m1;
  }
  for (int q = tid; q < a.s; q += nt) {
    const double* th = a.raw + (size_t)q * d;
    double tst = 0.;
    for (int c = 0; c < d; ++c) {
      double m2 = 0.;
      for (int b = 0; b < d; ++b) m2 += th[b] * a.siginv[(size_t)b * d + c];
      tst += th[c] * m2;
    }
    a.saux[q] = tst;
  }
  return 0;
}

// One coordinate of util/opt.py's _adam_loop / nn_opt, operation for operation (compile with -ffp-contract=off):
//   mom1 = b1 mom1 + (1 - b1) g;  mom2 = b2 mom2 + (1 - b2) g^2;  x = max(x - a mom1 / c1 / (eps + sqrt(mom2 / c2)), 0)
// omb1 = 1 - b1 and omb2 = 1 - b2 as the host rounds them.  np.maximum propagates NaN, and so does this.
BC_VIS_FN inline void bc_vi_adam_elem(double g, double* x, double* mom1, double* mom2, double b1, double omb1, double b2,
                                      double omb2, double eps, double step, double c1, double c2) {
  const double m1 = b1 * *mom1 + omb1 * g;
  const double m2 = b2 * *mom2 + omb2 * (g * g);
  const double upd = step * m1 / c1 / (eps + sqrt(m2 / c2));
  const double v = *x - upd;
  *mom1 = m1;
  *mom2 = m2;
  *x = (v != v) ? v : (v > 0. ? v : 0.);
}
