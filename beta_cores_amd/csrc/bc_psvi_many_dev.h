// The stages of one step of the batched BatchPSVI run (include/beta_cores_psvi_many.h) behind the Laplace fit and draw, for one
// thread block each.  Per problem p with points x_i (m rows of width D), weights w and this step's draws Theta (S x D):
//
//   bc_pm_ll_tile   L[r][q] = ll(z_r, th_q) - mean_q ll(z_r, .)  for the 16 rows of one tile and all S samples, in LDS:
//                   ll = -log1p(exp(m)) for m = -z . th < 100, else -m (model_lr.py:72-79); the contraction Z . Theta^T runs on
//                   v_mfma_f64_16x16x4_f64, one 16 x 16 tile of (rows, samples) per wave in turn; the row mean is projector.py:48.
//                   The caller either adds the tile's rows up per sample (a tile of the gathered data rows: one row of the
//                   target's partial sums) or stores them (a tile of the problem's own points: its corevecs).
//   bc_pm_gauss_tile  the same tile for the Gaussian location model (gaussian.py:7-15): ll = c0 - 1/2 ((ra_r + sa_q) - 2 p),
//                   p = x_r . Theta'_q on the same MFMA, Theta' = (Siginv Theta^T)^T, sa_q = th_q^T Siginv th_q (both from
//                   bc_vi_sampler) and ra_r = x_r^T Siginv x_r from bc_pm_rowaux_tile.  K1's expression for this model
//                   (bc_model_value<BC_MODEL_GAUSS_LL>), the terms the centring removes kept: the values round like K1's.
//   bc_pm_rowaux_tile ra of the 16 rows of one tile: k_row_quadform's expression (bc_project.hip), (x * (x . Siginv)).sum()
//   bc_pm_resid     target = scale * (partials added in tile order);  resid = target - w . corevecs;  g_w = -corevecs . resid / S
//   (the point-gradient is bc_psvi_dev.h's bc_psvi_point_grad on resid, one block per point)
//   bc_pm_adam      one step of util/opt.py's partial_nn_opt on x = (w, points), operation for operation; max(., 0) on w only
//
// Written the way bc_vi_laplace_dev.h is: every loop has a fixed bound, every sum a fixed order; the same text compiles for the
// host with tid = 0, nt = 1 and empty barriers, and what the host cannot compile (MFMA, cross-lane moves) stands under __HIPCC__
// with a plain loop of the same mathematical result beside it (tests/psvi_many_harness.cpp).  On the device a block is
// BC_PM_BLOCK threads.
#pragma once
#include <math.h>
#include <stddef.h>
#include "bc_vi_laplace_dev.h"      // the stages of the fit (a host build defines its BC_VIL_* macros before it includes that file)

#define BC_PM_BLOCK 256
#define BC_PM_TILE 16                                      // rows of a tile: one MFMA tile high
#define BC_PM_TILE_DOUBLES(s) ((size_t)BC_PM_TILE * (size_t)(s))      // bc_pm_ll_tile's LDS

#ifndef BC_PM_FN
#define BC_PM_FN __device__
#define BC_PM_TID ((int)threadIdx.x)
#define BC_PM_NT ((int)blockDim.x)
// (values other threads of the block wrote to device memory are re-read after a barrier)
#define BC_PM_SYNC() do { __threadfence_block(); __syncthreads(); } while (0)
#define BC_PM_ANY(x) __syncthreads_or(x)                   // block-uniform: some thread's x is not 0 (a barrier)
#endif

#ifdef __HIPCC__
typedef double bc_pm_d4 __attribute__((ext_vector_type(4)));
#endif

// The Laplace fit of one size: bc_vi_laplace_dev.h's mode search, ONE full Newton step behind it, then H at that point and its
// factor (W.A <- C, W.Li <- C^-1; the caller draws).  Why the extra step: the search restates the host's stopping rule, and like
// the host's it can end where its last line search backtracks in the rounding noise of f -- up to 1e-9 from the mode, 7e-12
// seen on two points of weight 300 (profiles/psvi_many_notes.md).  Inside a weight optimisation that noise is the largest error
// of a step by orders; this close to the mode Newton's full step squares it away for one more Gram product and factorisation.
// The search itself is left as it is: k_vi_laplace and k_laplace_many keep their bits.  Returns 1 (block-uniform) when the
// problem must be marked; nothing but the work space and rowc has been written.
BC_PM_FN inline int bc_pm_fit(const VilArgs& a, const VilWs& W, VilFit* fit) {
  const int tid = BC_VIL_TID, nt = BC_VIL_NT, d = a.d;
  if (bc_vil_mode(a, W, fit)) return 1;
  bc_vil_hessian(a, W);                                    // [H; g] at the search's end point (rowc holds its m_n)
  if (bc_vil_chol(W.A, W.rdiag, d, d + 1, tid, nt)) return 1;
  bc_vil_backsolve(W.A, W.rdiag, d, W.stp, tid);
  BC_VIL_SYNC();
  for (int j = tid; j < d; j += nt) W.mu[j] += W.stp[j];
  BC_VIL_SYNC();
  int grp = 1;                                             // lanes per row of the value pass, as bc_vil_mode chooses them
  while (grp < 16 && 2 * grp <= nt && (long)a.m * (2 * grp) <= nt && 2 * grp <= d) grp *= 2;
  const double f = bc_vil_value(a, W.mu, W.red, grp, tid, nt);      // (leaves the m_n of the new point in rowc)
  if (!(f - f == 0.)) return 1;
  fit->f = f;
  bc_vil_hessian(a, W);
  return bc_vil_factor(a, W);
}

BC_PM_FN inline double bc_pm_ll(double mm) { return mm < 100. ? -log1p(exp(mm)) : -mm; }

BC_PM_FN inline double bc_pm_row_elem(const void* rows, int elem, size_t at) {
  return elem == 4 ? (double)static_cast<const float*>(rows)[at] : static_cast<const double*>(rows)[at];
}

struct PmTileArgs {
  const void* rows;        // [n][d] row-major; elem == 4: floats, widened as they are read
  int elem;
  int n, d, s;
  const double* theta;     // [s][d]   (Gaussian kind: Theta')
  const double* ra;        // Gaussian kind: [n] x^T Siginv x of the rows
  const double* sa;        // Gaussian kind: [s] theta^T Siginv theta
  double c0;               // Gaussian kind: -d/2 log(2 pi) - 1/2 logdet Sigma
};

#define BC_PM_LOGISTIC 0                                   // the kinds of a run: what the tile evaluates
#define BC_PM_GAUSS 1
#define BC_PM_ROWAUX_DOUBLES(d) (2 * (size_t)BC_PM_TILE * (size_t)(d))      // bc_pm_rowaux_tile's LDS

// One element of the tile from the contraction p = row . theta_q.  Logistic: z = row, m = -p.  Gaussian: K1's expression.
template <int KIND>
BC_PM_FN inline double bc_pm_value(const PmTileArgs& a, double p, int row, int q) {
  if (KIND == BC_PM_LOGISTIC) return bc_pm_ll(-p);
  const double qf = (a.ra[row] + a.sa[q]) - 2. * p;
  return a.c0 - 1. / 2. * qf;
}

// t[r * s + q], r < 16, q < s: the row-centred log-likelihoods of rows tile * 16 + r (rows >= n: zeros); ends with a barrier.
// KIND: BC_PM_LOGISTIC (bc_pm_ll_tile) or BC_PM_GAUSS (bc_pm_gauss_tile); nothing but the element's value differs.
template <int KIND>
BC_PM_FN inline void bc_pm_tile(const PmTileArgs& a, int tile, double* t) {
  const int tid = BC_PM_TID, nt = BC_PM_NT;
  const int d = a.d, s = a.s, n = a.n, row0 = tile * BC_PM_TILE;
#ifdef __HIPCC__
  const int lane = tid & 63, wv = tid >> 6, nw = nt >> 6, r = lane & 15, kq = lane >> 4;
  const int qt = (s + 15) >> 4, ia = row0 + r;
  for (int Q = wv; Q < qt; Q += nw) {                      // (wave-uniform: every lane issues the MFMAs)
    const int qb = Q * 16 + r;
    bc_pm_d4 acc = {0., 0., 0., 0.};
    for (int k0 = 0; k0 < d; k0 += 4) {                    // operand maps: A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15]
      const int k = k0 + kq;
      const double av = (ia < n && k < d) ? bc_pm_row_elem(a.rows, a.elem, (size_t)ia * d + k) : 0.;
      const double bv = (qb < s && k < d) ? a.theta[(size_t)qb * d + k] : 0.;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
    }
    for (int q4 = 0; q4 < 4; ++q4) {                       // result map: col = lane & 15, row = (lane >> 4) + 4 q4
      const int i = kq + 4 * q4;
      if (qb < s) t[i * s + qb] = (row0 + i < n) ? bc_pm_value<KIND>(a, acc[q4], row0 + i, qb) : 0.;
    }
  }
  BC_PM_SYNC();
  // the row means: 16 lanes per row, lane g adds q = g, g + 16, ... in order, a butterfly adds the 16 partial sums
  for (int r2 = tid >> 4; r2 < BC_PM_TILE; r2 += nt >> 4) {
    const int g = tid & 15;
    double part = 0.;
    for (int q = g; q < s; q += 16) part += t[r2 * s + q];
    for (int o = 8; o > 0; o >>= 1) part += __shfl_xor(part, o);
    const double mean = part / (double)s;
    for (int q = g; q < s; q += 16) t[r2 * s + q] -= mean;
  }
#else
  for (int i = tid; i < BC_PM_TILE; i += nt) {
    double sum = 0.;
    for (int q = 0; q < s; ++q) {
      double acc = 0.;
      if (row0 + i < n)
        for (int k = 0; k < d; ++k) acc = fma(bc_pm_row_elem(a.rows, a.elem, (size_t)(row0 + i) * d + k), a.theta[(size_t)q * d + k], acc);
      t[i * s + q] = (row0 + i < n) ? bc_pm_value<KIND>(a, acc, row0 + i, q) : 0.;
      sum += t[i * s + q];
    }
    const double mean = sum / (double)s;
    for (int q = 0; q < s; ++q) t[i * s + q] -= mean;
  }
#endif
  BC_PM_SYNC();
}

BC_PM_FN inline void bc_pm_ll_tile(const PmTileArgs& a, int tile, double* t) { bc_pm_tile<BC_PM_LOGISTIC>(a, tile, t); }
BC_PM_FN inline void bc_pm_gauss_tile(const PmTileArgs& a, int tile, double* t) { bc_pm_tile<BC_PM_GAUSS>(a, tile, t); }

// ra[tile * 16 + r] = x_r^T Siginv x_r for the rows of one tile (rows >= n: untouched), in k_row_quadform's expression
// (bc_project.hip; gaussian.py:10): t_a = the fma chain over b of x_b Siginv[b][a], then the products x_a t_a added in
// ascending a.  The d chains of a row are spread over the block; one thread adds a row's products up.
// ws: BC_PM_ROWAUX_DOUBLES(d) doubles; ends with a barrier.
BC_PM_FN inline void bc_pm_rowaux_tile(const void* rows, int elem, int n, int d, const double* siginv, int tile, double* ws, double* ra) {
  const int tid = BC_PM_TID, nt = BC_PM_NT, row0 = tile * BC_PM_TILE;
  const int here = n - row0 < BC_PM_TILE ? n - row0 : BC_PM_TILE;
  double* x = ws;                                          // [16][d] the rows, widened
  double* u = ws + (size_t)BC_PM_TILE * d;                 // [16][d] x_a t_a
  for (int e = tid; e < here * d; e += nt) x[e] = bc_pm_row_elem(rows, elem, (size_t)row0 * d + e);
  BC_PM_SYNC();
  for (int e = tid; e < here * d; e += nt) {
    const int r = e / d, aa = e - r * d;
    const double* xr = x + (size_t)r * d;
    double acc = 0.;
    for (int bb = 0; bb < d; ++bb) acc = fma(xr[bb], siginv[(size_t)bb * d + aa], acc);
    u[e] = xr[aa] * acc;
  }
  BC_PM_SYNC();
  for (int r = tid; r < here; r += nt) {
    double tot = 0.;
    for (int aa = 0; aa < d; ++aa) tot += u[(size_t)r * d + aa];
    ra[row0 + r] = tot;
  }
  BC_PM_SYNC();
}

// The three S x d x d products of the Gaussian kind's posterior stage on the fp64 matrix cores, from the factor that
// bc_vi_sampler (called with no samples) leaves in its work space:
//   Theta[q][c]  = mu[c] + sum_{k <= c} E[q][k] L[c][k]            (L = C^-1, packed lower triangle: (i, k) at i (i + 1) / 2 + k)
//   Theta'[q][c] = sum_b Siginv[c][b] Theta[q][b]
//   sa[q]        = sum_c Theta[q][c] (sum_b Theta[q][b] Siginv[b][c])
// the expressions of bc_vi_sampler's Gaussian tail with its per-thread chains replaced by v_mfma_f64_16x16x4_f64 tiles of
// (16 samples, 16 coordinates): a wave takes a strip of 16 samples and walks the coordinate tiles in ascending order.  sa: each
// lane adds the products of its own column tile by tile, a butterfly adds the 16 columns -- a fixed order that depends on d
// alone.  Theta is written to device memory and re-read after a barrier, as bc_vi_sampler does.  Not bc_vi_sampler's bits; the
// same bounds (tests/psvi_many_gauss_cases.py).  The block is a multiple of 64 threads.
#define BC_PM_VIS_TRI(d) ((d) * ((d) + 1) / 2)
#define BC_PM_VIS_LI(d) BC_PM_VIS_TRI(d)                       // bc_vi_sampler's work space: C | L | rhs | t | mu | sc[2]
#define BC_PM_VIS_MU(d) (2 * BC_PM_VIS_TRI(d) + 2 * (d))
#define BC_PM_VIS_DOUBLES(d) (2 * BC_PM_VIS_TRI(d) + 3 * (d) + 2)      // (the unit that includes both headers asserts == BC_VIS_WS_DOUBLES)

struct PmPostArgs {
  int d, s;
  const double* E;         // [s][d] this step's normals
  const double* Li;        // packed L (LDS)
  const double* mu;        // [d] (LDS)
  const double* siginv;    // [d][d]
  double* raw;             // out [s][d] Theta
  double* thp;             // out [s][d] Theta'
  double* sa;              // out [s]
};

BC_PM_FN inline void bc_pm_post_products(const PmPostArgs& a) {
  const int tid = BC_PM_TID, nt = BC_PM_NT, d = a.d, s = a.s;
#ifdef __HIPCC__
  const int lane = tid & 63, wv = tid >> 6, nw = nt >> 6, r = lane & 15, kq = lane >> 4;
  const int qt = (s + 15) >> 4, ct = (d + 15) >> 4;
  for (int Q = wv; Q < qt; Q += nw) {                      // (wave-uniform: every lane issues the MFMAs)
    const int qa = Q * 16 + r;
    for (int Ct = 0; Ct < ct; ++Ct) {
      const int cb = Ct * 16 + r, kend = Ct * 16 + 16 < d ? Ct * 16 + 16 : d;      // L[c][k] = 0 for k > c
      bc_pm_d4 acc = {0., 0., 0., 0.};
      for (int k0 = 0; k0 < kend; k0 += 4) {               // operand maps: A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15]
        const int k = k0 + kq;
        const double av = (qa < s && k < d) ? a.E[(size_t)qa * d + k] : 0.;
        const double bv = (cb < d && k <= cb) ? a.Li[cb * (cb + 1) / 2 + k] : 0.;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
      }
      for (int q4 = 0; q4 < 4; ++q4) {                     // result map: col = lane & 15, row = (lane >> 4) + 4 q4
        const int q = Q * 16 + kq + 4 * q4;
        if (q < s && cb < d) a.raw[(size_t)q * d + cb] = a.mu[cb] + acc[q4];
      }
    }
  }
  BC_PM_SYNC();
  for (int Q = wv; Q < qt; Q += nw) {
    const int qa = Q * 16 + r;
    double part[4] = {0., 0., 0., 0.};
    for (int Ct = 0; Ct < ct; ++Ct) {
      const int cb = Ct * 16 + r;
      bc_pm_d4 acc1 = {0., 0., 0., 0.}, acc2 = {0., 0., 0., 0.};
      for (int k0 = 0; k0 < d; k0 += 4) {
        const int k = k0 + kq;
        const bool in = cb < d && k < d;
        const double av = (qa < s && k < d) ? a.raw[(size_t)qa * d + k] : 0.;
        const double b1 = in ? a.siginv[(size_t)cb * d + k] : 0.;
        const double b2 = in ? a.siginv[(size_t)k * d + cb] : 0.;
        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, b1, acc1, 0, 0, 0);
        acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, b2, acc2, 0, 0, 0);
      }
      for (int q4 = 0; q4 < 4; ++q4) {
        const int q = Q * 16 + kq + 4 * q4;
        if (q < s && cb < d) {
          a.thp[(size_t)q * d + cb] = acc1[q4];
          part[q4] += a.raw[(size_t)q * d + cb] * acc2[q4];
        }
      }
    }
    for (int q4 = 0; q4 < 4; ++q4) {
      double v = part[q4];
      for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o);
      const int q = Q * 16 + kq + 4 * q4;
      if (r == 0 && q < s) a.sa[q] = v;
    }
  }
#else
  for (int e = tid; e < s * d; e += nt) {
    const int q = e / d, c = e - q * d;
    double acc = 0.;
    for (int k = 0; k <= c; ++k) acc = fma(a.E[(size_t)q * d + k], a.Li[c * (c + 1) / 2 + k], acc);
    a.raw[e] = a.mu[c] + acc;
  }
  BC_PM_SYNC();
  for (int q = tid; q < s; q += nt) {
    const double* th = a.raw + (size_t)q * d;
    double tst = 0.;
    for (int c = 0; c < d; ++c) {
      double m1 = 0., m2 = 0.;
      for (int b = 0; b < d; ++b) {
        m1 = fma(a.siginv[(size_t)c * d + b], th[b], m1);
        m2 = fma(th[b], a.siginv[(size_t)b * d + c], m2);
      }
      a.thp[(size_t)q * d + c] = m1;
      tst += th[c] * m2;
    }
    a.sa[q] = tst;
  }
#endif
}

// A tile of the gathered data rows: part[q] = sum over the tile's rows, top to bottom.
BC_PM_FN inline void bc_pm_tile_colsum(const PmTileArgs& a, int tile, const double* t, double* part) {
  const int rows = a.n - tile * BC_PM_TILE < BC_PM_TILE ? a.n - tile * BC_PM_TILE : BC_PM_TILE;
  for (int q = BC_PM_TID; q < a.s; q += BC_PM_NT) {
    double sum = 0.;
    for (int r = 0; r < rows; ++r) sum += t[r * a.s + q];
    part[q] = sum;
  }
}

// A tile of the problem's points: cv[(tile * 16 + r) * s + q] <- the tile's rows.
BC_PM_FN inline void bc_pm_tile_store(const PmTileArgs& a, int tile, const double* t, double* cv) {
  const int rows = a.n - tile * BC_PM_TILE < BC_PM_TILE ? a.n - tile * BC_PM_TILE : BC_PM_TILE;
  for (int e = BC_PM_TID; e < rows * a.s; e += BC_PM_NT) cv[(size_t)tile * BC_PM_TILE * a.s + e] = t[e];
}

struct PmResidArgs {
  int m, s, tiles;
  double scale;            // N / n_sub
  const double* part;      // [tiles][s]
  const double* cv;        // [m][s]
  const double* w;         // [m]
  double* target;          // out [s]
  double* resid;           // out [s]
  double* gw;              // out [m]
};

// Returns 1 (block-uniform) when a target, a residual or a component of g_w is not finite; everything has been written then,
// and the caller marks the problem.
BC_PM_FN inline int bc_pm_resid(const PmResidArgs& a) {
  const int tid = BC_PM_TID, nt = BC_PM_NT;
  int bad = 0;
  for (int q = tid; q < a.s; q += nt) {
    double sum = 0.;
    for (int b = 0; b < a.tiles; ++b) sum += a.part[(size_t)b * a.s + q];
    const double tg = a.scale * sum;
    double dot = 0.;
    for (int i = 0; i < a.m; ++i) dot = fma(a.w[i], a.cv[(size_t)i * a.s + q], dot);
    const double r = tg - dot;
    a.target[q] = tg;
    a.resid[q] = r;
    if (!(tg - tg == 0.) || !(r - r == 0.)) bad = 1;
  }
  BC_PM_SYNC();
  for (int i = tid; i < a.m; i += nt) {
    double dot = 0.;
    for (int q = 0; q < a.s; ++q) dot = fma(a.cv[(size_t)i * a.s + q], a.resid[q], dot);
    const double g = -dot / (double)a.s;
    a.gw[i] = g;
    if (!(g - g == 0.)) bad = 1;
  }
  return BC_PM_ANY(bad) ? 1 : 0;
}

// One coordinate of util/opt.py's _adam_loop, operation for operation (compile with -ffp-contract=off):
//   mom1 = b1 mom1 + (1 - b1) g;  mom2 = b2 mom2 + (1 - b2) g^2;  x = x - a mom1 / c1 / (eps + sqrt(mom2 / c2))
// and, for a coordinate of nn_idcs, x = max(x, 0) (np.maximum propagates NaN, and so does this).
BC_PM_FN inline void bc_pm_adam_elem(double g, double* x, double* mom1, double* mom2, double step, double c1, double c2, int project) {
  const double b1 = 0.9, b2 = 0.999, eps = 1e-8;
  const double m1 = b1 * *mom1 + (1. - b1) * g;
  const double m2 = b2 * *mom2 + (1. - b2) * (g * g);
  const double upd = step * m1 / c1 / (eps + sqrt(m2 / c2));
  const double v = *x - upd;
  *mom1 = m1;
  *mom2 = m2;
  *x = (project && v == v) ? (v > 0. ? v : 0.) : v;
}

struct PmAdamArgs {
  int m, d;
  const double *gw, *gp;   // [m], [m][d]
  double *w, *pts;         // [m], [m][d]
  double *m1w, *m1p, *m2w, *m2p;
  double step, c1, c2;     // step_sched(m)(i), 1 - b1^(i+1), 1 - b2^(i+1)
};

// Returns 1 (block-uniform) when a component of the gradient is not finite (nothing has been written) or a coordinate is not
// finite after the step.
BC_PM_FN inline int bc_pm_adam(const PmAdamArgs& a) {
  const int tid = BC_PM_TID, nt = BC_PM_NT;
  const int nw = a.m, np = a.m * a.d;
  int bad = 0;
  for (int e = tid; e < nw + np; e += nt) {
    const double g = e < nw ? a.gw[e] : a.gp[e - nw];
    if (!(g - g == 0.)) bad = 1;
  }
  if (BC_PM_ANY(bad)) return 1;
  for (int e = tid; e < nw + np; e += nt) {
    if (e < nw) {
      bc_pm_adam_elem(a.gw[e], a.w + e, a.m1w + e, a.m2w + e, a.step, a.c1, a.c2, 1);
      if (!(a.w[e] - a.w[e] == 0.)) bad = 1;
    } else {
      const int j = e - nw;
      bc_pm_adam_elem(a.gp[j], a.pts + j, a.m1p + j, a.m2p + j, a.step, a.c1, a.c2, 0);
      if (!(a.pts[j] - a.pts[j] == 0.)) bad = 1;
    }
  }
  return BC_PM_ANY(bad) ? 1 : 0;
}
