// The logistic Laplace sampler of the greedy-VI weight optimisation, for one thread block (k_vi_laplace in bc_viopt.hip); the
// same four stages, one block per problem, are the batched fit of many small posteriors (k_laplace_many in bc_laplace_small.hip).
//
//   mu = argmax_th  f(th) = -sum_n w_n softplus(-z_n . th) - D/2 log(2 pi) - th . th / 2          (rows z = y * x, prior N(0, I))
//   Theta = mu + E . C^-T            with  C = chol(H(mu)),  H(th) = I + Z^T diag(w p (1 - p)) Z,  p_n = sigmoid(-z_n . th)
//   diag:  Theta[q][j] = mu[j] + E[q][j] / sqrt(H(mu)[j][j])
//
// restates samplers._lr_mode_newton followed by the solver == 'newton' branch of samplers.logistic_laplace (model_lr.py:72-137,
// zellner_logreg/main.py:86-111, 139-144): damped Newton steps with the host's backtracking constants and stopping rule, from
// the start point in `mode` (the previous step's mode: the ADAM step moved the weights a little, 2-3 iterations instead of 10-20).
//
// How the time is spent differently from bc_vi_sampler (profiles/vi_laplace_notes.md):
//   * H and the gradient are ONE Gram product of the rows widened by a column: the lower triangle of
//     [Z | 1]^T diag(.) [Z | 1] in 16 x 16 tiles on v_mfma_f64_16x16x4_f64, a tile (or, for few tiles, a slice of the rows of a
//     tile) per wave; row D of the result is the gradient.
//   * the Cholesky is right-looking, one barrier per column: every thread takes part in each trailing update.  The gradient
//     rides along as row D of the packed triangle, so the forward solve y = C^-1 g and the decrement g . H^-1 g = y . y
//     (minus the trailing corner) fall out of the factorisation.
//   * the Newton step is one back substitution C^T step = y by one wave with the running right-hand side in registers; the
//     inverse C^-1 is formed once per launch, for the draw, and E . C^-T runs on the matrix cores.
//
// Every loop has a fixed upper count, every sum a fixed order (a repeated run gives the same bits), a comparison with NaN
// ends a loop.  A weight, f, the decrement (hence any component of the gradient) or a pivot that is not finite -- a pivot
// must also be positive -- returns 1 before anything has been written to theta, mode or counts.  A weight that is not
// positive contributes exactly nothing (the reference's Z[wts > 0]).
//
// Written the way bc_vi_sampler_dev.h is: the same text compiles for the host with tid = 0, nt = 1 and an empty barrier; what
// the host cannot compile (MFMA, cross-lane moves) is under __HIPCC__ with a plain loop of the same mathematical result beside
// it (tests/vi_laplace_harness.cpp, tests/laplace_many_harness.cpp).  On the device the block is BC_VIL_BLOCK threads.
#pragma once
#include <math.h>

#define BC_VIL_MAXD 128
#define BC_VIL_BLOCK 512
#define BC_VIL_MAX_ITER 200                               // Newton iterations (the host's max_iter)
#define BC_VIL_MAX_HALVINGS 34                            // 2^-34 < 1e-10 <= 2^-33: the host's `t < 1e-10` ends the search there
#define BC_VIL_TRI(d) ((d) * ((d) + 1) / 2)
// partial tiles of the Gram product when there are fewer tiles than waves (D < 32: at most 3 tiles, 8 slices of 256)
#define BC_VIL_PART_DOUBLES(d) ((d) < 32 ? 2048 : 0)
// [H | g] packed, (D + 1) rows; C^-1 packed; mu, step, cand, 1 / diag C; 16 block-wide scalars; the partial tiles: 134 KiB at
// D = 128
#define BC_VIL_WS_DOUBLES(d) (BC_VIL_TRI((d) + 1) + BC_VIL_TRI(d) + 4 * (d) + 16 + BC_VIL_PART_DOUBLES(d))
#define BC_VIL_ROW_DOUBLES(m) (3 * (size_t)(m))           // VilArgs::rowc

#ifndef BC_VIL_FN
#define BC_VIL_FN __device__
#define BC_VIL_TID ((int)threadIdx.x)
#define BC_VIL_NT ((int)blockDim.x)
// (values other threads of the block wrote to device memory -- rowc -- are re-read after a barrier)
#define BC_VIL_SYNC() do { __threadfence_block(); __syncthreads(); } while (0)
#endif

struct VilArgs {
  int d, m, dz, s, dk;     // dimension, coreset rows, their width (== d), samples, row pitch of the zero-padded Theta K1 reads
  int diag;                // != 0: the diagonal form of the covariance
  const double* core;      // [m][dz] the coreset rows z = y * x
  const double* w;         // [m]
  const double* E;         // [s][d] this step's normals
  double* theta;           // out: [.][dk], rows q < s, columns a < d (the padding is never touched)
  double* mode;            // [d + 1] in: the start point.  out: the mode, then the decrement of the last Newton system solved
  double* rowc;            // scratch in device memory, BC_VIL_ROW_DOUBLES(m): w p | w p (1 - p) | m_n = -z_n . th
  int* counts;             // out [4]: Newton steps of this launch | halvings of its last line search | [2] += the steps |
                           // halvings of all its line searches
};

#ifdef __HIPCC__
typedef double bc_vil_d4 __attribute__((ext_vector_type(4)));
#endif

BC_VIL_FN inline int bc_vil_tri(int i, int k) { return i * (i + 1) / 2 + k; }

// The sum of one value per thread, the same bits in every thread: lanes by a butterfly, waves in order.
BC_VIL_FN inline double bc_vil_block_sum(double v, double* red, int tid, int nt) {
#ifdef __HIPCC__
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((tid & 63) == 0) red[tid >> 6] = v;
  BC_VIL_SYNC();
  double r = 0.;
  for (int k = 0; k < (nt >> 6); ++k) r += red[k];
  BC_VIL_SYNC();      // (red is written again by the next sum)
  return r;
#else
  (void)red; (void)tid; (void)nt;
  return v;
#endif
}

// f(th), block-uniform; leaves m_n = -z_n . th in rowc[2m + n].  `grp` lanes share a row (a power of two that divides the
// wave, fixed for the run): each takes every grp-th column, a butterfly adds them.  A weight that is not finite gives NaN.
BC_VIL_FN inline double bc_vil_value(const VilArgs& a, const double* th, double* red, int grp, int tid, int nt) {
  const int d = a.d, m = a.m, rows_per = nt / grp, g = tid % grp;
  double part = 0.;
  for (int base = 0; base < m; base += rows_per) {      // (the same trip count in every thread: the butterfly needs them all)
    const int n = base + tid / grp;
    double acc = 0.;
    if (n < m) {
      const double* z = a.core + (size_t)n * a.dz;
      for (int j = g; j < d; j += grp) acc = fma(z[j], th[j], acc);
    }
#ifdef __HIPCC__
    for (int o = grp >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
#endif
    if (n < m && g == 0) {
      const double wn = a.w[n], mm = -acc;
      a.rowc[2 * (size_t)m + n] = mm;
      if (wn - wn != 0.) part = NAN;                    // NaN or an infinity
      else if (wn > 0.) part += wn * (fmax(mm, 0.) + log1p(exp(-fabs(mm))));
    }
  }
  double q = 0.;
  for (int j = 0; j < d; ++j) q = fma(th[j], th[j], q);
  const double sum = bc_vil_block_sum(part, red, tid, nt);      // (its barriers: th may be rewritten once this returns)
  return -sum - 0.5 * d * 1.8378770664093453 - 0.5 * q;      // log(2 pi)
}

// rowc[n] = w p, rowc[m + n] = w p (1 - p) from the m_n the last bc_vil_value left; 0 for a weight that is not positive.
BC_VIL_FN inline void bc_vil_row_coefs(const VilArgs& a, int tid, int nt) {
  const int m = a.m;
  for (int n = tid; n < m; n += nt) {
    const double wn = a.w[n];
    double wp = 0., c = 0.;
    if (wn > 0.) {
      const double p = 0.5 * (1. + tanh(0.5 * a.rowc[2 * (size_t)m + n]));      // e^m / (1 + e^m), overflow-free
      wp = wn * p;
      c = wp * (1. - p);
    }
    a.rowc[n] = wp;
    a.rowc[(size_t)m + n] = c;
  }
}

// One element of the widened Gram product into the packed triangle A: rows i < d are H = I + sum, row d is g = -mu + sum.
BC_VIL_FN inline void bc_vil_put(double* A, const double* mu, int d, int i, int j, double sum) {
  if (i > d || j > i || j >= d) return;
  A[bc_vil_tri(i, j)] = (i == d) ? -mu[j] + sum : (i == j ? 1. + sum : sum);
}

// A (packed, d + 1 rows) <- [H(mu); g(mu)^T] with the row coefficients of bc_vil_row_coefs; corner (d, d) = 0.
BC_VIL_FN inline void bc_vil_gram(const VilArgs& a, double* A, const double* mu, double* part, int tid, int nt) {
  const int d = a.d, m = a.m, dz = a.dz;
  if (tid == 0) A[bc_vil_tri(d, d)] = 0.;
#ifdef __HIPCC__
  const int lane = tid & 63, wv = tid >> 6, nw = nt >> 6, r = lane & 15, kq = lane >> 4;
  const int ntile = (d + 1 + 15) >> 4, T = ntile * (ntile + 1) / 2;
  const int P = (BC_VIL_PART_DOUBLES(d) > 0 && T < nw) ? nw / T : 1;      // slices of the rows per tile
  const int nch = (m + 3) >> 2, per = (nch + P - 1) / P;                  // k-steps of 4 rows
  for (int it = wv; it < T * P; it += nw) {                               // (wave-uniform: every lane issues the MFMAs)
    const int t = it / P, p = it - t * P;
    int I = 0;
    while ((I + 1) * (I + 2) / 2 <= t) ++I;
    const int J = t - I * (I + 1) / 2, ia = I * 16 + r, jb = J * 16 + r;
    const int c1 = (p + 1) * per < nch ? (p + 1) * per : nch;
    bc_vil_d4 acc = {0., 0., 0., 0.};
    for (int c = p * per; c < c1; ++c) {
      const int n = c * 4 + kq;      // operand maps: A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15]
      double av = 0., bv = 0.;
      if (n < m && a.w[n] > 0.) {
        const double* z = a.core + (size_t)n * dz;
        if (ia < d) av = a.rowc[(size_t)m + n] * z[ia];
        else if (ia == d) av = a.rowc[n];
        if (jb < d) bv = z[jb];
      }
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
    }
    for (int q = 0; q < 4; ++q) {    // result map of the f64 form: col = lane & 15, row = (lane >> 4) + 4 q
      if (P == 1) bc_vil_put(A, mu, d, I * 16 + kq + 4 * q, J * 16 + r, acc[q]);
      else part[(p * T + t) * 256 + (kq + 4 * q) * 16 + r] = acc[q];
    }
  }
  if (P > 1) {
    BC_VIL_SYNC();
    for (int e = tid; e < T * 256; e += nt) {
      const int t = e >> 8;
      int I = 0;
      while ((I + 1) * (I + 2) / 2 <= t) ++I;
      const int J = t - I * (I + 1) / 2;
      double sum = 0.;
      for (int p = 0; p < P; ++p) sum += part[(p * T + t) * 256 + (e & 255)];
      bc_vil_put(A, mu, d, I * 16 + ((e >> 4) & 15), J * 16 + (e & 15), sum);
    }
  }
#else
  (void)part;
  for (int i = tid; i <= d; i += nt)
    for (int j = 0; j <= i && j < d; ++j) {
      double acc = 0.;
      for (int n = 0; n < m; ++n) {
        if (!(a.w[n] > 0.)) continue;
        const double* z = a.core + (size_t)n * dz;
        acc = fma(i < d ? a.rowc[(size_t)m + n] * z[i] : a.rowc[n], z[j], acc);
      }
      bc_vil_put(A, mu, d, i, j, acc);
    }
#endif
}

// Right-looking Cholesky of the leading d x d block of the packed triangle A, in place; rows d .. rows - 1 ride along (their
// columns < d become row . C^-T, their own trailing block is updated like any other).  Returns 1 (block-uniform) on a pivot
// that is not finite and positive.  ONE barrier per column: every thread takes the pivot's root and its reciprocal r itself and
// updates the trailing triangle from the column as it stands, scaling on the fly (a_ij -= (a_ik r) (a_jk r)); the column is
// stored scaled -- the same products -- one phase later, when nobody reads it unscaled any more.  16 lanes along a row, the row
// groups down the rows; a thread first loads the operands of up to BC_VIL_CHOL_NJ elements, then updates them, so that the LDS
// latencies overlap instead of adding up.  rdiag[k] = 1 / C[k][k] is kept for the solves.
#define BC_VIL_CHOL_NJ 9
#ifdef __HIPCC__
#define BC_VIL_UNROLL _Pragma("unroll")
#else
#define BC_VIL_UNROLL
#endif
BC_VIL_FN inline int bc_vil_chol(double* A, double* rdiag, int d, int rows, int tid, int nt) {
  const int nc = nt >= 16 ? 16 : 1, nr = nt / nc, tr = tid / nc, tc = tid - tr * nc;
  double dd_prev = 0., rinv_prev = 0.;
  for (int k = 0; k <= d; ++k) {
    double rinv = 0., dd = 0.;
    if (k < d) {
      const double piv = A[bc_vil_tri(k, k)];
      if (!(piv > 0. && piv < INFINITY)) return 1;      // (NaN fails the first comparison)
      dd = sqrt(piv);
      rinv = 1. / dd;
    }
    if (k > 0) {                                        // column k - 1, final: nothing of this phase reads or writes it
      for (int i = k + tid; i < rows; i += nt) A[bc_vil_tri(i, k - 1)] *= rinv_prev;
      if (tid == 0) { A[bc_vil_tri(k - 1, k - 1)] = dd_prev; rdiag[k - 1] = rinv_prev; }
    }
    if (k < d)
      for (int i = k + 1 + tr; i < rows; i += nr) {
        double* ri = A + bc_vil_tri(i, 0);
        const double lik = ri[k] * rinv;
        for (int j0 = k + 1 + tc; j0 <= i; j0 += BC_VIL_CHOL_NJ * nc) {
          double lj[BC_VIL_CHOL_NJ] = {0.}, rv[BC_VIL_CHOL_NJ] = {0.};
          BC_VIL_UNROLL
          for (int c = 0; c < BC_VIL_CHOL_NJ; ++c) {
            const int j = j0 + c * nc;
            if (j <= i) { lj[c] = A[bc_vil_tri(j, k)]; rv[c] = ri[j]; }
          }
          BC_VIL_UNROLL
          for (int c = 0; c < BC_VIL_CHOL_NJ; ++c) {
            const int j = j0 + c * nc;
            if (j <= i) ri[j] = fma(-lik, lj[c] * rinv, rv[c]);
          }
        }
      }
    BC_VIL_SYNC();
    dd_prev = dd;
    rinv_prev = rinv;
  }
  return 0;
}

// x = C^-T y: y is row d of the packed triangle, C its leading block.  On the device one wave holds the running right-hand
// side in registers (two per lane) and hands each finished x_i round by a cross-lane read; callers put a barrier behind it.
BC_VIL_FN inline void bc_vil_backsolve(const double* A, const double* rdiag, int d, double* x, int tid) {
#ifdef __HIPCC__
  if (tid >= 64) return;
  double r0 = tid < d ? A[bc_vil_tri(d, tid)] : 0., r1 = tid + 64 < d ? A[bc_vil_tri(d, tid + 64)] : 0.;
  for (int i = d - 1; i >= 0; --i) {
    const double* ci = A + bc_vil_tri(i, 0);
    const double xi = __shfl(i < 64 ? r0 : r1, i & 63) * rdiag[i];
    if (tid == (i & 63)) { if (i < 64) r0 = xi; else r1 = xi; }
    if (tid < i) r0 = fma(-ci[tid], xi, r0);
    if (tid + 64 < i) r1 = fma(-ci[tid + 64], xi, r1);
  }
  if (tid < d) x[tid] = r0;
  if (tid + 64 < d) x[tid + 64] = r1;
#else
  if (tid != 0) return;
  for (int i = 0; i < d; ++i) x[i] = A[bc_vil_tri(d, i)];
  for (int i = d - 1; i >= 0; --i) {
    const double* ci = A + bc_vil_tri(i, 0);
    const double xi = x[i] * rdiag[i];
    x[i] = xi;
    for (int k = 0; k < i; ++k) x[k] = fma(-ci[k], xi, x[k]);
  }
#endif
}

// ---- the four stages of a fit.  bc_vi_laplace() below runs them in order; k_laplace_many (bc_laplace_small.hip) runs the same
// four and stores, between and after them, what bc_vi_laplace() computes but does not keep.
struct VilWs {             // the pieces of the BC_VIL_WS_DOUBLES(d) doubles of work space
  double* A;               // [H; g^T], then [C; y^T], packed: (i, k) at i (i + 1) / 2 + k
  double* Li;              // C^-1, packed
  double *mu, *stp, *cand;
  double* rdiag;           // 1 / C[k][k]
  double* red;             // [16]
  double* part;
};

struct VilFit {            // what the mode search found besides mu (block-uniform)
  double f;                // f(mu)
  double dec;              // the decrement of the last Newton system solved
  int steps, halvings, halvings_all;
};

BC_VIL_FN inline VilWs bc_vil_ws(double* ws, int d) {
  VilWs W;
  W.A = ws;
  W.Li = W.A + BC_VIL_TRI(d + 1);
  W.mu = W.Li + BC_VIL_TRI(d);
  W.stp = W.mu + d;
  W.cand = W.stp + d;
  W.rdiag = W.cand + d;
  W.red = W.rdiag + d;
  W.part = W.red + 16;
  return W;
}

// The mode search from the start point in a.mode: W.mu <- the mode; rowc keeps the m_n of the mode.  Returns 1 (block-uniform)
// when the run must stop; writes nothing but the work space and rowc.
BC_VIL_FN inline int bc_vil_mode(const VilArgs& a, const VilWs& W, VilFit* fit) {
  const int tid = BC_VIL_TID, nt = BC_VIL_NT;
  const int d = a.d, m = a.m;
  double *A = W.A, *mu = W.mu, *stp = W.stp, *cand = W.cand, *rdiag = W.rdiag, *red = W.red, *part = W.part;
  int grp = 1;                                  // lanes per row of the value pass
  while (grp < 16 && 2 * grp <= nt && (long)m * (2 * grp) <= nt && 2 * grp <= d) grp *= 2;
  for (int j = tid; j < d; j += nt) mu[j] = a.mode[j];
  BC_VIL_SYNC();
  double f = bc_vil_value(a, mu, red, grp, tid, nt);
  if (!(f - f == 0.)) return 1;                 // a weight, a row or the start point is not finite
  int steps = 0, halvings = 0, halvings_all = 0;
  double dec = 0.;
  for (int iter = 0; iter < BC_VIL_MAX_ITER; ++iter) {
    bc_vil_row_coefs(a, tid, nt);
    BC_VIL_SYNC();
    bc_vil_gram(a, A, mu, part, tid, nt);
    BC_VIL_SYNC();
    if (bc_vil_chol(A, rdiag, d, d + 1, tid, nt)) return 1;
    dec = -A[bc_vil_tri(d, d)];                 // g . H^-1 g = y . y: the corner started at 0 and lost y_k^2 per column
    if (!(dec >= 0. && dec < INFINITY)) return 1;      // (a component of g that is not finite ends here)
    if (dec == 0.) break;                       // g == 0: the Newton step is 0, mu stays where it is
    bc_vil_backsolve(A, rdiag, d, stp, tid);
    BC_VIL_SYNC();
    // backtracking: Newton's full step once near the mode
    double t = 1., fc = f;
    halvings = 0;
    for (int h = 0; h <= BC_VIL_MAX_HALVINGS; ++h) {
      for (int j = tid; j < d; j += nt) cand[j] = mu[j] + t * stp[j];
      BC_VIL_SYNC();
      fc = bc_vil_value(a, cand, red, grp, tid, nt);
      if (fc != fc) return 1;
      if (fc >= f + 1e-4 * t * dec || t < 1e-10) break;
      t *= 0.5;
      halvings = h + 1;
    }
    if (!(fc - fc == 0.)) return 1;
    halvings_all += halvings;
    double smax = 0., mmax = 0.;
    for (int j = 0; j < d; ++j) {
      smax = fmax(smax, fabs(t * stp[j]));
      mmax = fmax(mmax, fabs(cand[j]));
    }
    BC_VIL_SYNC();
    for (int j = tid; j < d; j += nt) mu[j] = cand[j];
    BC_VIL_SYNC();
    f = fc;
    ++steps;
    // the host's rule: a FULL step whose decrement was at the rounding floor of f, or a step at the rounding floor of mu
    if ((t == 1. && dec <= 64. * 2.220446049250313e-16 * (1. + fabs(f))) || smax <= 1e-13 * (1. + mmax)) break;
  }
  fit->f = f;
  fit->dec = dec;
  fit->steps = steps;
  fit->halvings = halvings;
  fit->halvings_all = halvings_all;
  return 0;
}

// H at the mode into the packed triangle W.A (rowc holds the m_n of the last point evaluated, which is mu); ends with a barrier.
BC_VIL_FN inline void bc_vil_hessian(const VilArgs& a, const VilWs& W) {
  const int tid = BC_VIL_TID, nt = BC_VIL_NT;
  bc_vil_row_coefs(a, tid, nt);
  BC_VIL_SYNC();
  bc_vil_gram(a, W.A, W.mu, W.part, tid, nt);
  BC_VIL_SYNC();
}

// The factor and its inverse: W.A <- C = chol(H), W.Li <- C^-1 (both packed); ends with a barrier.  The diagonal form only
// looks at the diagonal of H.  Returns 1 (block-uniform) on a pivot that is not finite and positive.
BC_VIL_FN inline int bc_vil_factor(const VilArgs& a, const VilWs& W) {
  const int tid = BC_VIL_TID, nt = BC_VIL_NT;
  const int d = a.d;
  double *A = W.A, *Li = W.Li, *rdiag = W.rdiag;
  if (a.diag) {
    for (int j = 0; j < d; ++j) {
      const double h = A[bc_vil_tri(j, j)];
      if (!(h > 0. && h < INFINITY)) return 1;
    }
    return 0;
  }
  if (bc_vil_chol(A, rdiag, d, d, tid, nt)) return 1;
  // L = C^-1 by forward substitution on the identity, column by column, top to bottom
#ifdef __HIPCC__
  // four lanes per column: lane g takes the terms k = j + g, j + g + 4, ... of a row's sum, four at a time so that their LDS
  // latencies overlap; a butterfly adds the four partial sums (the same bits in all four); element (i, j) is stored by the
  // lane that will read it, so nobody reads what another lane wrote
  for (int j = tid >> 2; j < d; j += nt >> 2) {
    const int g = tid & 3;
    if (g == 0) Li[bc_vil_tri(j, j)] = rdiag[j];
    for (int i = j + 1; i < d; ++i) {
      const double* ci = A + bc_vil_tri(i, 0);
      double sum = 0.;
      int k = j + g;
      for (; k + 12 < i; k += 16) {
        const double c0 = ci[k], c1 = ci[k + 4], c2 = ci[k + 8], c3 = ci[k + 12];
        const double l0 = Li[bc_vil_tri(k, j)], l1 = Li[bc_vil_tri(k + 4, j)], l2 = Li[bc_vil_tri(k + 8, j)], l3 = Li[bc_vil_tri(k + 12, j)];
        sum = fma(c3, l3, fma(c2, l2, fma(c1, l1, fma(c0, l0, sum))));
      }
      for (; k < i; k += 4) sum = fma(ci[k], Li[bc_vil_tri(k, j)], sum);
      sum += __shfl_xor(sum, 1);
      sum += __shfl_xor(sum, 2);
      if (((i - j) & 3) == g) Li[bc_vil_tri(i, j)] = -sum * rdiag[i];
    }
  }
#else
  for (int j = tid; j < d; j += nt) {      // column j is one thread's (it reads what it wrote)
    Li[bc_vil_tri(j, j)] = rdiag[j];
    for (int i = j + 1; i < d; ++i) {
      double sum = 0.;
      const double* ci = A + bc_vil_tri(i, 0);
      for (int k = j; k < i; ++k) sum = fma(ci[k], Li[bc_vil_tri(k, j)], sum);
      Li[bc_vil_tri(i, j)] = -sum * rdiag[i];
    }
  }
#endif
  BC_VIL_SYNC();
  return 0;
}

// The draw: a.theta <- mu + E . L^T, or with the diagonal form mu + E / sqrt(diag H) from the H bc_vil_hessian left.
BC_VIL_FN inline void bc_vil_draw(const VilArgs& a, const VilWs& W) {
  const int tid = BC_VIL_TID, nt = BC_VIL_NT;
  const int d = a.d;
  const double *A = W.A, *Li = W.Li, *mu = W.mu;
  const int total = a.s * d;
  if (a.diag) {
    for (int e = tid; e < total; e += nt) {
      const int q = e / d, c = e - q * d;
      a.theta[(size_t)q * a.dk + c] = mu[c] + a.E[e] / sqrt(A[bc_vil_tri(c, c)]);
    }
    return;
  }
#ifdef __HIPCC__
  (void)total;
  const int lane = tid & 63, wv = tid >> 6, nw = nt >> 6, r = lane & 15, kq = lane >> 4;
  const int qt = (a.s + 15) >> 4, ct = (d + 15) >> 4;
  for (int it = wv; it < qt * ct; it += nw) {
    const int Q = it / ct, Cc = it - Q * ct, qa = Q * 16 + r, cb = Cc * 16 + r;
    const int kend = (Cc + 1) * 16 < d ? (Cc + 1) * 16 : d;      // L is lower: k <= c
    bc_vil_d4 acc = {0., 0., 0., 0.};
    for (int k0 = 0; k0 < kend; k0 += 4) {
      const int k = k0 + kq;
      const double av = (qa < a.s && k < d) ? a.E[(size_t)qa * d + k] : 0.;
      const double bv = (cb < d && k <= cb) ? Li[bc_vil_tri(cb, k)] : 0.;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
    }
    for (int q4 = 0; q4 < 4; ++q4) {
      const int q = Q * 16 + kq + 4 * q4;
      if (q < a.s && cb < d) a.theta[(size_t)q * a.dk + cb] = mu[cb] + acc[q4];
    }
  }
#else
  for (int e = tid; e < total; e += nt) {
    const int q = e / d, c = e - q * d;
    const double* eq = a.E + (size_t)q * d;
    const double* lc = Li + bc_vil_tri(c, 0);
    double acc = 0.;
    for (int k = 0; k <= c; ++k) acc = fma(eq[k], lc[k], acc);
    a.theta[(size_t)q * a.dk + c] = mu[c] + acc;
  }
#endif
}

// Returns 1 (block-uniform) when the run must stop; nothing has been written to theta, mode or counts then.
// ws: BC_VIL_WS_DOUBLES(d) doubles.
BC_VIL_FN inline int bc_vi_laplace(const VilArgs& a, double* ws) {
  const int tid = BC_VIL_TID, nt = BC_VIL_NT;
  const int d = a.d;
  const VilWs W = bc_vil_ws(ws, d);
  VilFit fit;
  if (bc_vil_mode(a, W, &fit)) return 1;
  bc_vil_hessian(a, W);
  if (bc_vil_factor(a, W)) return 1;
  bc_vil_draw(a, W);
  for (int j = tid; j < d; j += nt) a.mode[j] = W.mu[j];
  if (tid == 0) {
    a.mode[d] = fit.dec;
    a.counts[0] = fit.steps;
    a.counts[1] = fit.halvings;
    a.counts[2] += fit.steps;
    a.counts[3] = fit.halvings_all;
  }
  return 0;
}
