// The arithmetic of the chain summary (include/beta_cores_diag.h has the definitions) as block functions, for ONE coordinate of
// one problem each.  The coordinate's draws lie contiguously, chain after chain: x[c * n + i], c < C, i < n (the retained layout
// [p][j][c][i] of csrc/bc_diag.hip), so that sequence s = 2 c + half is the h consecutive doubles at x + c n + half (n - h).
//
//   bc_dg_mean      the mean over all N = n C draws and whether one of them is not finite
//   bc_dg_stage     the 2 C sequences into the block's LDS (when they fit; the functions below read either place)
//   bc_dg_moments   m_s and v_s of every sequence, then W, Bh, varplus and rhat
//   bc_dg_ess       the lag products pair by pair until P_k is not > 0 (block-uniform exit, the loop bound fixed at the
//                   number of pairs), Geyer's monotone sums on the way, then tau and ess
//   bc_dg_cov_entry one entry of the covariance from the per-chunk partial tiles, added in chunk order
//   bc_dg_cov_chunk_host  (host builds only) a chunk's partial tiles by plain loops: what the MFMA kernel of bc_diag.hip computes
//
// Written the way bc_psvi_many_dev.h is: every loop has a fixed bound, every sum a fixed order; the same text compiles for the
// host with tid = 0, nt = 1, one lane per wave and empty barriers (tests/diag_harness.cpp).  On the device a block is BC_DG_BLOCK
// threads: a wave takes the sequences wv, wv + 4, ... and its 64 lanes interleave over a sequence's draws; what is summed over
// sequences is summed by every thread alike from LDS, in ascending order, so every thread holds the same bits and every exit
// is block-uniform.
#pragma once
#include <math.h>
#include <stddef.h>

#define BC_DG_BLOCK 256
#define BC_DG_TILE 16                                  // a covariance tile: one MFMA tile
#define BC_DG_TILE_DOUBLES 256

#ifndef BC_DG_FN
#define BC_DG_FN __device__
#define BC_DG_HD __host__ __device__      // (index arithmetic the host side shares)
#define BC_DG_TID ((int)threadIdx.x)
#define BC_DG_NT BC_DG_BLOCK
#define BC_DG_LANES 64
#define BC_DG_SYNC() __syncthreads()
#define BC_DG_WAVE_SUM(v) bc_wave_sum_all(v)           // (bc_internal.h: the total in every lane, all 64 lanes active)
#define BC_DG_BLOCK_SUM(v, red) bc_block_sum(v, red)   // (bc_internal.h: the total in every thread; ends with a barrier)
#endif
#ifndef BC_DG_HD
#define BC_DG_HD BC_DG_FN
#endif

// the block's LDS behind the staged sequences: red [64] | m_s [2 C] | v_s [2 C] | a_s of the two lags of a pair [2][2 C]
#define BC_DG_WS_DOUBLES(c) (64 + 8 * (size_t)(c))
struct DgWs {
  double *red, *ms, *vs, *as;
  const double* seq;        // the staged sequences [2 C][h], or null: they are read where they lie
};

BC_DG_FN inline DgWs bc_dg_ws(double* lds, int c, bool staged) {
  DgWs w;
  w.red = lds;
  w.ms = lds + 64;
  w.vs = w.ms + 2 * c;
  w.as = w.vs + 2 * c;
  w.seq = staged ? w.as + 4 * c : nullptr;
  return w;
}

BC_DG_FN inline double bc_dg_nan() { return nan(""); }

// *mean of x[0 .. N) as x_0 + mean(x - x_0); returns 1 (block-uniform) when a draw is not finite.  Everything below works on the
// SHIFTED draws y = x - x_0 too (the sequences' moments and lag products do not depend on a common shift): a coordinate of
// mean 1e8 and unit spread loses nothing to its mean, and a constant coordinate is all zeros, so its mean is its value.
BC_DG_FN inline int bc_dg_mean(const double* x, int N, double* red, double* mean) {
  const int tid = BC_DG_TID, nt = BC_DG_NT;
  const double x0 = x[0];
  double s = 0., bad = 0.;
  for (int e = tid; e < N; e += nt) {
    const double v = x[e];
    s += v - x0;
    if (!(v - v == 0.)) bad = 1.;
  }
  s = BC_DG_BLOCK_SUM(s, red);
  bad = BC_DG_BLOCK_SUM(bad, red);
  *mean = x0 + s / (double)N;
  return bad != 0.;
}

// where sequence s lies: staged [s][h], or in the coordinate's draws
BC_DG_FN inline const double* bc_dg_seq(const double* x, const double* staged, int s, int n, int h) {
  return staged ? staged + (size_t)s * h : x + (size_t)(s >> 1) * n + ((s & 1) ? n - h : 0);
}

// the shifted sequences y = x - x_0 into dst [2 C][h]
BC_DG_FN inline void bc_dg_stage(const double* x, int n, int c, double* dst) {
  const int tid = BC_DG_TID, nt = BC_DG_NT, h = n / 2;
  const double x0 = x[0];
  for (int e = tid; e < 2 * c * h; e += nt) {
    const int s = e / h;
    dst[e] = bc_dg_seq(x, nullptr, s, n, h)[e - s * h] - x0;
  }
  BC_DG_SYNC();
}
// what a reader of bc_dg_seq's draws subtracts to get y: nothing from the staged ones (y - 0 is y: the same bits either way)
BC_DG_FN inline double bc_dg_shift(const double* x, const double* staged) { return staged ? 0. : x[0]; }

// out[0] = W, out[1] = varplus, out[2] = rhat: the same bits in every thread.  Leaves m_s (of y) and v_s in W.ms / W.vs.
BC_DG_FN inline void bc_dg_moments(const double* x, int n, int c, const DgWs& W, double* out) {
  const int tid = BC_DG_TID, nt = BC_DG_NT, lane = tid % BC_DG_LANES, wv = tid / BC_DG_LANES, nw = nt / BC_DG_LANES;
  const int h = n / 2, S = 2 * c;
  const double sh = bc_dg_shift(x, W.seq);
  for (int s = wv; s < S; s += nw) {                  // (wave-uniform)
    const double* q = bc_dg_seq(x, W.seq, s, n, h);
    double sum = 0.;
    for (int i = lane; i < h; i += BC_DG_LANES) sum += q[i] - sh;
    sum = BC_DG_WAVE_SUM(sum);
    const double m = sum / (double)h;                 // (of y: the sequence's mean less x_0)
    double ss = 0.;
    for (int i = lane; i < h; i += BC_DG_LANES) {
      const double dl = (q[i] - sh) - m;
      ss += dl * dl;
    }
    ss = BC_DG_WAVE_SUM(ss);
    if (lane == 0) {
      W.ms[s] = m;
      W.vs[s] = ss / (double)(h - 1);
    }
  }
  BC_DG_SYNC();
  double w = 0., mm = 0., b = 0.;
  for (int s = 0; s < S; ++s) {
    w += W.vs[s];
    mm += W.ms[s];
  }
  w /= (double)S;
  mm /= (double)S;
  for (int s = 0; s < S; ++s) {
    const double dl = W.ms[s] - mm;
    b += dl * dl;
  }
  b /= (double)(S - 1);
  const double vp = (double)(h - 1) / (double)h * w + b;
  out[0] = w;
  out[1] = vp;
  out[2] = w == 0. ? bc_dg_nan() : sqrt(vp / w);
}

// *ess and *truncated from W = wv[0] and varplus = wv[1] (bc_dg_moments' values: m_s is read from W.ms).  rho: [L + 1] or null;
// written by thread 0: rho_0 = 1, every rho_t that was evaluated, NaN behind them.
BC_DG_FN inline void bc_dg_ess(const double* x, int n, int c, long long max_lag, const DgWs& W, const double* wvp, double* rho, double* ess,
                               int* truncated) {
  const int tid = BC_DG_TID, nt = BC_DG_NT, lane = tid % BC_DG_LANES, wv = tid / BC_DG_LANES, nw = nt / BC_DG_LANES;
  const int h = n / 2, S = 2 * c, L = max_lag < (long long)(h - 1) ? (int)max_lag : h - 1, pairs = (L + 1) / 2;
  const double w = wvp[0], vp = wvp[1], sh = bc_dg_shift(x, W.seq);
  double sum = 0., prev = 0.;
  int K = 0, full = 1;
  for (int k = 0; k < pairs; ++k) {
    const int t0 = 2 * k, t1 = t0 + 1;
    for (int s = wv; s < S; s += nw) {                // (wave-uniform)
      const double* q = bc_dg_seq(x, W.seq, s, n, h);
      const double m = W.ms[s];
      double a0 = 0., a1 = 0.;
      if (k > 0)
        for (int i = lane; i < h - t0; i += BC_DG_LANES) a0 += ((q[i] - sh) - m) * ((q[i + t0] - sh) - m);
      for (int i = lane; i < h - t1; i += BC_DG_LANES) a1 += ((q[i] - sh) - m) * ((q[i + t1] - sh) - m);
      a0 = BC_DG_WAVE_SUM(a0);
      a1 = BC_DG_WAVE_SUM(a1);
      if (lane == 0) {
        W.as[s] = a0 / (double)h;
        W.as[S + s] = a1 / (double)h;
      }
    }
    BC_DG_SYNC();
    double ab0 = 0., ab1 = 0.;
    for (int s = 0; s < S; ++s) {
      ab0 += W.as[s];
      ab1 += W.as[S + s];
    }
    ab0 /= (double)S;
    ab1 /= (double)S;
    const double r0 = k == 0 ? 1. : 1. - (w - ab0) / vp, r1 = 1. - (w - ab1) / vp;
    if (rho && tid == 0) {
      rho[t0] = r0;
      rho[t1] = r1;
    }
    const double pk = r0 + r1;
    BC_DG_SYNC();                                     // (a_s is written again by the next pair)
    if (!(pk > 0.)) {                                 // (block-uniform: every thread added the same numbers in the same order)
      full = 0;
      break;
    }
    prev = (k == 0 || pk < prev) ? pk : prev;
    sum += prev;
    ++K;
  }
  if (rho && tid == 0)
    for (int t = full ? 2 * pairs : 2 * K + 2; t <= L; ++t) rho[t] = bc_dg_nan();
  const double tau = -1. + 2. * sum;
  *ess = K == 0 ? bc_dg_nan() : (double)((long long)S * h) / tau;
  *truncated = full;
}

// ---- the covariance: tiles of 16 x 16 on or above the diagonal, numbered row by row
BC_DG_HD inline int bc_dg_tiles(int d) {
  const int t = (d + BC_DG_TILE - 1) / BC_DG_TILE;
  return t * (t + 1) / 2;
}
BC_DG_HD inline int bc_dg_tile_index(int nt16, int I, int J) { return I * nt16 - I * (I - 1) / 2 + (J - I); }      // I <= J
BC_DG_HD inline void bc_dg_tile_ij(int nt16, int tile, int* I, int* J) {
  int i = 0;
  while (i + 1 < nt16 && tile >= nt16 - i) {
    tile -= nt16 - i;
    ++i;
  }
  *I = i;
  *J = i + tile;
}

// cov[a][b] of one problem from its partial tiles part[chunk][tile][16][16]: the chunks added in order, then / (N - 1).  The entry
// below the diagonal is the one above it (within a diagonal tile too), so the matrix is symmetric bit for bit.
BC_DG_FN inline double bc_dg_cov_entry(const double* part, int chunks, int d, int a, int b, int N) {
  const int nt16 = (d + BC_DG_TILE - 1) / BC_DG_TILE, T = nt16 * (nt16 + 1) / 2;
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  const size_t off = (size_t)bc_dg_tile_index(nt16, lo / BC_DG_TILE, hi / BC_DG_TILE) * BC_DG_TILE_DOUBLES + (lo % BC_DG_TILE) * BC_DG_TILE + hi % BC_DG_TILE;
  double s = 0.;
  for (int ch = 0; ch < chunks; ++ch) s += part[(size_t)ch * T * BC_DG_TILE_DOUBLES + off];
  return s / (double)(N - 1);
}

#ifndef __HIPCC__
// one chunk's partial tiles [T][16][16] of the draws r0 <= r < r1 of a problem x[j][r] (d coordinates, N draws each), centred by
// mean: the sum over r ascending, one fma per term (the matrix cores' accumulation is such a chain)
static inline void bc_dg_cov_chunk_host(const double* x, const double* mean, int d, int N, int r0, int r1, double* part) {
  const int nt16 = (d + BC_DG_TILE - 1) / BC_DG_TILE, T = nt16 * (nt16 + 1) / 2;
  for (int tile = 0; tile < T; ++tile) {
    int I, J;
    bc_dg_tile_ij(nt16, tile, &I, &J);
    for (int i = 0; i < BC_DG_TILE; ++i)
      for (int j = 0; j < BC_DG_TILE; ++j) {
        const int a = I * BC_DG_TILE + i, b = J * BC_DG_TILE + j;
        double acc = 0.;
        if (a < d && b < d)
          for (int r = r0; r < r1; ++r) acc = fma(x[(size_t)a * N + r] - mean[a], x[(size_t)b * N + r] - mean[b], acc);
        part[(size_t)tile * BC_DG_TILE_DOUBLES + i * BC_DG_TILE + j] = acc;
      }
  }
}
#endif
