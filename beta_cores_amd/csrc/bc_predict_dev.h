// The arithmetic of k_linreg_predict (bc_predict.hip) that does not need the matrix cores, and EVERY summation order of the
// kernel.  Written in the host-compilable style of bc_score_dev.h: tests/predict_harness.cpp compiles this header with
// BC_PREDICT_FN = static and walks the lanes, the staged chunks, the blocks and the combine stage in a loop.
//
// For held-out rows [phi_n, y_n] and a Gaussian posterior N(mu, F F^T) of a linear head with noise and scale:
//
//   m_n   = phi_n . mu                       v_nj = (phi_n F)[j]              q_n = sum_j v_nj^2
//   var_n = noise + scale q_n                r_n  = y_n - m_n
//   ll    = sum_n -1/2 ((r_n^2 / var_n + log var_n) + log 2 pi)               sse = sum_n r_n^2
//
// Who computes what.  A block of BC_PRED_WAVES waves owns BC_PRED_ROWS_PER_BLOCK consecutive rows of ONE posterior and stages
// them BC_PRED_STAGE_ROWS(D) at a time.  The wave w owns the 16-column groups g = w, w + 8, w + 16, ... of F (a group: the
// columns 16 g .. 16 g + 15), a lane one column of a group.  The constants below depend on D alone -- never on T, Nt or the grid.
//
// Summation orders, all fixed here:
//   v_nj   one ascending chain over k (on the device: v_mfma_f64_16x16x4_f64 steps k = 0, 4, 8, ... over D zero-padded to a
//          multiple of 4, one accumulator carried through the k-panels of 128; here: bc_predict_dot).
//   q_n    a lane adds the squares of ITS column over the wave's groups in ascending g, starting from 0 (bc_predict_lane_q);
//          the 16 lanes of a row are added by the butterfly bc_predict_tree(16) (x[i] + x[i ^ 1], then ^ 2, ^ 4, ^ 8: every
//          lane ends with the same bits, addition being commutative); the waves' sums are added in wave order 0 .. 7 starting
//          from 0 (bc_predict_wave_q).  Columns from D on and waves without a group contribute exact zeros.
//   m_n    eight partial chains, part p over k = p, p + 8, p + 16, ... < D by fma from 0 (bc_predict_mean_part), added by the
//          butterfly bc_predict_tree(8).  The mean is made by the vector ALU: at D = 128 a 129th column on the matrix cores would
//          open a ninth group for eight waves.
//   rows   the thread i < STAGE_ROWS of a block adds the terms of the block's rows i, i + STAGE_ROWS, ... in ascending order,
//          from 0; the block's partial is the butterfly bc_predict_tree(64) over the threads (those from STAGE_ROWS on hold 0).
//   blocks a posterior's partials are added in ascending block (row chunk) order, from 0 (bc_predict_chunks).
// Nothing in a posterior's chain of operations depends on T, on its place in the batch, on the other posteriors or on whether
// the per-row outputs are written: its bits do not either.  All arithmetic is fp64 and built with -ffp-contract=off.
#pragma once
#include <math.h>
#include <stddef.h>

#ifndef BC_PREDICT_FN
#define BC_PREDICT_FN __device__
#endif

#define BC_PRED_ROWS_PER_BLOCK 192                         // rows of one posterior per block: at D = 128 F's 128 KiB of loads stay
                                                           // below the chunk's 192 KiB of float64 rows, and T = 1 with Nt = 50 000
                                                           // gives 261 blocks for 256 CUs; a multiple of both stage sizes
#define BC_PRED_MAX_DIM 512
#define BC_PRED_WAVES 8
#define BC_PRED_TILE 16                                    // rows per tile, columns per group
#define BC_PRED_PANEL 128                                  // the k-panel whose B operands a lane keeps in registers
#define BC_PRED_MEAN_PARTS 8
#define BC_PRED_STAGE_ROWS(d) ((d) <= BC_PRED_PANEL ? 64 : 32)
#define BC_PRED_KPAD(d) ((((d) + 3) >> 2) << 2)            // the padded length of the contraction
#define BC_PRED_GROUPS(d) (((d) + 15) >> 4)
#define BC_PRED_LOG_2PI 1.8378770664093453                 // log(2 pi) rounded to nearest

// the host's stand-in for the matrix cores: v_nj, one ascending fma chain over the zero-padded length; F row-major D x D
BC_PREDICT_FN inline double bc_predict_dot(const double* phi, const double* f, int d, int j) {
  double s = 0.;
  for (int k = 0; k < BC_PRED_KPAD(d); ++k) s = fma(k < d ? phi[k] : 0., (k < d && j < d) ? f[(size_t)k * d + j] : 0., s);
  return s;
}

// x[0 .. n) -> the butterfly sum, n a power of two <= 64 (x is overwritten; on the device: __shfl_xor of 1, 2, 4, ... n / 2)
BC_PREDICT_FN inline double bc_predict_tree(double* x, int n) {
  double y[64];
  for (int s = 1; s < n; s <<= 1) {
    for (int i = 0; i < n; ++i) y[i] = x[i] + x[i ^ s];
    for (int i = 0; i < n; ++i) x[i] = y[i];
  }
  return x[0];
}

// part p of the mean's eight chains
BC_PREDICT_FN inline double bc_predict_mean_part(const double* phi, const double* mu, int d, int p) {
  double s = 0.;
  for (int k = p; k < d; k += BC_PRED_MEAN_PARTS) s = fma(phi[k], mu[k], s);
  return s;
}

// the lane (wave w, column c of a group): the squares of its entries over the wave's groups; v: the row's D' >= 16 G entries
BC_PREDICT_FN inline double bc_predict_lane_q(const double* v, int groups, int w, int c) {
  double q = 0.;
  for (int g = w; g < groups; g += BC_PRED_WAVES) q += v[BC_PRED_TILE * g + c] * v[BC_PRED_TILE * g + c];
  return q;
}

// the waves' sums of one row, in wave order
BC_PREDICT_FN inline double bc_predict_wave_q(const double* qw, int stride) {
  double q = 0.;
  for (int w = 0; w < BC_PRED_WAVES; ++w) q += qw[(size_t)w * stride];
  return q;
}

// one row: the predictive variance, the squared residual, and the row's term of ll
BC_PREDICT_FN inline double bc_predict_row(double y, double m, double q, double noise, double scale, double* var, double* r2) {
  const double sq = scale * q;
  const double v = noise + sq;
  const double r = y - m;
  const double rr = r * r;
  *var = v;
  *r2 = rr;
  return -0.5 * ((rr / v + log(v)) + BC_PRED_LOG_2PI);
}

// a posterior's block partials part[c][2] = (ll, sse) in ascending block order
BC_PREDICT_FN inline void bc_predict_chunks(const double* part, long long chunks, double* ll, double* sse) {
  double a = 0., b = 0.;
  for (long long c = 0; c < chunks; ++c) {
    a += part[2 * c];
    b += part[2 * c + 1];
  }
  *ll = a;
  *sse = b;
}
