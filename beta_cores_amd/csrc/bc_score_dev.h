// The arithmetic of k_lr_score (bc_score.hip) that does not need the matrix cores: what one lane does with its share of a
// 16 thetas x 16 rows tile of margins, and how a theta's four lane sums are combined.  Written in the host-compilable style of
// bc_hmc_dev.h: tests/score_harness.cpp compiles this header with BC_SCORE_FN = static and walks the lanes in a loop.
//
// For held-out rows z_n = y_n x_n (the labels y_n = +-1 are kept beside them) and a parameter vector theta:
//
//   s_n = z_n . theta        ll(theta) = sum_n ll(-s_n)        correct(theta) = #{n : the reference predicts y_n}
//
// with ll(m) the log-likelihood of lr_terms (bc_lr_terms.h): the same expressions, the branch at m = 100 kept.
//
// The prediction rule.  The reference (model_lr.py:32-42) predicts -1 iff log_likelihood(-x, theta) > log_likelihood(x, theta)
// and +1 otherwise, a tie included; the log-likelihood falls with m = -x . theta, so that is -1 iff x . theta < 0.  In terms of
// s = z . theta = y (x . theta) a row is predicted correctly
//
//   iff  (y = +1 and s >= 0)  or  (y = -1 and s > 0).
//
// An exact zero of either sign is a tie and predicts +1 (an all-zero row is "correct" for y = +1 only).  The rule gives the
// reference's prediction for every margin with |x . theta| >= 1.5e-16, beyond +-100 and +-745 (where exp underflows) too.  For
// 0 < |x . theta| < about 2.2e-16 the reference's two log-likelihoods can round to the same double, and it then predicts +1
// where the sign says -1: that artefact of its rounding is NOT emulated here.
//
// Summation order.  The contraction over D is one ascending chain (on the device: v_mfma_f64_16x16x4_f64 steps k = 0, 4, 8, ...
// over D zero-padded to a multiple of 4; here: bc_score_dot).  The result tile has col = lane & 15 (the theta), row = (lane >> 4)
// + 4 reg, so the lane (h, t) of a wave sees the rows h, h + 4, h + 8, h + 12 of every tile for ITS theta t.  It adds their ll to
// its own sum in that order, tile after tile in ascending row order (bc_score_lane_tile); at the end the four lane sums of a
// theta are combined as (a0 + a1) + (a2 + a3) (bc_score_combine).  The counts are integers.  Nothing in a theta's chain of
// operations depends on T, on the theta's place in the batch or on the other thetas: its bits do not either.
#pragma once
#include <math.h>

#ifndef BC_SCORE_FN
#define BC_SCORE_FN __device__
#endif

#define BC_SCORE_TILE 16                                   // rows per tile, thetas per tile
#define BC_SCORE_KPAD(d) ((((d) + 3) >> 2) << 2)           // the padded length of the contraction

// ll of lr_terms (bc_lr_terms.h) for m = -s
BC_SCORE_FN inline double bc_score_ll(double m) {
  if (m < 100.) {
    const double e = exp(-fabs(m));
    return -(fmax(m, 0.) + log1p(e));
  }
  return -m;
}

// the prediction rule above
BC_SCORE_FN inline int bc_score_correct(double y, double s) { return y > 0. ? (s >= 0. ? 1 : 0) : (s > 0. ? 1 : 0); }

// the host's stand-in for the matrix cores: one ascending fma chain over the zero-padded length
BC_SCORE_FN inline double bc_score_dot(const double* z, const double* th, int d) {
  double s = 0.;
  for (int k = 0; k < BC_SCORE_KPAD(d); ++k) s = fma(k < d ? z[k] : 0., k < d ? th[k] : 0., s);
  return s;
}

// one lane's share of the tile whose first row is r0: s[reg], y[reg] belong to row r0 + h + 4 reg; rows from nt on do not exist
BC_SCORE_FN inline void bc_score_lane_tile(const double* s, const double* y, long long r0, int h, long long nt, double* acc, int* cnt) {
  for (int reg = 0; reg < 4; ++reg) {
    if (r0 + h + 4 * reg < nt) {
      *acc += bc_score_ll(-s[reg]);
      *cnt += bc_score_correct(y[reg], s[reg]);
    }
  }
}

// a theta's four lane sums
BC_SCORE_FN inline double bc_score_combine(double a0, double a1, double a2, double a3) { return (a0 + a1) + (a2 + a3); }
