// The in-block rows pass of the batched small-problem HMC run (include/beta_cores_hmc_small.h): value and gradient of the weighted
// logistic likelihood of ONE problem at ONE parameter vector, over rows that one thread block holds in its work space (LDS on
// the device), written in the host-compilable style of bc_hmc_dev.h (BC_HMC_FN / BC_HMC_TID / BC_HMC_NT / BC_HMC_SYNC).
//
//   m_i = -z_i . theta        value = sum_i w_i ll(m_i)        grad = sum_i (w_i p(m_i)) z_i        (ll, p: lr_terms of bc_lr_terms.h)
//
// Row layout.  Row i occupies zs[i * ld .. i * ld + d - 1] with ld = BC_HMC_SMALL_LD(d) = d | 1: the smallest ODD stride.  Phase A
// reads row-wise (thread = row, all lanes at the same column: doubles i * ld + k -- with an odd ld the 32 lanes of a ds_read_b64
// group fall on 32 different bank pairs, and the 16 lanes of a ds_read2_b64 group on 16), phase B reads column-wise (thread =
// column, all lanes in the same row: consecutive doubles).  The rows and the weights are only read, so the chains of a block may
// share them; w p and ll are per chain.  The value is "column d" of phase B: sum_i w_i ll_i.
//
// Summation order (no atomics; nothing depends on the thread count):
//   m_i        one ascending fma chain over the D columns, by one thread
//   grad, value  rows are cut into segments of BC_HMC_SMALL_SEG consecutive rows; one thread sums (segment, column) as an ascending
//              fma chain over the segment's rows into part[segment][column]; one thread per column then adds the segments in
//              ascending order, starting from the first
// so the same text on the host (tid = 0, nt = 1) walks the same chains (tests/hmc_small_harness.cpp).
#pragma once
#include <math.h>

#define BC_HMC_SMALL_SEG 64
#define BC_HMC_SMALL_LD(d) ((d) | 1)
#define BC_HMC_SMALL_NSEG(n) (((n) + BC_HMC_SMALL_SEG - 1) / BC_HMC_SMALL_SEG)
// the work space of bc_hmc_small_rows_pass for n rows of d columns, in doubles: what the chains of a block share (rows | w) and
// what each chain needs for itself (w p | ll | part)
#define BC_HMC_SMALL_ROWS_DOUBLES(n, d) ((size_t)(n) * (BC_HMC_SMALL_LD(d) + 1))
#define BC_HMC_SMALL_CHAIN_DOUBLES(n, d) (2 * (size_t)(n) + (size_t)BC_HMC_SMALL_NSEG(n) * ((d) + 1))

#ifndef BC_HMC_FN
#define BC_HMC_FN __device__
#define BC_HMC_TID ((int)threadIdx.x)
#define BC_HMC_NT ((int)blockDim.x)
#define BC_HMC_SYNC() do { __threadfence_block(); __syncthreads(); } while (0)
#endif

// lr_terms of bc_lr_terms.h without the curvature term: the same expressions, the branch at m = 100 kept
BC_HMC_FN inline void bc_hmc_small_terms(double m, int value, double* ll, double* p) {
  if (m < 100.) {
    const double e = exp(-fabs(m)), ope = 1. + e;
    if (value) *ll = -(fmax(m, 0.) + log1p(e));
    *p = m >= 0. ? 1. / ope : e / ope;
  } else {
    *ll = -m;
    *p = 1.;
  }
}

// red[0] = value (only when `value`, else untouched), red[1 + k] = grad[k] at th [d].  zs: n rows at stride BC_HMC_SMALL_LD(d);
// w [n]; wp [n], ll [n] and part [nseg][d + 1]: this chain's scratch.  th must be visible to the block on entry (a barrier after
// its last write); red is visible on return.
BC_HMC_FN inline void bc_hmc_small_rows_pass(const double* zs, const double* w, int n, int d, const double* th, int value, double* wp,
                                             double* ll, double* part, double* red) {
  const int tid = BC_HMC_TID, nt = BC_HMC_NT;
  const int ld = BC_HMC_SMALL_LD(d), nseg = BC_HMC_SMALL_NSEG(n);
  for (int i = tid; i < n; i += nt) {
    const double* z = zs + (size_t)i * ld;
    double s = 0.;
    for (int k = 0; k < d; ++k) s = fma(z[k], th[k], s);
    double l = 0., p;
    bc_hmc_small_terms(-s, value, &l, &p);
    wp[i] = w[i] * p;
    if (value) ll[i] = l;
  }
  BC_HMC_SYNC();
  const int nc = value ? d + 1 : d;      // column d: the value
  for (int it = tid; it < nseg * nc; it += nt) {
    const int sg = it / nc, k = it - sg * nc;
    const int i0 = sg * BC_HMC_SMALL_SEG, i1 = i0 + BC_HMC_SMALL_SEG < n ? i0 + BC_HMC_SMALL_SEG : n;
    double acc = 0.;
    if (k == d)
      for (int i = i0; i < i1; ++i) acc = fma(w[i], ll[i], acc);
    else
      for (int i = i0; i < i1; ++i) acc = fma(wp[i], zs[(size_t)i * ld + k], acc);
    part[sg * (d + 1) + k] = acc;
  }
  BC_HMC_SYNC();
  for (int k = tid; k < nc; k += nt) {
    double acc = part[k];
    for (int sg = 1; sg < nseg; ++sg) acc += part[sg * (d + 1) + k];
    red[k == d ? 0 : 1 + k] = acc;
  }
  BC_HMC_SYNC();
}
