// The device side of one greedy step of the sparse-NNLS solver: the single-block building blocks (xw and its error, the next
// sweep vectors, the pick, the step sizes, the reweight), the OrthoPursuit placement and Gram update, and the stages of the
// guarded iteration (fin_*).  Included by bc_snnls.hip ONLY, whose kernels are thin sequences of these functions: the fused
// loop's finish kernels and the step-wise protocol's kernels share them, which is what makes the two produce the same bits.
// Every __shared__ object is declared inside the function that uses it.  FSTAMP comes from the including unit's diagnostic
// build (-DBC_FIN_STAMPS), else from bc_rescore_dev.h, where it is empty.
#pragma once
#include "bc_snnls_state.h"
#include "bc_i8_quant.h"
#include "bc_i4_quant.h"
#include <climits>
#include <cmath>

// ------------------------------------------------------------------ device building blocks (single block)
// The S-vector algebra of a step (dot products, step sizes, the next sweep vectors) is done by WAVE 0 alone:
// lane l owns elements l, l+64, ... of every vector and reductions are shuffle trees, so a step needs a handful
// of block barriers instead of three per reduction.  Only the O(nnz*S) work -- rebuilding xw from the list,
// scaling / searching the list -- uses the whole block.  Every kernel goes through the same helpers, so the
// fused loop and the step-wise protocol produce the same bits.

// xw = sum_j val[j] * cols[j], err = ||xw - b||, ||xw||^2 and the positive count.  The list is split over
// G = blockDim/S thread groups (fixed split => deterministic), partial vectors are combined in group order.
#define BC_PF_NC 16     // list columns per thread requested up front by the _pf kernels (32 was measured: no gain)
// PF: the first BC_PF_NC terms of every thread's share come from `c16` (cols prefetched at kernel start, slot u <->
// list entry g + u*G) except the entry appended in this very step (`at_new`), whose column is P.xf.
template <bool PF>
__device__ void dev_xw_err_t(const SnnlsDev& P, SnnlsState& S, double* red, const double (&c16)[BC_PF_NC], long long at_new) {
  __shared__ double part[BC_FIN_THREADS];
  __shared__ int npos_sh;
  const int s = P.s;
  const long long nnz = S.nnz;
  if (threadIdx.x == 0) npos_sh = 0;
  __syncthreads();
  int np = 0;
  if (s <= (int)blockDim.x) {
    const int G = blockDim.x / s;
    const int g = threadIdx.x / s, k = threadIdx.x - g * s;
    double acc = 0.0;
    if (g < G) {
      // 16 independent loads in flight per thread: the list lives in global memory (L2) and a dependent
      // load per term would cost a full memory latency each.  The k == 0 thread of each group also counts
      // the positive weights it walks over (every list slot belongs to exactly one group).
      long long j = g;
      if (PF) {
#pragma unroll
        for (int u = 0; u < BC_PF_NC; ++u) {
          if (j < nnz) {
            const double vj = P.val[j];
            const double cv = (j == at_new) ? P.xf[k] : c16[u];
            acc = fma(vj, cv, acc);
            np += (vj > 0.) ? 1 : 0;
            j += G;
          }
        }
      }
      for (; j + 15 * (long long)G < nnz; j += 16 * (long long)G) {
        double v8[16], c8[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          v8[u] = P.val[j + u * (long long)G];
          c8[u] = P.cols[(size_t)(j + u * (long long)G) * s + k];
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          acc = fma(v8[u], c8[u], acc);
          np += (v8[u] > 0.) ? 1 : 0;
        }
      }
      for (; j + 3 * (long long)G < nnz; j += 4 * (long long)G) {
        double v4[4], c4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          v4[u] = P.val[j + u * (long long)G];
          c4[u] = P.cols[(size_t)(j + u * (long long)G) * s + k];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          acc = fma(v4[u], c4[u], acc);
          np += (v4[u] > 0.) ? 1 : 0;
        }
      }
      for (; j < nnz; j += G) {
        const double vj = P.val[j];
        acc = fma(vj, P.cols[(size_t)j * s + k], acc);
        np += (vj > 0.) ? 1 : 0;
      }
      if (k == 0 && np) atomicAdd(&npos_sh, np);
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x < BC_WAVE) {
      double e = 0.0, q = 0.0;
      for (int kk = threadIdx.x; kk < s; kk += BC_WAVE) {
        double t = part[kk];
        for (int gg = 1; gg < G; ++gg) t += part[gg * s + kk];
        P.xw[kk] = t;
        const double d = t - P.b[kk];
        e = fma(d, d, e);
        q = fma(t, t, q);
      }
      e = bc_wave_sum(e);
      q = bc_wave_sum(q);
      if (threadIdx.x == 0) {
        S.err_cur = sqrt(e);
        S.xw_sq = q;
        S.npos = npos_sh;
      }
    }
  } else {
    for (long long j = threadIdx.x; j < nnz; j += blockDim.x) np += (P.val[j] > 0.) ? 1 : 0;
    if (np) atomicAdd(&npos_sh, np);
    double e = 0.0, q = 0.0;
    for (int k = threadIdx.x; k < s; k += blockDim.x) {
      double acc = 0.0;
      for (long long j = 0; j < nnz; ++j) acc = fma(P.val[j], P.cols[(size_t)j * s + k], acc);
      P.xw[k] = acc;
      const double d = acc - P.b[k];
      e = fma(d, d, e);
      q = fma(acc, acc, q);
    }
    double r2[2] = {e, q};
    bc_block_sum_n<2>(r2, red);
    if (threadIdx.x == 0) {
      S.err_cur = sqrt(r2[0]);
      S.xw_sq = r2[1];
      S.npos = npos_sh;
    }
  }
  __syncthreads();
}

__device__ void dev_xw_err(const SnnlsDev& P, SnnlsState& S, double* red) {
  const double none[BC_PF_NC] = {0.};
  dev_xw_err_t<false>(P, S, red, none, -1);
}

// vectors for the next sweep.  GIGA: giga.py:21-30 ; FW / OMP: residual b - A.w          (wave 0 + one barrier)
// With an int8 pre-filter (P.qv) the same wave also leaves the vectors' int8 digits behind (bc_i8_quant.h): the maxima are
// taken while the elements are in registers, and the digits' pass reads them back from a 4 KB LDS copy (S <= BC_VQ_MAX;
// larger S re-reads v from global memory).
#define BC_VQ_MAX 256
#ifndef BC_QD_INTS
#define BC_QD_INTS 512
#endif
template <int ALG>
__device__ void dev_prep(const SnnlsDev& P, SnnlsState& S, double* red) {
  __shared__ double vq[2 * BC_VQ_MAX];
  __shared__ int qd[BC_QD_INTS];           // LDS image of the two digit records (S <= ~256)
  const int s = P.s;
  if (threadIdx.x < BC_WAVE) {
    const int lane = threadIdx.x;
    const bool quant = P.qv != nullptr;
    const bool lds_copy = quant && s <= BC_VQ_MAX;
    double vnorm = 1.;                  // ||v|| of the sweep vector (GIGA's are unit vectors)
    double m0 = 0., m1 = 0.;            // this lane's max |v0|, |v1|
    if (ALG == BC_ALG_GIGA) {
      double nw = sqrt(S.xw_sq);
      nw = (nw == 0.) ? 1. : nw;
      double bd = 0.0;
      for (int k = lane; k < s; k += BC_WAVE) {
        const double xn = P.xw[k] / nw;
        P.v[2 * k + 1] = xn;
        if (lds_copy) vq[2 * k + 1] = xn;
        m1 = bc_i8q_absmax(m1, xn);
        bd = fma(P.bn[k], xn, bd);
      }
      bd = bc_wave_sum_all(bd);
      double cn = 0.0;
      for (int k = lane; k < s; k += BC_WAVE) {
        const double c = P.bn[k] - bd * (P.xw[k] / nw);
        cn = fma(c, c, cn);
      }
      cn = sqrt(bc_wave_sum_all(cn));
      const bool fail = cn < P.tol;
      for (int k = lane; k < s; k += BC_WAVE) {
        const double c = P.bn[k] - bd * (P.xw[k] / nw);
        const double v0 = fail ? c : c / cn;
        P.v[2 * k] = v0;
        if (lds_copy) vq[2 * k] = v0;
        m0 = bc_i8q_absmax(m0, v0);
      }
      if (lane == 0) S.select_fail = fail ? 1 : 0;
    } else {
      double vn = 0.0;
      for (int k = lane; k < s; k += BC_WAVE) {
        const double r = P.b[k] - P.xw[k];
        P.v[k] = r;
        if (lds_copy) vq[k] = r;
        m0 = bc_i8q_absmax(m0, r);
        vn = fma(r, r, vn);
      }
      vn = bc_wave_sum(vn);
      vnorm = sqrt(vn);
      if (lane == 0) {
        S.select_fail = 0;
        S.v_norm = vnorm;
      }
    }
    if (lane == 0) S.skip = S.select_fail | S.reached_limit | S.pf_overflow;
    FSTAMP(15);
    if (quant) {
      // this wave wrote v (and its LDS copy) itself: a wave-level fence orders the digits' reads behind those stores
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      const double* vsrc = lds_copy ? vq : P.v;
      m0 = bc_wave_max_all(m0);
      m1 = bc_wave_max_all(m1);
      if (4 * (P.sp4 + P.sp8) <= BC_QD_INTS) {
        // one element per lane, both records in one pass (bc_i4_quant.h: bc_q_wave_both)
        if (ALG == BC_ALG_GIGA) bc_q_wave_both<0>(vsrc, s, P.sp4, P.sp8, 1., P.qv, P.qv4, lane, m0, m1, qd);
        else bc_q_wave_both<1>(vsrc, s, P.sp4, P.sp8, vnorm, P.qv, P.qv4, lane, m0, m1, qd);
      } else {
        if (ALG == BC_ALG_GIGA) bc_i8q_wave<0>(vsrc, s, P.sp4, 1., P.qv, lane, m0, m1);
        else bc_i8q_wave<1>(vsrc, s, P.sp4, vnorm, P.qv, lane, m0, m1);
        if (P.qv4 != nullptr) {
          if (ALG == BC_ALG_GIGA) bc_i4q_wave<0>(vsrc, s, P.sp8, 1., P.qv4, lane, m0, m1);
          else bc_i4q_wave<1>(vsrc, s, P.sp8, vnorm, P.qv4, lane, m0, m1);
        }
      }
    }
  }
  __syncthreads();
}

// winner over the gathered candidate records: max score, lowest global index on ties.
// OMP additionally weighs the active set's negative direction (orthopursuit.py:25-35).
template <int ALG>
__device__ void dev_pick(const SnnlsDev& P, SnnlsState& S, double* red) {
  __shared__ int src_rec;
  __shared__ long long src_list;
  const int s = P.s;
  if (P.world == 1 && ALG != BC_ALG_OMP) {
    // one record: nothing to reduce (the shuffle argmax below costs ~3.5k cycles of ds_bpermute latency)
    const double* rec = P.cand_all;
    const bool valid = rec[3] != 0.0;
    if (threadIdx.x == 0) {
      S.sel_valid = valid ? 1 : 0;
      S.sel_f = valid ? reinterpret_cast<const long long*>(rec)[1] : -1;
      S.sel_score = valid ? rec[0] : -INFINITY;
      if (valid) S.sel_norm = rec[2];
    }
    if (P.xf != rec + BC_REC_HDR) {                 // (block-uniform; the fused kernel aliases the two)
      if (valid)
        for (int k = threadIdx.x; k < s; k += blockDim.x) P.xf[k] = rec[BC_REC_HDR + k];
    }
    __syncthreads();
    return;
  }
  if (threadIdx.x < BC_WAVE) {
    // wave 0: one record header per lane (independent loads), shuffle argmax on (score, global index)
    // carrying the record slot; the winner's column is copied straight from its record
    const int lane = threadIdx.x;
    double bv = -INFINITY;
    long long bi = LLONG_MAX;
    int br = -1;
    for (int r = lane; r < P.world; r += BC_WAVE) {
      const double* rec = P.cand_all + (size_t)r * P.rec_len;
      const double sc = rec[0], ok = rec[3];
      const long long gi = reinterpret_cast<const long long*>(rec)[1];
      if (ok != 0.0 && bc_better(sc, gi, bv, bi)) { bv = sc; bi = gi; br = r; }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const double ov = __shfl_down(bv, d, BC_WAVE);
      const long long oi = bc_shfl_down_ll(bi, d);
      const int orr = __shfl_down(br, d, BC_WAVE);
      if (bc_better(ov, oi, bv, bi)) { bv = ov; bi = oi; br = orr; }
    }
    br = __shfl(br, 0, BC_WAVE);
    const bool valid = br >= 0;
    const double* win = P.cand_all + (size_t)(valid ? br : 0) * P.rec_len;
    if (lane == 0) {
      S.sel_valid = valid ? 1 : 0;
      S.sel_f = valid ? bi : -1;
      S.sel_score = bv;
      if (valid) S.sel_norm = win[2];
      src_rec = br;
      src_list = -1;
    }
    if (ALG != BC_ALG_OMP && valid)
      for (int k = lane; k < s; k += BC_WAVE) P.xf[k] = win[BC_REC_HDR + k];
  }
  __syncthreads();
  if (ALG != BC_ALG_OMP) return;
  if (ALG == BC_ALG_OMP && S.sel_valid && S.npos > 0) {
    // neg = max over active j of -(An[:,j] . residual)
    __shared__ double nv[16];
    __shared__ long long ni[16], nj[16];
    double bv = -INFINITY;
    long long bi = LLONG_MAX, bj = -1;
    for (long long j = threadIdx.x; j < S.nnz; j += blockDim.x) {
      if (!(P.val[j] > 0.)) continue;
      double acc = 0.0;
      for (int k = 0; k < s; ++k) acc = fma(P.cols[(size_t)j * s + k], P.v[k], acc);
      const double d = -(acc / P.colnorm[j]);
      if (bc_better(d, P.idx[j], bv, bi)) { bv = d; bi = P.idx[j]; bj = j; }
    }
    // block argmax carrying the list slot
    for (int dlt = 32; dlt >= 1; dlt >>= 1) {
      const double ov = __shfl_down(bv, dlt, BC_WAVE);
      const long long oi = bc_shfl_down_ll(bi, dlt), oj = bc_shfl_down_ll(bj, dlt);
      if (bc_better(ov, oi, bv, bi)) { bv = ov; bi = oi; bj = oj; }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { nv[wave] = bv; ni[wave] = bi; nj[wave] = bj; }
    __syncthreads();
    if (threadIdx.x == 0) {
      const int nwv = (blockDim.x + 63) >> 6;
      for (int w = 1; w < nwv; ++w)
        if (bc_better(nv[w], ni[w], bv, bi)) { bv = nv[w]; bi = ni[w]; bj = nj[w]; }
      if (!(S.sel_score >= bv)) {   // orthopursuit.py:31 `if pos >= neg` else take the active point
        S.sel_f = bi;
        S.sel_score = bv;
        S.sel_norm = P.colnorm[bj];
        src_rec = -1;
        src_list = bj;
      }
    }
    __syncthreads();
  }
  if (S.sel_valid) {
    const double* src = (src_rec >= 0) ? P.cand_all + (size_t)src_rec * P.rec_len + BC_REC_HDR
                                       : P.cols + (size_t)src_list * s;
    for (int k = threadIdx.x; k < s; k += blockDim.x) P.xf[k] = src[k];
  }
  __syncthreads();
}

// single-rank variant of dev_pick: reduce the sweep's per-block candidates here (no record round trip)
__device__ void dev_pick_blocks(const SnnlsDev& P, SnnlsState& S) {
  __shared__ double sv[16];
  __shared__ long long si[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double bv = -INFINITY;
  long long bi = LLONG_MAX;
  for (int i = threadIdx.x; i < P.nblk; i += blockDim.x)
    if (bc_better(P.blk_val[i], P.blk_idx[i], bv, bi)) { bv = P.blk_val[i]; bi = P.blk_idx[i]; }
  bc_wave_argmax(bv, bi);
  if (lane == 0) { sv[wave] = bv; si[wave] = bi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int nwv = (blockDim.x + 63) >> 6;
    for (int w = 1; w < nwv; ++w)
      if (bc_better(sv[w], si[w], bv, bi)) { bv = sv[w]; bi = si[w]; }
    const bool valid = bi != LLONG_MAX;
    S.sel_valid = valid ? 1 : 0;
    S.sel_f = valid ? bi : -1;
    S.sel_score = bv;
    S.sel_norm = valid ? P.norms[bi - P.row_offset] : 0.0;
  }
  __syncthreads();
  if (S.sel_valid) {
    const long long r = S.sel_f - P.row_offset;
    for (int k = threadIdx.x; k < P.s; k += blockDim.x) P.xf[k] = P.tiles[bc_tile_off(r, k, P.s)];
  }
  __syncthreads();
}

// closed-form step sizes.  Returns 1 when the reference would raise NumericalPrecisionError
// (w untouched), else 0 with (alpha, beta) set.                                    (wave 0 + one barrier)
template <int ALG>
__device__ int dev_step_sizes(const SnnlsDev& P, const SnnlsState& S, double* red, double& alpha, double& beta) {
  __shared__ double ab[2];
  __shared__ int ab_fail;
  const int s = P.s;
  if (threadIdx.x < BC_WAVE) {
    const int lane = threadIdx.x;
    int fail = 0;
    double al = 0., be = 0.;
    if (ALG == BC_ALG_GIGA) {   // giga.py:42-61
      double nw = sqrt(S.xw_sq);
      nw = (nw == 0.) ? 1. : nw;
      double ff = 0.;
      for (int k = lane; k < s; k += BC_WAVE) ff = fma(P.xf[k], P.xf[k], ff);
      const double nf = sqrt(bc_wave_sum_all(ff));
      double r0 = 0., r1 = 0., r2 = 0.;
      for (int k = lane; k < s; k += BC_WAVE) {
        const double fn = P.xf[k] / nf, wn = P.xw[k] / nw;
        r0 = fma(P.bn[k], fn, r0);
        r1 = fma(P.bn[k], wn, r1);
        r2 = fma(wn, fn, r2);
      }
      const double bxf = bc_wave_sum_all(r0), bxw = bc_wave_sum_all(r1), xwxf = bc_wave_sum_all(r2);
      const double gA = bxf - bxw * xwxf;
      const double gB = bxw - bxf * xwxf;
      if (gA <= 0. || gB < 0.) {
        fail = 1;
      } else {
        const double a = gB / (gA + gB) / nw;
        const double b = gA / (gA + gB) / nf;
        double nx = 0.;
        for (int k = lane; k < s; k += BC_WAVE) {
          const double x = a * P.xw[k] + b * P.xf[k];
          nx = fma(x, x, nx);
        }
        nx = sqrt(bc_wave_sum_all(nx));
        double xb = 0.;
        for (int k = lane; k < s; k += BC_WAVE) {
          const double x = a * P.xw[k] + b * P.xf[k];
          xb = fma(x / nx, P.bn[k], xb);
        }
        xb = bc_wave_sum_all(xb);
        const double scale = P.bnorm / nx * xb;
        al = a * scale;
        be = b * scale;
      }
    } else {                    // frankwolfe.py:20-37
      const double nf = S.sel_norm;
      if (S.npos == 0) {
        al = 0.;
        be = P.norm_sum / nf;
      } else {
        const double c = P.norm_sum / nf;
        double num = 0., den = 0.;
        for (int k = lane; k < s; k += BC_WAVE) {
          const double d = c * P.xf[k] - P.xw[k];
          num = fma(d, P.b[k] - P.xw[k], num);
          den = fma(d, d, den);
        }
        num = bc_wave_sum_all(num);
        den = bc_wave_sum_all(den);
        if (num < 0. || den == 0. || num > den) {
          fail = 1;
        } else {
          al = 1. - num / den;
          be = c * num / den;
        }
      }
    }
    if (lane == 0) {
      ab[0] = al;
      ab[1] = be;
      ab_fail = fail;
    }
  }
  __syncthreads();
  alpha = ab[0];
  beta = ab[1];
  return ab_fail;
}

// list slot `at` is about to hold another column (thread 0): the Gram state of the device NNLS refit, if this solver has one,
// no longer covers it
__device__ __forceinline__ void dev_gram_touch(const SnnlsDev& P, long long at) {
  if (P.nnls_stats != nullptr && P.nnls_stats[3] > at) P.nnls_stats[3] = at;
}

// w = alpha*w ; w[f] = max(0, w[f] + beta)   (giga.py:63-64, frankwolfe.py:39-40)
__device__ void dev_apply(const SnnlsDev& P, SnnlsState& S, double alpha, double beta) {
  __shared__ int slot;
  const int s = P.s;
  const long long f = S.sel_f;
  if (threadIdx.x == 0) slot = INT_MAX;
  __syncthreads();
  for (long long j = threadIdx.x; j < S.nnz; j += blockDim.x) {
    P.val[j] = alpha * P.val[j];
    if (P.idx[j] == f) atomicMin(&slot, (int)j);
  }
  __syncthreads();
  long long at = slot == INT_MAX ? -1 : slot;
  if (at >= 0) {
    if (threadIdx.x == 0) {
      const double nv = P.val[at] + beta;
      P.val[at] = nv > 0. ? nv : 0.;
    }
  } else {
    const double nv = (0. + beta) > 0. ? (0. + beta) : 0.;
    if (nv > 0.) {
      if (S.nnz < P.cap) {
        at = S.nnz;
        for (int k = threadIdx.x; k < s; k += blockDim.x) P.cols[(size_t)at * s + k] = P.xf[k];
        if (threadIdx.x == 0) {
          P.idx[at] = f;
          P.val[at] = nv;
          P.colnorm[at] = S.sel_norm;
          dev_gram_touch(P, at);
        }
        __syncthreads();
        if (threadIdx.x == 0) S.nnz = at + 1;
      } else if (threadIdx.x == 0) {
        S.overflow = 1;
      }
    }
  }
  __syncthreads();
}

__device__ __forceinline__ void dev_trace(const SnnlsDev& P, SnnlsState& S, long long f, int status) {
  if (threadIdx.x == 0) {
    if (S.iter < P.tr_cap) {
      P.tr_f[S.iter] = f;
      P.tr_status[S.iter] = status;
      P.tr_err[S.iter] = S.err_cur;
    }
    S.iter += 1;
  }
}

// any gathered record carrying the overflow marker?  (block-uniform; every rank sees the same records)
__device__ bool dev_records_overflow(const double* cand_all, int world, int rec_len) {
  __shared__ int ovf;
  if (threadIdx.x == 0) ovf = 0;
  __syncthreads();
  for (int r = threadIdx.x; r < world; r += blockDim.x)
    if (cand_all[(size_t)r * rec_len + 3] < 0.) ovf = 1;
  __syncthreads();
  return ovf != 0;
}

// column f -> P.xf (and its norm -> S.sel_norm) for a step-wise reweight: it is the last pick, or sits in a gathered
// record, or in the local shard.  Returns 0 (block-uniform) when this rank cannot supply it.
__device__ int dev_fetch_column(const SnnlsDev& P, SnnlsState& S, long long f) {
  __shared__ int found;
  const int s = P.s;
  if (threadIdx.x == 0) {
    int fd = 0;   // 0: not found, 1: xf already holds it, 2+r: record r, -1: local shard
    if (S.sel_valid && S.sel_f == f) fd = 1;
    if (!fd)
      for (int r = 0; r < P.world; ++r) {
        const double* rec = P.cand_all + (size_t)r * P.rec_len;
        if (rec[3] != 0.0 && reinterpret_cast<const long long*>(rec)[1] == f) { fd = 2 + r; break; }
      }
    if (!fd && f >= P.row_offset && f < P.row_offset + P.n_rows) fd = -1;
    found = fd;
  }
  __syncthreads();
  if (found == 0) return 0;
  if (found >= 2) {
    const double* rec = P.cand_all + (size_t)(found - 2) * P.rec_len;
    for (int k = threadIdx.x; k < s; k += blockDim.x) P.xf[k] = rec[BC_REC_HDR + k];
    if (threadIdx.x == 0) S.sel_norm = rec[2];
  } else if (found == -1) {
    const long long r = f - P.row_offset;
    for (int k = threadIdx.x; k < s; k += blockDim.x) P.xf[k] = P.tiles[bc_tile_off(r, k, s)];
    if (threadIdx.x == 0) S.sel_norm = P.norms[r];
  }
  if (threadIdx.x == 0) { S.sel_f = f; S.sel_valid = 1; }
  __syncthreads();
  return 1;
}

// ------------------------------------------------------------------ device NNLS refit (OrthoPursuit, optimize())
#include "bc_nnls_dev.h"

// would column f find a slot (dev_omp_place below): it is listed, or a slot has weight 0, or the list may grow
__device__ bool dev_omp_room(const SnnlsDev& P, const SnnlsState& S, long long f, long long limit) {
  __shared__ int room;
  const long long nnz = S.nnz;
  if (threadIdx.x == 0) room = nnz < limit ? 1 : 0;
  __syncthreads();
  for (long long j = threadIdx.x; j < nnz; j += blockDim.x)
    if (P.idx[j] == f || !(P.val[j] > 0.)) room = 1;
  __syncthreads();
  return room != 0;
}

// orthopursuit.py:38 `w[f] = 1` on the sparse list: make sure the picked column (S.sel_f, in P.xf) has a slot -- with weight
// 0 when it is new: the refit lets it enter.  A slot whose weight is 0 is reused before the list grows.  Returns the slot, or
// -1 when the list is full; *fresh: the slot's column was (re)written, so its Gram row is stale (the callers go straight on to
// dev_gram_update, which recomputes it).
__device__ long long dev_omp_place(const SnnlsDev& P, SnnlsState& S, long long limit, int* fresh) {
  __shared__ int hit, zero;
  const int s = P.s;
  const long long f = S.sel_f, nnz = S.nnz;
  if (threadIdx.x == 0) { hit = INT_MAX; zero = INT_MAX; }
  __syncthreads();
  for (long long j = threadIdx.x; j < nnz; j += blockDim.x) {
    if (P.idx[j] == f) atomicMin(&hit, (int)j);
    else if (!(P.val[j] > 0.)) atomicMin(&zero, (int)j);
  }
  __syncthreads();
  *fresh = 0;
  if (hit != INT_MAX) return hit;
  const long long at = zero != INT_MAX ? (long long)zero : nnz;
  if (at == nnz && at >= limit) return -1;
  for (int k = threadIdx.x; k < s; k += blockDim.x) P.cols[(size_t)at * s + k] = P.xf[k];
  if (threadIdx.x == 0) {
    P.idx[at] = f;
    P.val[at] = 0.;
    P.colnorm[at] = S.sel_norm;
    if (at == nnz) S.nnz = at + 1;
  }
  __syncthreads();
  *fresh = 1;
  return at;
}

// bring the Gram state up to the list: entries [covered, n) are new to it (covered = P.nnls_stats[3], never trusted beyond
// the list as it was when this kernel started), and so is a slot below them that was reused in this kernel
__device__ void dev_gram_update(const SnnlsDev& P, long long nnz0, long long n, long long at, int fresh) {
  const long long covered = P.nnls_stats[3];
  const long long from = covered < nnz0 ? covered : nnz0;
  __syncthreads();                 // every thread has read the mark before thread 0 moves it
  if (from < n) bc_nnls_gram_rows(P.cols, P.s, P.b, P.gram, P.gram_c, (int)n, (int)from, (int)n);
  if (fresh && at < from) bc_nnls_gram_rows(P.cols, P.s, P.b, P.gram, P.gram_c, (int)n, (int)at, (int)at + 1);
  if (threadIdx.x == 0) P.nnls_stats[3] = n;
}

// ------------------------------------------------------------------ stages of one guarded greedy iteration (snnls.py:41-74)
// Written once for the finish kernels below: the kernels differ in where the vectors and the list live and in the reweight in
// the middle, not in the guard, the retry rule or the close -- which is what keeps the fused loop and its forms bit-identical.

// the five S-vectors into dynamic LDS: P points there, b / bn / xw are copied in (the caller's barrier publishes them)
__device__ __forceinline__ void fin_stage_vecs(SnnlsDev& P, const SnnlsDev& P0, double* vec_lds) {
  const int s = P.s;
  P.b = vec_lds;
  P.bn = vec_lds + s;
  P.xw = vec_lds + 2 * s;
  P.xf = vec_lds + 3 * s;
  P.xw_prev = vec_lds + 4 * s;
  for (int k = threadIdx.x; k < s; k += blockDim.x) {
    P.b[k] = P0.b[k];
    P.bn[k] = P0.bn[k];
    P.xw[k] = P0.xw[k];
  }
}

// snnls.py:32-34 / :73-74: over the limit, or a pending exact redo: the step consumes nothing
__device__ __forceinline__ bool fin_idle(const SnnlsState& S) { return S.reached_limit || S.pf_overflow; }

// a pre-filter's candidate lists overflowed in this step: mark it (sticky until the host's exact redo) and consume nothing
__device__ __forceinline__ void fin_refuse_overflow(SnnlsState& S, SnnlsState* st) {
  if (threadIdx.x == 0) { S.pf_overflow = 1; S.skip = 1; *st = S; }
}

// the winner (column -> P.xf, index -> f); returns 1 when _select raised or nothing is selectable
template <int ALG>
__device__ __forceinline__ int fin_pick(const SnnlsDev& P, SnnlsState& S, double* red, long long& f) {
  int fail = S.select_fail;                          // _select raised
  f = -1;
  if (!fail) {
    if (ALG != BC_ALG_OMP && P.fuse_winner) dev_pick_blocks(P, S);
    else dev_pick<ALG>(P, S, red);
    if (!S.sel_valid) fail = 1;
    f = S.sel_f;
  }
  return fail;
}

// what a revert puts back (snnls.py:46-47)
struct FinSaved {
  long long nnz0, npos0;
  double err0, xwsq0;
};
__device__ __forceinline__ FinSaved fin_save(const SnnlsState& S) { return {S.nnz, S.npos, S.err_cur, S.xw_sq}; }

// ... and the vectors: xw -> xw_prev, and val -> prev_val where the kernel reweights the global list in place (LIST).  (No
// barrier needed: each thread later rewrites exactly the val[j] it saved, and xw is only overwritten behind dev_xw_err's barriers)
template <bool LIST>
__device__ __forceinline__ void fin_keep_prev(const SnnlsDev& P, long long nnz0) {
  if (LIST)
    for (long long j = threadIdx.x; j < nnz0; j += blockDim.x) P.prev_val[j] = P.val[j];
  for (int k = threadIdx.x; k < P.s; k += blockDim.x) P.xw_prev[k] = P.xw[k];
}

// the monotone-error guard (snnls.py:58-62) behind a reweight: returns 1 after reverting a step that raised the error
template <bool LIST>
__device__ __forceinline__ int fin_guard(const SnnlsDev& P, SnnlsState& S, const FinSaved& sv, bool guard) {
  int fail = 0;
  if (guard) {
    if (S.err_cur > sv.err0) {                       // snnls.py:58-61
      if (LIST)
        for (long long j = threadIdx.x; j < sv.nnz0; j += blockDim.x) P.val[j] = P.prev_val[j];
      for (int k = threadIdx.x; k < P.s; k += blockDim.x) P.xw[k] = P.xw_prev[k];
      __syncthreads();
      if (threadIdx.x == 0) {
        S.nnz = sv.nnz0;
        S.npos = sv.npos0;
        S.err_cur = sv.err0;
        S.xw_sq = sv.xwsq0;
      }
      fail = 1;
    } else if (threadIdx.x == 0) {
      S.retried = 0;                                 // snnls.py:62
    }
    __syncthreads();
  }
  return fail;
}

// retry-once-then-stop (snnls.py:63-72), the trace entry, the next sweep vectors, and xw back to global memory where it
// lived in LDS
template <int ALG>
__device__ __forceinline__ void fin_close(const SnnlsDev& P, SnnlsState& S, double* red, int fail, long long f, double* xw_out) {
  __shared__ int sh_fail;
  if (threadIdx.x == 0) {
    if (fail) {
      if (S.retried) S.reached_limit = 1;
      else S.retried = 1;
    }
    sh_fail = fail;
  }
  __syncthreads();
  FSTAMP(7);
  dev_trace(P, S, f, sh_fail);
  __syncthreads();
  dev_prep<ALG>(P, S, red);
  FSTAMP(8);
  if (xw_out)
    for (int k = threadIdx.x; k < P.s; k += blockDim.x) xw_out[k] = P.xw[k];
}

// the picked column lived in LDS: a later step-wise reweight / refit must fetch it again
__device__ __forceinline__ void fin_store_state(SnnlsState& S, SnnlsState* st) {
  if (threadIdx.x == 0) {
    S.sel_valid = 0;
    *st = S;
  }
}
