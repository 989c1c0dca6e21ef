// Sparse-NNLS solver state on the device: the guarded greedy loop of
// bayesiancoresets/snnls/snnls.py:31-79 run WITHOUT a host round trip per iteration,
// plus the step-wise (_select / _reweight) protocol of snnls.py:102-106.
//
// Per iteration:   K3 sweep (bc_sweep.hip)  ->  k_local_winner  -> [host all-gather when
// world > 1]  ->  k_step_finish (single block): global winner, closed-form reweight
// (giga.py:40-64 / frankwolfe.py:19-40), monotone-error guard with revert, the
// retry-once-then-stop state machine, and the S-vector prep for the next sweep
// (giga.py:20-30 / frankwolfe.py:16).  All replicated state (sparse w, selected
// columns, xw = A.w) lives in device memory; every rank runs the identical finish
// kernel on identical gathered records, so ranks stay bit-identical.
//
// This unit holds the kernels and the host side.  What the solver is (SnnlsState, SnnlsDev, struct bc_snnls) is
// bc_snnls_state.h; the device functions the kernels are made of are bc_snnls_dev.h; the pre-filter's diagnostic
// seam (test aids) is a unit of its own, bc_snnls_diag.hip, and nothing here knows of it.
#ifdef BC_FIN_STAMPS          // diagnostic build: phase time stamps of the single-block step kernels
#include <hip/hip_runtime.h>
__device__ unsigned long long g_fin_stamps[64];
#define FSTAMP(i) do { if (threadIdx.x == 0) g_fin_stamps[i] = __builtin_amdgcn_s_memtime(); } while (0)
#define FDBG(i, v) do { if (threadIdx.x == 0) g_fin_stamps[i] = (unsigned long long)(v); } while (0)
extern "C" int bc_debug_fin_stamps(unsigned long long* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fin_stamps), sizeof(g_fin_stamps)) == hipSuccess ? 0 : -1;
}
#endif
#include "bc_snnls_state.h"
#include "bc_snnls_dev.h"          // takes FSTAMP from the block above, as bc_rescore_dev.h does
#include "../../include/beta_cores_nnls.h"
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <algorithm>

// ------------------------------------------------------------------ kernels (grid = 1 block)
template <int ALG>
__global__ __launch_bounds__(BC_FIN_THREADS) void k_prep(SnnlsDev P, int reset_retry) {
  __shared__ SnnlsState S;
  __shared__ double red[64];
  if (threadIdx.x == 0) {
    S = *P.st;
    if (reset_retry) S.retried = 0;
  }
  __syncthreads();
  dev_prep<ALG>(P, S, red);
  if (threadIdx.x == 0) *P.st = S;
}

// one guarded greedy iteration, snnls.py:41-74.  The S-vectors (b, bn, xw, xf, previous xw) live in
// LDS for the duration of the kernel (lds_vecs != 0): one parallel load at the start instead of a
// global-memory round trip per use.
// ALG == BC_ALG_OMP (orthopursuit.py:17-41): the closed-form step in the middle is replaced by "give the picked column a slot,
// extend the Gram state, NNLS refit", whose workspace sits in front of the vectors in dynamic LDS; the winner comes from the
// gathered candidate record(s).
template <int ALG>
__global__ __launch_bounds__(BC_FIN_THREADS) void k_step_finish(SnnlsDev P0, int lds_vecs) {
  extern __shared__ double fin_lds[];
  __shared__ SnnlsState S;
  __shared__ double red[64];
  constexpr bool OMP = ALG == BC_ALG_OMP;
  if (threadIdx.x == 0) S = *P0.st;
  SnnlsDev P = P0;
  if (lds_vecs) fin_stage_vecs(P, P0, fin_lds + (OMP ? BC_NNLS_WS_DOUBLES : 0));
  __syncthreads();
  if (fin_idle(S)) return;
  if ((OMP || !P.fuse_winner) && !S.select_fail && dev_records_overflow(P0.cand_all, P.world, P.rec_len)) {
    fin_refuse_overflow(S, P0.st);
    return;
  }
  const bool guard = S.npos > 0;                     // snnls.py:44-45 (check_error_monotone is True for GIGA/FW/OMP)
  long long f;
  int fail = fin_pick<ALG>(P, S, red, f);
  if (!fail) {
    FinSaved sv;
    if constexpr (OMP) {
      sv = fin_save(S);
      const long long limit = P.cap < BC_NNLS_MAXP ? P.cap : BC_NNLS_MAXP;
      int fresh = 0;
      const long long at = sv.nnz0 <= BC_NNLS_MAXP ? dev_omp_place(P, S, limit, &fresh) : -1;
      if (at < 0) {                                  // the host's bound on the list length was wrong: refuse
        if (threadIdx.x == 0) { S.overflow = 1; *P0.st = S; }
        return;
      }
      fin_keep_prev<true>(P, sv.nnz0);
      dev_gram_update(P, sv.nnz0, S.nnz, at, fresh);
      fail = bc_nnls_solve(P.gram, P.gram_c, (int)S.nnz, P.val, (int)at, 0, P.bnorm, bc_nnls_ws(fin_lds), P.nnls_stats);
      if (fail) {                                    // like a NumericalPrecisionError out of _reweight: w was not touched
        if (threadIdx.x == 0) S.nnz = sv.nnz0;
        __syncthreads();
      }
    } else {
      double alpha = 0., beta = 0.;
      fail = dev_step_sizes<ALG>(P, S, red, alpha, beta);
      if (!fail) {
        sv = fin_save(S);
        fin_keep_prev<true>(P, sv.nnz0);
        dev_apply(P, S, alpha, beta);
      }
    }
    if (!fail) {
      dev_xw_err(P, S, red);
      fail = fin_guard<true>(P, S, sv, guard);
    }
  }
  fin_close<ALG>(P, S, red, fail, f, lds_vecs ? P0.xw : nullptr);
  fin_store_state(S, P0.st);
}

// The same step with ONE round of global loads up front: state, S-vectors, all candidate records (with their
// columns), the weight list (val, idx) and each thread's first 16 list columns are requested before anything is
// consumed, then the step runs out of LDS / registers and the results are written back at the end.  The plain
// kernel above pays a memory latency per phase (state -> records -> column -> list -> columns ...), ~7 dependent
// round trips; both produce the same bits (same device functions, same orders).  Used when the list and the records
// fit the LDS budget (nnz_hint + 1 <= BC_PF_MAXNNZ, world * rec_len <= BC_PF_MAXREC, S <= blockDim).
// RS: the pre-filter's rescoring stage (bc_rescore_dev.h) runs INSIDE this launch, between the up-front loads and
// the step: its record goes straight into LDS (single rank, no exchange).  One launch per greedy step besides the
// sweep instead of two (k_rescore 11.7 us + k_step_finish_pf 12.6 us in round 1).
// RS = 2: the branch-and-bound sweep (bc_prefilter_bb.h) already rescored its candidates: the "rescoring stage" is the argmax
// over its per-block records (bc_bb_pick), one round of loads that travels with the other up-front loads.
template <int ALG, int RS>
__global__ __launch_bounds__(BC_FIN_THREADS) void k_step_finish_pf(SnnlsDev P0, int nnz_hint, RescoreArgs ra, long long n_rows) {
  extern __shared__ double pf_lds[];
  __shared__ SnnlsState S;
  __shared__ double red[64];
  const int s = P0.s;
  const int nrec = RS ? P0.rec_len : (P0.fuse_winner ? 0 : P0.world * P0.rec_len);
  FSTAMP(0);
  double* l_b = pf_lds;
  double* l_bn = l_b + s;
  double* l_xw = l_bn + s;
  double* l_xf = l_xw + s;
  double* l_xwp = l_xf + s;
  double* l_rec = l_xwp + s;
  double* l_val = l_rec + nrec;
  long long* l_idx = reinterpret_cast<long long*>(l_val + (nnz_hint + 1));
  // ---- one round of loads.  Everything is requested into REGISTERS first and parked in LDS afterwards: written as
  // "load, store to LDS" group by group the compiler waited for each group before it issued the next -- six dependent
  // round trips (state, vectors, list, bounds, ...) instead of one: 6.6k of the step's 45k cycles (tools/fin_stamps.py).
  // Indices are clamped instead of branched around, so that nothing separates the requests.
  const int k0 = (int)threadIdx.x < s ? (int)threadIdx.x : 0;                 // (s <= blockDim: one element per thread)
  const double r_b = P0.b[k0], r_bn = P0.bn[k0], r_xw = P0.xw[k0];
  double r_rec[BC_PF_MAXREC / BC_FIN_THREADS];
  if (!RS) {
#pragma unroll
    for (int u = 0; u < BC_PF_MAXREC / BC_FIN_THREADS; ++u) {
      const int i = threadIdx.x + u * BC_FIN_THREADS;
      r_rec[u] = (nrec > 0) ? P0.cand_all[i < nrec ? i : 0] : 0.;
    }
  }
  double r_val[BC_PF_MAXNNZ / BC_FIN_THREADS];
  long long r_idx[BC_PF_MAXNNZ / BC_FIN_THREADS];
#pragma unroll
  for (int u = 0; u < BC_PF_MAXNNZ / BC_FIN_THREADS; ++u) {
    const int j = threadIdx.x + u * BC_FIN_THREADS;
    const int jc = j < nnz_hint ? j : 0;                                      // (the list slab always holds slot 0)
    r_val[u] = P0.val[jc];
    r_idx[u] = P0.idx[jc];
  }
  RescorePre pre;
  BbPre bbpre;
  if (RS == 1) pre = bc_rescore_prefetch(ra);        // the sweep blocks' bounds travel with the other up-front loads
  if (RS == 2) bbpre = bc_bb_prefetch(ra.bb);        // ... or their records
  const int G = blockDim.x / s;
  const int g = threadIdx.x / s, kk = threadIdx.x - g * s;
  double c16[BC_PF_NC];
#pragma unroll
  for (int u = 0; u < BC_PF_NC; ++u) {
    long long j = (g < G ? g : 0) + (long long)u * G;
    j = j < nnz_hint ? j : (nnz_hint > 0 ? nnz_hint - 1 : 0);      // clamped: always a valid slot, unused when past the list
    c16[u] = P0.cols[(size_t)j * s + (g < G ? kk : 0)];
  }
  FSTAMP(25);
  // ---- park
  if (threadIdx.x == 0) S = *P0.st;                  // (requested behind the others: it arrives with them)
  if ((int)threadIdx.x < s) {
    l_b[threadIdx.x] = r_b;
    l_bn[threadIdx.x] = r_bn;
    l_xw[threadIdx.x] = r_xw;
  }
  if (!RS) {
#pragma unroll
    for (int u = 0; u < BC_PF_MAXREC / BC_FIN_THREADS; ++u) {
      const int i = threadIdx.x + u * BC_FIN_THREADS;
      if (i < nrec) l_rec[i] = r_rec[u];
    }
  }
#pragma unroll
  for (int u = 0; u < BC_PF_MAXNNZ / BC_FIN_THREADS; ++u) {
    const int j = threadIdx.x + u * BC_FIN_THREADS;
    if (j < nnz_hint) {
      l_val[j] = r_val[u];
      l_idx[j] = r_idx[u];
    }
  }
  __syncthreads();
  SnnlsDev P = P0;
  P.b = l_b;
  P.bn = l_bn;
  P.xw = l_xw;
  P.xf = l_xf;
  P.xw_prev = l_xwp;
  P.val = l_val;
  P.idx = l_idx;
  if (nrec) P.cand_all = l_rec;
  if (RS) { P.world = 1; P.fuse_winner = 0; }
  // one record, already in LDS (the rescoring stage of this launch wrote it): its column IS the picked column -- dev_pick
  // then has nothing to copy (and no barrier to pass)
  if (RS && ALG != BC_ALG_OMP) P.xf = l_rec + BC_REC_HDR;
  FSTAMP(1);
  if (fin_idle(S)) return;
  bool pf_ovf = false;
  if (RS) {
    if (RS == 2) {
      if (!S.skip) pf_ovf = bc_bb_pick(ra.bb, bbpre, s, ra.ctrl, l_rec) != 0;
    } else if (!S.skip) {
      pf_ovf = bc_rescore_block<(ALG == BC_ALG_GIGA) ? 0 : 1>(ra, n_rows, l_rec, pre) != 0;
    }
    __syncthreads();
    FSTAMP(2);
  } else if (!P.fuse_winner && !S.select_fail) {
    pf_ovf = dev_records_overflow(l_rec, P.world, P.rec_len);
  }
  if (pf_ovf) {
    fin_refuse_overflow(S, P0.st);
    return;
  }
  if (S.nnz > nnz_hint) {                            // the host's bound on the list length was wrong: refuse
    if (threadIdx.x == 0) { S.overflow = 1; *P0.st = S; }
    return;
  }
  const bool guard = S.npos > 0;                     // snnls.py:44-45
  bool wrote = false;
  const FinSaved sv = fin_save(S);
  long long f;
  int fail = fin_pick<ALG>(P, S, red, f);
  FSTAMP(3);
  if (!fail) {
    double alpha = 0., beta = 0.;
    fail = dev_step_sizes<ALG>(P, S, red, alpha, beta);
    FSTAMP(4);
    if (!fail) {
      fin_keep_prev<false>(P, sv.nnz0);
      dev_apply(P, S, alpha, beta);                  // on the LDS copy of (val, idx); a new column goes to global cols
      FSTAMP(5);
      const long long at_new = (S.nnz == sv.nnz0 + 1) ? sv.nnz0 : -1;
      dev_xw_err_t<true>(P, S, red, c16, at_new);
      FSTAMP(6);
      fail = fin_guard<false>(P, S, sv, guard);      // nothing was written back yet: a revert just drops the LDS list
      wrote = !fail;
    }
  }
  fin_close<ALG>(P, S, red, fail, f, P0.xw);
  // ---- write back
  if (wrote) {
    const long long nnz = S.nnz;
    for (long long j = threadIdx.x; j < nnz; j += blockDim.x) P0.val[j] = l_val[j];
    if (nnz == sv.nnz0 + 1 && threadIdx.x == 0) P0.idx[sv.nnz0] = l_idx[sv.nnz0];
  }
  fin_store_state(S, P0.st);
  FSTAMP(9);
}

template <int ALG>
__global__ __launch_bounds__(BC_FIN_THREADS) void k_pick(SnnlsDev P) {
  __shared__ SnnlsState S;
  __shared__ double red[64];
  if (threadIdx.x == 0) S = *P.st;
  __syncthreads();
  if (!S.select_fail && dev_records_overflow(P.cand_all, P.world, P.rec_len)) {
    if (threadIdx.x == 0) { S.last_status = BC_RETRY_EXACT; *P.st = S; }     // some rank's pre-filter overflowed
    return;
  }
  if (!S.select_fail) dev_pick<ALG>(P, S, red);
  if (threadIdx.x == 0) {
    S.last_status = S.select_fail ? BC_NUMERICAL_PRECISION : (S.sel_valid ? BC_OK : BC_INVALID_ARGUMENT);
    *P.st = S;
  }
}

// step-wise _reweight(f): no guard here, the host loop owns it (snnls.py:53-61)
template <int ALG>
__global__ __launch_bounds__(BC_FIN_THREADS) void k_reweight(SnnlsDev P, long long f) {
  __shared__ SnnlsState S;
  __shared__ double red[64];
  if (threadIdx.x == 0) S = *P.st;
  __syncthreads();
  if (!dev_fetch_column(P, S, f)) {
    if (threadIdx.x == 0) { S.last_status = BC_INVALID_ARGUMENT; *P.st = S; }
    return;
  }
  double alpha = 0., beta = 0.;
  const int fail = dev_step_sizes<ALG>(P, S, red, alpha, beta);
  if (!fail) {
    dev_apply(P, S, alpha, beta);
    dev_xw_err(P, S, red);
  }
  if (threadIdx.x == 0) {
    S.last_status = fail ? BC_NUMERICAL_PRECISION : BC_OK;
    *P.st = S;
  }
}

// rebuild the sparse list from (idx, val[, cols]); columns not supplied are looked up in the
// old list, then in the last candidate records, then in the local shard.
__global__ __launch_bounds__(BC_FIN_THREADS) void k_set_weights(SnnlsDev P, long long n, const long long* __restrict__ nidx,
                                                    const double* __restrict__ nval, const double* __restrict__ ncols,
                                                    long long* idx2, double* val2, double* cols2, double* colnorm2) {
  __shared__ SnnlsState S;
  __shared__ double red[64];
  __shared__ int kind, hit;
  __shared__ long long where;
  const int s = P.s;
  if (threadIdx.x == 0) { S = *P.st; S.last_status = BC_OK; }
  __syncthreads();
  for (long long j = 0; j < n; ++j) {
    const long long f = nidx[j];
    if (threadIdx.x == 0) { kind = ncols ? 1 : 0; where = -1; hit = INT_MAX; }
    __syncthreads();
    if (!ncols) {
      for (long long q = threadIdx.x; q < S.nnz; q += blockDim.x)
        if (P.idx[q] == f) atomicMin(&hit, (int)q);
      __syncthreads();
      if (threadIdx.x == 0) {
        int kd = 0;
        long long w = -1;
        if (hit != INT_MAX) { kd = 2; w = hit; }
        if (!kd)
          for (int r = 0; r < P.world; ++r) {
            const double* rec = P.cand_all + (size_t)r * P.rec_len;
            if (rec[3] != 0.0 && reinterpret_cast<const long long*>(rec)[1] == f) { kd = 3; w = r; break; }
          }
        if (!kd && f >= P.row_offset && f < P.row_offset + P.n_rows) { kd = 4; w = f - P.row_offset; }
        if (!kd) S.last_status = BC_INVALID_ARGUMENT;
        kind = kd;
        where = w;
      }
    }
    __syncthreads();
    const int kd = kind;
    const long long w = where;
    for (int k = threadIdx.x; k < s; k += blockDim.x) {
      double v = 0.0;
      if (kd == 1) v = ncols[(size_t)j * s + k];
      else if (kd == 2) v = P.cols[(size_t)w * s + k];
      else if (kd == 3) v = P.cand_all[(size_t)w * P.rec_len + BC_REC_HDR + k];
      else if (kd == 4) v = P.tiles[bc_tile_off(w, k, s)];
      cols2[(size_t)j * s + k] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      double nrm = 0.0;
      for (int k = 0; k < s; ++k) nrm = fma(cols2[(size_t)j * s + k], cols2[(size_t)j * s + k], nrm);
      colnorm2[j] = sqrt(nrm);
      idx2[j] = f;
      val2[j] = nval[j];
    }
    __syncthreads();
  }
  // from here on the new buffers are the list
  SnnlsDev Q = P;
  Q.idx = idx2;
  Q.val = val2;
  Q.cols = cols2;
  Q.colnorm = colnorm2;
  if (threadIdx.x == 0) { S.nnz = n; S.sel_valid = 0; dev_gram_touch(P, 0); }
  __syncthreads();
  dev_xw_err(Q, S, red);
  if (threadIdx.x == 0) *P.st = S;
}

__global__ __launch_bounds__(BC_FIN_THREADS) void k_reset(SnnlsDev P) {
  __shared__ double red[64];
  __shared__ SnnlsState S;
  if (threadIdx.x == 0) {
    memset(&S, 0, sizeof(S));
    S.sel_f = -1;
    dev_gram_touch(P, 0);
  }
  __syncthreads();
  dev_xw_err(P, S, red);   // nnz = 0 -> xw = 0, err = ||b||
  if (threadIdx.x == 0) *P.st = S;
}

// The same refit behind a single launch, for the step-wise protocol and optimize():
//   mode 0  orthopursuit.py:37-41 for column f (no guard here, the host loop owns it)
//   mode 1  NNLS over every cached column of the list, zero-weight slots included
//   mode 2  snnls.py:82-97: refit the entries with a positive weight; keep the result unless the error grew beyond
//           (1 + tol) times the previous one (or the refit failed), else restore the weights and set reached_limit
__global__ __launch_bounds__(BC_FIN_THREADS) void k_refit(SnnlsDev P, long long f, int mode) {
  extern __shared__ double refit_lds[];
  __shared__ SnnlsState S;
  __shared__ double red[64];
  if (threadIdx.x == 0) S = *P.st;
  __syncthreads();
  const long long nnz0 = S.nnz;
  const double err0 = S.err_cur;
  const long long limit = P.cap < BC_NNLS_MAXP ? P.cap : BC_NNLS_MAXP;
  // refusals come first: nothing but last_status has changed when one is reported
  if (nnz0 > BC_NNLS_MAXP || (mode == 0 && !dev_omp_room(P, S, f, limit))) {
    if (threadIdx.x == 0) { P.st->last_status = BC_ST_LIST_LIMIT; }
    return;
  }
  if (mode == 0 && !dev_fetch_column(P, S, f)) {
    if (threadIdx.x == 0) { P.st->last_status = BC_INVALID_ARGUMENT; }
    return;
  }
  int fresh = 0;
  long long at = -1;
  if (mode == 0) {
    at = dev_omp_place(P, S, limit, &fresh);
    if (at < 0) {                    // (dev_omp_room said otherwise: cannot happen)
      if (threadIdx.x == 0) { P.st->last_status = BC_ST_LIST_LIMIT; }
      return;
    }
  }
  for (long long j = threadIdx.x; j < nnz0; j += blockDim.x) P.prev_val[j] = P.val[j];
  dev_gram_update(P, nnz0, S.nnz, at, fresh);
  const int fail = bc_nnls_solve(P.gram, P.gram_c, (int)S.nnz, P.val, (int)at, mode == 1, P.bnorm, bc_nnls_ws(refit_lds), P.nnls_stats);
  int status = fail ? BC_NUMERICAL_PRECISION : BC_OK;
  if (fail) {
    if (threadIdx.x == 0) S.nnz = nnz0;
    __syncthreads();
  } else {
    dev_xw_err(P, S, red);
  }
  if (mode == 2) {
    if (!fail && S.err_cur > err0 * (1. + P.tol)) {
      for (long long j = threadIdx.x; j < nnz0; j += blockDim.x) P.val[j] = P.prev_val[j];
      __syncthreads();
      dev_xw_err(P, S, red);
      status = BC_NUMERICAL_PRECISION;
    }
    if (status != BC_OK && threadIdx.x == 0) {
      S.reached_limit = 1;
      S.skip = 1;
    }
  }
  if (threadIdx.x == 0) {
    S.last_status = status;
    *P.st = S;
  }
}

__global__ void k_clear_pf_overflow(SnnlsState* st) {
  st->pf_overflow = 0;
  st->skip = st->select_fail | st->reached_limit;
}

__global__ void k_set_flag(SnnlsState* st, int reached) {
  st->reached_limit = reached;
  st->skip = st->select_fail | reached;
}

// ------------------------------------------------------------------ host side: handle lifetime and buffers
static void free_lists(bc_snnls* h) {
  if (h->list_slab) (void)hipFree(h->list_slab);
  h->list_slab = nullptr;
  h->d.idx = h->idx2 = nullptr;
  h->d.val = h->val2 = h->d.prev_val = nullptr;
  h->d.cols = h->cols2 = nullptr;
  h->d.colnorm = h->colnorm2 = nullptr;
}

static int ensure_capacity(bc_snnls* h, long long need) {
  if (need <= h->d.cap) return BC_OK;
  bc_ctx* ctx = h->ctx;
  long long ncap = std::max<long long>(need, std::max<long long>(256, h->d.cap * 2));
  const int s = h->d.s;
  // one slab: [idx | val | prev_val | colnorm | cols] of the live set first (what the step kernel reads), then the
  // second set (bc_snnls_set_weights rebuilds into it and swaps)
  const size_t n8 = (size_t)ncap * 8, ncols = (size_t)ncap * s * 8;
  const size_t total = 7 * n8 + 2 * ncols;
  char* slab = nullptr;
  hipError_t e = hipMalloc((void**)&slab, total);
  if (e != hipSuccess) return bc_hip_fail(e, "hipMalloc(active list)", __FILE__, __LINE__);
  long long* idx = (long long*)slab;
  double* val = (double*)(slab + n8);
  double* pv = (double*)(slab + 2 * n8);
  double* cn = (double*)(slab + 3 * n8);
  double* cols = (double*)(slab + 4 * n8);
  long long* idx2 = (long long*)(slab + 4 * n8 + ncols);
  double* val2 = (double*)(slab + 5 * n8 + ncols);
  double* cn2 = (double*)(slab + 6 * n8 + ncols);
  double* cols2 = (double*)(slab + 7 * n8 + ncols);
  if (h->d.cap > 0) {
    e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = hipMemcpy(idx, h->d.idx, h->d.cap * sizeof(long long), hipMemcpyDeviceToDevice);
    if (e == hipSuccess) e = hipMemcpy(val, h->d.val, h->d.cap * sizeof(double), hipMemcpyDeviceToDevice);
    if (e == hipSuccess) e = hipMemcpy(cn, h->d.colnorm, h->d.cap * sizeof(double), hipMemcpyDeviceToDevice);
    if (e == hipSuccess) e = hipMemcpy(cols, h->d.cols, (size_t)h->d.cap * s * sizeof(double), hipMemcpyDeviceToDevice);
    if (e != hipSuccess) { (void)hipFree(slab); return bc_hip_fail(e, "hipMemcpy(active list)", __FILE__, __LINE__); }   // the old list stays
  }
  free_lists(h);
  h->list_slab = slab;
  h->d.idx = idx; h->idx2 = idx2;
  h->d.val = val; h->d.prev_val = pv; h->val2 = val2;
  h->d.colnorm = cn; h->colnorm2 = cn2;
  h->d.cols = cols; h->cols2 = cols2;
  h->d.cap = ncap;
  return BC_OK;
}

static int ensure_trace(bc_snnls* h, long long need) {
  if (need <= h->d.tr_cap) return BC_OK;
  long long ncap = std::max<long long>(need, std::max<long long>(1024, h->d.tr_cap * 2));
  long long* f = nullptr;
  int* st = nullptr;
  double* er = nullptr;
  hipError_t e = hipMalloc((void**)&f, ncap * sizeof(long long));
  if (e == hipSuccess) e = hipMalloc((void**)&st, ncap * sizeof(int));
  if (e == hipSuccess) e = hipMalloc((void**)&er, ncap * sizeof(double));
  if (e == hipSuccess && h->d.tr_cap > 0) {
    e = hipStreamSynchronize(h->ctx->stream);
    if (e == hipSuccess) e = hipMemcpy(f, h->d.tr_f, h->d.tr_cap * sizeof(long long), hipMemcpyDeviceToDevice);
    if (e == hipSuccess) e = hipMemcpy(st, h->d.tr_status, h->d.tr_cap * sizeof(int), hipMemcpyDeviceToDevice);
    if (e == hipSuccess) e = hipMemcpy(er, h->d.tr_err, h->d.tr_cap * sizeof(double), hipMemcpyDeviceToDevice);
  }
  if (e != hipSuccess) {                 // the old trace stays
    void* fresh[] = {f, st, er};
    for (void* p : fresh)
      if (p) (void)hipFree(p);
    return bc_hip_fail(e, "hipMalloc / hipMemcpy(trace)", __FILE__, __LINE__);
  }
  if (h->d.tr_cap > 0) {
    (void)hipFree(h->d.tr_f); (void)hipFree(h->d.tr_status); (void)hipFree(h->d.tr_err);
  }
  h->d.tr_f = f; h->d.tr_status = st; h->d.tr_err = er; h->d.tr_cap = ncap;
  return BC_OK;
}

extern "C" int bc_snnls_destroy(bc_snnls* h) {
  if (!h) return BC_OK;
  (void)hipStreamSynchronize(h->ctx->stream);
  bc_pref_destroy(h->pref);
  h->pref = nullptr;
  free_lists(h);
  void* ptrs[] = {h->state_slab, h->cand_all_owned, h->d.tr_f, h->d.tr_status, h->d.tr_err, h->nnls_slab};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  delete h;
  return BC_OK;
}

// ------------------------------------------------------------------ what the environment asks of the pre-filter (read by bc_snnls_create, below)
// Two-level pre-filter (bc_prefilter_i4.h) wanted?  BC_PREFILTER=4 forces it, =8 keeps the one-level int8 sweep; by default it
// is used from BC_TWO_LEVEL_MIN_ROWS rows: measured per step at S = 100 (tools/two_level_probe.py, us, two-level / one-level):
// 1.25M rows 43.4 / 42.5, 2.5M 53.6 / 62, 5M 72.5 / 102, 10M 114 / 177.  S <= 256.
#define BC_TWO_LEVEL_MIN_ROWS 2000000LL
static bool bc_want_two_level(int preq, long long n_rows, int s) {
  if (s > 256 || n_rows <= 0) return false;
  if (preq == 4) return true;
  if (preq >= 0 && preq != 1) return false;          // an explicit BC_PREFILTER precision other than 4
  const char* tenv = getenv("BC_TWO_LEVEL_MIN_ROWS");
  const long long min_rows = tenv ? atoll(tenv) : BC_TWO_LEVEL_MIN_ROWS;
  return n_rows >= min_rows;
}

// What the environment asks of a new solver's pre-filter, read once per bc_snnls_create (tests set it per solver).
// BC_PREFILTER = 0 (off) / 1 (on, default precision) / 8 / 16 / 32 (on, that storage precision) / 4 (the int8 mirror behind a
// 4-bit first level); unset: on from BC_PREF_MIN_ROWS rows, where it is worth its extra launches (measured break-even ~131k
// rows at S = 100 with the int8 mirror, profiles/r01_notes.md).  BC_I8_QV=0: sweeps quantise in their own prologue (A/B, tests).
#define BC_PREF_MIN_ROWS 163840
struct PrefWish {
  bool want;        // a pre-filter is created ...
  int prec;         // ... with this precision asked of bc_pref_create (4: the two-level form)
  bool keep_qv;     // the step kernels keep v's int8 digit record current from the start (the int8 sweep reads v as digits) ...
  bool keep_qv4;    // ... and its 4-bit record, which only the two-level form reads
};
static PrefWish pref_wish(long long n_rows, int s) {
  const char* env = getenv("BC_PREFILTER");
  const int req = env ? atoi(env) : -1;
  const char* qenv = getenv("BC_I8_QV");
  const int prec = (req == 8 || req == 16 || req == 32) ? req : BC_PREF_DEFAULT_PREC;
  PrefWish w;
  w.want = (env ? req != 0 : n_rows >= BC_PREF_MIN_ROWS) && n_rows > 0;
  w.keep_qv = w.want && prec == 8 && (s + 3) / 4 <= BC_LAY_IMAXG - BC_LAY_IU && !(qenv && atoi(qenv) == 0);
  w.keep_qv4 = w.keep_qv && bc_want_two_level(req, n_rows, s);
  w.prec = w.keep_qv4 ? 4 : prec;
  return w;
}

extern "C" int bc_snnls_create(bc_ctx* ctx, bc_phi* phi, const double* b, int alg, double norm_sum,
                               int allow_zero_rows, bc_snnls** out) {
  if (!ctx || !phi || !b || !out || alg < 0 || alg > 2) { bc_set_error("bc_snnls_create: bad argument"); return BC_INVALID_ARGUMENT; }
  if (phi->ctx != ctx) { bc_set_error("bc_snnls_create: phi belongs to another context"); return BC_INVALID_ARGUMENT; }
  int64_t zr = 0;
  int rc = bc_phi_norm_stats(phi, &zr, nullptr);
  if (rc) return rc;
  if (zr > 0 && !allow_zero_rows) {
    bc_set_error("A must not have any 0 columns (%lld zero-norm rows)", (long long)zr);   // giga.py:11-12
    return BC_INVALID_ARGUMENT;
  }
  const int s = phi->s;
  double bnorm = 0.0;
  for (int k = 0; k < s; ++k) bnorm += b[k] * b[k];
  bnorm = sqrt(bnorm);
  if (alg == BC_ALG_GIGA && bnorm == 0.) {
    bc_set_error("norm of b must be > 0");   // giga.py:16-17
    return BC_NUMERICAL_PRECISION;
  }
  bc_snnls* h = new bc_snnls();
  h->ctx = ctx;
  h->phi = phi;
  h->alg = alg;
  memset(&h->d, 0, sizeof(h->d));
  SnnlsDev& d = h->d;
  d.s = s;
  d.world = 1;
  d.rec_len = s + BC_REC_HDR;
  d.bnorm = bnorm;
  d.tol = 1e-12;
  d.norm_sum = norm_sum;
  d.tiles = phi->tiles;
  d.norms = phi->norms;
  d.n_rows = phi->n_rows;
  d.row_offset = phi->row_offset;
  const PrefWish pw = pref_wish(phi->n_rows, s);
  {
    // one slab (see bc_snnls::state_slab): st | b | bn | xw | xw_prev | xf | send record | v (zero tail: the fp16
    // sweep reads whole plane batches), every piece 256-byte aligned
    const size_t o_st = 0, o_b = bc_up256(sizeof(SnnlsState)), o_bn = o_b + bc_up256(s * 8), o_xw = o_bn + bc_up256(s * 8), o_xwp = o_xw + bc_up256(s * 8),
                 o_xf = o_xwp + bc_up256(s * 8), o_rec = o_xf + bc_up256(s * 8), o_v = o_rec + bc_up256(d.rec_len * 8),
                 o_qv = o_v + bc_up256(2 * (s + BC_V_PAD) * 8), o_qv4 = o_qv + bc_up256((size_t)BC_I8Q_INTS(bc_lay_i8_sp4(s)) * sizeof(int)),
                 total = o_qv4 + bc_up256((size_t)BC_I4Q_INTS(bc_lay_i4_sp8(s, bc_lay_i4_batch(s))) * sizeof(int));
    char* slab = nullptr;
    hipError_t e0 = hipMalloc((void**)&slab, total);
    if (e0 == hipSuccess) e0 = hipMemsetAsync(slab, 0, total, ctx->stream);
    if (e0 != hipSuccess) { if (slab) (void)hipFree(slab); bc_snnls_destroy(h); return bc_hip_fail(e0, "hipMalloc(snnls)", __FILE__, __LINE__); }
    h->state_slab = slab;
    d.st = (SnnlsState*)(slab + o_st);
    d.b = (double*)(slab + o_b);
    d.bn = (double*)(slab + o_bn);
    d.xw = (double*)(slab + o_xw);
    d.xw_prev = (double*)(slab + o_xwp);
    d.xf = (double*)(slab + o_xf);
    h->cand_send = (double*)(slab + o_rec);
    d.v = (double*)(slab + o_v);
    const char* fenv = getenv("BC_FINISH_NOPF");         // finish-kernel forms ruled out for this solver (tests, A/B)
    h->no_pf = fenv && atoi(fenv) != 0;
    fenv = getenv("BC_FINISH_NOFUSE");
    h->no_fuse = fenv && atoi(fenv) != 0;
    // the int8 pre-filter (created below, after k_reset has produced the first sweep vector) reads v as digits: the step
    // kernels keep that record current from the start when such a pre-filter is going to exist
    d.sp4 = bc_lay_i8_sp4(s);
    d.qv = pw.keep_qv ? (int*)(slab + o_qv) : nullptr;
    d.sp8 = bc_lay_i4_sp8(s, bc_lay_i4_batch(s));
    d.qv4 = pw.keep_qv4 ? (int*)(slab + o_qv4) : nullptr;
  }
  hipError_t e = hipSuccess;
  d.cand_all = h->cand_send;
  rc = ensure_capacity(h, 256);
  if (!rc) rc = ensure_trace(h, 1024);
  if (rc) { bc_snnls_destroy(h); return rc; }
  // bn = b / ||b|| element-wise like giga.py:18
  std::vector<double> tmp(2 * s);
  for (int k = 0; k < s; ++k) {
    tmp[k] = b[k];
    tmp[s + k] = bnorm != 0. ? b[k] / bnorm : 0.;
  }
  e = hipMemcpyAsync(d.b, tmp.data(), s * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d.bn, tmp.data() + s, s * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(h->cand_send, 0, d.rec_len * sizeof(double), ctx->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_reset, dim3(1), dim3(BC_FIN_THREADS), 0, ctx->stream, d);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) { bc_snnls_destroy(h); return bc_hip_fail(e, "snnls init", __FILE__, __LINE__); }
  // the reduced-precision pre-filter (pref_wish), now that k_reset has produced the first sweep vector
  if (pw.want) {
    rc = bc_pref_create(phi, pw.prec, &h->pref);
    if (rc) { bc_snnls_destroy(h); return rc; }
    const char* cap = getenv("BC_PREFILTER_CAP");
    if (cap) bc_pref_set_cap(h->pref, atoi(cap));
    if (d.qv && bc_pref_sp4(h->pref) == d.sp4) bc_pref_set_qv(h->pref, d.qv);
    if (d.qv4 && bc_pref_two_level(h->pref) && bc_pref_sp8(h->pref) == d.sp8) bc_pref_set_qv4(h->pref, d.qv4);
  }
  *out = h;
  return BC_OK;
}

extern "C" int bc_snnls_set_tolerance(bc_snnls* h, double tol) {
  if (!h) return BC_INVALID_ARGUMENT;
  h->d.tol = tol;
  return BC_OK;
}

// ------------------------------------------------------------------ readers and counters
static int fetch_state(bc_snnls* h, SnnlsState* out) {
  bc_ctx* ctx = h->ctx;
  BC_HIP(hipMemcpyAsync(ctx->pinned, h->d.st, sizeof(SnnlsState), hipMemcpyDeviceToHost, ctx->stream));
  BC_HIP(hipStreamSynchronize(ctx->stream));
  memcpy(out, ctx->pinned, sizeof(SnnlsState));
  if (out->overflow) {
    bc_set_error("bc_snnls: active-list capacity exceeded on device (internal error)");
    return BC_INVALID_ARGUMENT;
  }
  return BC_OK;
}

extern "C" int bc_snnls_prefilter_active(const bc_snnls* h, int* on) {
  if (!h || !on) return BC_INVALID_ARGUMENT;
  *on = h->pref ? bc_pref_precision(h->pref) : 0;   // 0 = off, else the storage precision (16 / 32)
  return BC_OK;
}

extern "C" int bc_snnls_prefilter_form(const bc_snnls* h, int* form) {
  if (!h || !form) { bc_set_error("bc_snnls_prefilter_form: bad argument"); return BC_INVALID_ARGUMENT; }
  *form = !h->pref ? 0 : (bc_pref_bb(h->pref) ? 2 : (bc_pref_two_level_active(h->pref) ? 3 : 1));      // (3 put aside by the watch: 1)
  return BC_OK;
}

extern "C" int bc_snnls_finish_form(const bc_snnls* h, int* form) {
  if (!h || !form) { bc_set_error("bc_snnls_finish_form: bad argument"); return BC_INVALID_ARGUMENT; }
  *form = h->finish_form;
  return BC_OK;
}

extern "C" int bc_snnls_prefilter_fallbacks(const bc_snnls* h, int64_t* n) {
  if (!h || !n) return BC_INVALID_ARGUMENT;
  *n = 0;
  if (!h->pref) return BC_OK;
  bc_pref_counters c;
  const int rc = bc_pref_read_counters(h->pref, &c);
  if (rc) return rc;
  *n = c.overflows;
  return BC_OK;
}

extern "C" int bc_snnls_prefilter_stats(const bc_snnls* h, int64_t* sweeps, int64_t* candidates, int64_t* fallbacks) {
  if (!h) return BC_INVALID_ARGUMENT;
  if (sweeps) *sweeps = 0;
  if (candidates) *candidates = 0;
  if (fallbacks) *fallbacks = 0;
  if (!h->pref) return BC_OK;
  bc_pref_counters c;
  const int rc = bc_pref_read_counters(h->pref, &c);
  if (rc) return rc;
  if (sweeps) *sweeps = c.sweeps;
  if (candidates) *candidates = c.rescored;
  if (fallbacks) *fallbacks = c.overflows;
  return BC_OK;
}

extern "C" int bc_snnls_prefilter_levels(const bc_snnls* h, int64_t* l1_sweeps, int64_t* listed, int64_t* refined) {
  if (!h) { bc_set_error("bc_snnls_prefilter_levels: bad argument"); return BC_INVALID_ARGUMENT; }
  if (l1_sweeps) *l1_sweeps = 0;
  if (listed) *listed = 0;
  if (refined) *refined = 0;
  if (!h->pref || !bc_pref_two_level(h->pref)) return BC_OK;
  bc_pref_counters c;
  const int rc = bc_pref_read_counters(h->pref, &c);
  if (rc) return rc;
  if (l1_sweeps) *l1_sweeps = c.l1_seq;
  if (listed) *listed = c.l1_passed;               // (every row the first level passes on is re-bounded by the same wave)
  if (refined) *refined = c.l1_passed;
  return BC_OK;
}

extern "C" int bc_snnls_record_doubles(const bc_snnls* h, int32_t* n) {
  if (!h || !n) return BC_INVALID_ARGUMENT;
  *n = h->d.rec_len;
  return BC_OK;
}

extern "C" int bc_snnls_error(bc_snnls* h, double* err) {
  if (!h || !err) return BC_INVALID_ARGUMENT;
  SnnlsState st;
  int rc = fetch_state(h, &st);
  if (rc) return rc;
  *err = st.err_cur;
  return BC_OK;
}

extern "C" int bc_snnls_size(bc_snnls* h, int64_t* n) {
  if (!h || !n) return BC_INVALID_ARGUMENT;
  SnnlsState st;
  int rc = fetch_state(h, &st);
  if (rc) return rc;
  *n = st.npos;
  return BC_OK;
}

extern "C" int bc_snnls_weights(bc_snnls* h, int64_t cap, int64_t* idx, double* val, int64_t* n) {
  if (!h || !n) return BC_INVALID_ARGUMENT;
  SnnlsState st;
  int rc = fetch_state(h, &st);
  if (rc) return rc;
  *n = st.nnz;
  if (st.nnz == 0 || (!idx && !val)) return BC_OK;
  if (cap < st.nnz) { bc_set_error("bc_snnls_weights: capacity %lld < nnz %lld", (long long)cap, (long long)st.nnz); return BC_INVALID_ARGUMENT; }
  if (idx) BC_HIP(hipMemcpyAsync(idx, h->d.idx, st.nnz * sizeof(long long), hipMemcpyDeviceToHost, h->ctx->stream));
  if (val) BC_HIP(hipMemcpyAsync(val, h->d.val, st.nnz * sizeof(double), hipMemcpyDeviceToHost, h->ctx->stream));
  BC_HIP(hipStreamSynchronize(h->ctx->stream));
  return BC_OK;
}

extern "C" int bc_snnls_columns(bc_snnls* h, int64_t cap, double* cols, int64_t* n) {
  if (!h || !n) return BC_INVALID_ARGUMENT;
  SnnlsState st;
  int rc = fetch_state(h, &st);
  if (rc) return rc;
  *n = st.nnz;
  if (st.nnz == 0 || !cols) return BC_OK;
  if (cap < st.nnz) { bc_set_error("bc_snnls_columns: capacity too small"); return BC_INVALID_ARGUMENT; }
  BC_HIP(hipMemcpyAsync(cols, h->d.cols, (size_t)st.nnz * h->d.s * sizeof(double), hipMemcpyDeviceToHost, h->ctx->stream));
  BC_HIP(hipStreamSynchronize(h->ctx->stream));
  return BC_OK;
}

extern "C" int bc_snnls_get_flags(bc_snnls* h, int* reached_numeric_limit) {
  if (!h) return BC_INVALID_ARGUMENT;
  SnnlsState st;
  int rc = fetch_state(h, &st);
  if (rc) return rc;
  if (reached_numeric_limit) *reached_numeric_limit = st.reached_limit;
  return BC_OK;
}

extern "C" int bc_snnls_trace(bc_snnls* h, int64_t cap, int64_t* f, int32_t* status, double* err, int64_t* n) {
  if (!h || !n) return BC_INVALID_ARGUMENT;
  SnnlsState st;
  int rc = fetch_state(h, &st);
  if (rc) return rc;
  long long m = std::min<long long>(st.iter, h->d.tr_cap);
  *n = m;
  if (m == 0 || (!f && !status && !err)) return BC_OK;
  if (cap < m) { bc_set_error("bc_snnls_trace: capacity too small"); return BC_INVALID_ARGUMENT; }
  hipStream_t sm = h->ctx->stream;
  if (f) BC_HIP(hipMemcpyAsync(f, h->d.tr_f, m * sizeof(long long), hipMemcpyDeviceToHost, sm));
  if (status) BC_HIP(hipMemcpyAsync(status, h->d.tr_status, m * sizeof(int), hipMemcpyDeviceToHost, sm));
  if (err) BC_HIP(hipMemcpyAsync(err, h->d.tr_err, m * sizeof(double), hipMemcpyDeviceToHost, sm));
  BC_HIP(hipStreamSynchronize(sm));
  return BC_OK;
}

// ------------------------------------------------------------------ exchange binding
extern "C" int bc_snnls_bind_exchange(bc_snnls* h, int world, void* cand_send_dev, void* cand_all_dev) {
  if (!h || world < 1 || (world > 1 && (!cand_send_dev || !cand_all_dev))) {
    bc_set_error("bc_snnls_bind_exchange: bad argument");
    return BC_INVALID_ARGUMENT;
  }
  BC_HIP(hipStreamSynchronize(h->ctx->stream));
  if (cand_send_dev && cand_all_dev) {
    h->cand_send = (double*)cand_send_dev;      // borrowed (typically torch tensors); the own record stays in the state slab
    h->cand_send_owned = false;
    h->d.cand_all = (const double*)cand_all_dev;
  } else {
    h->d.cand_all = h->cand_send;
  }
  h->d.world = world;
  return BC_OK;
}

extern "C" int bc_snnls_bind_comm(bc_snnls* h, bc_comm* c) {
  if (!h || !c) { bc_set_error("bc_snnls_bind_comm: bad argument"); return BC_INVALID_ARGUMENT; }
  if (!h->cand_send_owned || h->comm) { bc_set_error("bc_snnls_bind_comm: an exchange is already bound"); return BC_INVALID_ARGUMENT; }
  int32_t rank = 0, world = 1;
  bc_comm_info(c, &rank, &world);
  BC_HIP(hipStreamSynchronize(h->ctx->stream));
  const size_t bytes = (size_t)world * h->d.rec_len * sizeof(double);
  BC_HIP(hipMalloc((void**)&h->cand_all_owned, bytes));
  BC_HIP(hipMemsetAsync(h->cand_all_owned, 0, bytes, h->ctx->stream));
  h->d.cand_all = h->cand_all_owned;
  h->d.world = world;
  h->comm = c;
  return BC_OK;
}

// the record all-gather between the local sweep and the replicated finish / pick (native exchange only)
static int exchange(bc_snnls* h) {
  if (!h->comm) return BC_OK;
  int rc = bc_timer_begin(h->ctx, 4);
  if (!rc) rc = bc_comm_all_gather_dev(h->comm, h->cand_send, h->cand_all_owned, (size_t)h->d.rec_len);
  if (!rc) rc = bc_timer_end(h->ctx, 4);
  return rc;
}

// ------------------------------------------------------------------ launch helpers
#define LAUNCH1(kern, ...)                                                         \
  do {                                                                             \
    hipLaunchKernelGGL(kern, dim3(1), dim3(BC_FIN_THREADS), 0, h->ctx->stream, __VA_ARGS__);   \
    BC_HIP(hipGetLastError());                                                     \
  } while (0)

#define BY_ALG(kern, ...)                                                          \
  do {                                                                             \
    if (h->alg == BC_ALG_GIGA) LAUNCH1(kern<BC_ALG_GIGA>, __VA_ARGS__);             \
    else if (h->alg == BC_ALG_FW) LAUNCH1(kern<BC_ALG_FW>, __VA_ARGS__);            \
    else LAUNCH1(kern<BC_ALG_OMP>, __VA_ARGS__);                                    \
  } while (0)

static int launch_prep(bc_snnls* h, int reset_retry) {
  BY_ALG(k_prep, h->d, reset_retry);
  return BC_OK;
}

// the finish kernel may take the sweep's block candidates directly when nobody else needs the record
static bool fuse_winner(const bc_snnls* h) { return h->d.world == 1 && h->cand_send_owned && !h->pref && !h->comm; }
static bool use_pref(const bc_snnls* h) { return h->pref && !h->pref_suspended && !h->exact_step; }

#define BC_RS_MAX_DYN_LDS (48 * 1024)   // dynamic LDS the fused kernel may ask for (on top of ~42 KB static: rescoring strips, lists)
// one-round-of-loads finish kernel (k_step_finish_pf) possible for the step in flight?
static bool finish_pf_ok(const bc_snnls* h, long long nrec) {
  return !h->no_pf && h->d.s <= BC_FIN_THREADS && h->nnz_upper + 1 <= BC_PF_MAXNNZ && nrec <= BC_PF_MAXREC && h->nnz_upper + 1 <= h->d.cap;
}
// ... with the rescoring stage inside the same launch (single rank, pre-filtered sweep)?
static bool fused_rescore_ok(const bc_snnls* h) {
  if (h->no_fuse || !use_pref(h) || h->d.world != 1 || h->comm || !h->cand_send_owned) return false;
  if (!finish_pf_ok(h, h->d.rec_len)) return false;
  const size_t lds = ((size_t)5 * h->d.s + h->d.rec_len + 2 * (size_t)(h->nnz_upper + 1)) * sizeof(double);
  // static LDS of the fused kernel (rescoring strips 32 KB, current / best row 16 KB, tile list 4 KB, ...) + the dynamic part
  // must fit the device's per-block limit (160 KB on gfx950; the two-launch path is taken otherwise)
  return lds <= BC_RS_MAX_DYN_LDS && lds + 64 * 1024 <= (size_t)h->ctx->max_lds;      // (63.5 KB static, of which 4 KB dev_prep copy of the sweep vectors and 2 KB image of the digit records)
}

static int launch_sweep(bc_snnls* h, bool with_record, bool allow_fused) {
  h->rs_pending = false;
  if (use_pref(h)) {
    // reduced-precision pre-filter -> candidates -> exact fp64 rescoring into the record
    if (allow_fused && fused_rescore_ok(h)) {
      h->rs_pending = true;       // step_finish runs rescoring + finish as one launch
      return bc_pref_launch_sweep(h->pref, mode_of(h), h->d.v, &h->d.st->v_norm, 1.0, &h->d.st->skip, h->cand_send, &h->rs);
    }
    return bc_pref_launch(h->pref, mode_of(h), h->d.v, &h->d.st->v_norm, 1.0, &h->d.st->skip, h->cand_send);
  }
  const bool rec = with_record || h->exact_step || h->pref != nullptr;     // (pref suspended: the finish reads the record)
  return bc_launch_sweep(h->phi, mode_of(h), h->d.v, 1.0, &h->d.st->skip, rec ? h->cand_send : nullptr);
}

// ------------------------------------------------------------------ device refit
static size_t nnls_lds_bytes(int s_vecs) { return ((size_t)BC_NNLS_WS_DOUBLES + (size_t)5 * s_vecs) * sizeof(double); }

// Gram state of the list and the refit counters (allocated on first use), and the kernels' dynamic-LDS allowance: the packed
// factor alone is 66 KB, above the 64 KB a kernel gets without asking
static int ensure_nnls(bc_snnls* h, const char* who) {
  if (h->d.world != 1 || h->comm || !h->cand_send_owned) {
    bc_set_error("%s: the device NNLS refit serves single-rank solvers only (world != 1: sharded solvers keep the host refit)", who);
    return BC_INVALID_ARGUMENT;
  }
  const size_t need = nnls_lds_bytes(h->d.s <= 1024 ? h->d.s : 0) + 16 * 1024;      // + the step kernel's static LDS
  if (need > (size_t)h->ctx->max_lds) {
    bc_set_error("%s: the device NNLS refit needs %zu bytes of LDS per block, the device offers %d", who, need, h->ctx->max_lds);
    return BC_INVALID_ARGUMENT;
  }
  static unsigned attr_done_mask = 0;      // per device
  if (!((attr_done_mask >> (h->ctx->device & 31)) & 1u)) {
    BC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_step_finish<BC_ALG_OMP>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)nnls_lds_bytes(1024)));
    BC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_refit), hipFuncAttributeMaxDynamicSharedMemorySize, (int)nnls_lds_bytes(0)));
    attr_done_mask |= 1u << (h->ctx->device & 31);
  }
  if (h->nnls_slab) return BC_OK;
  const size_t gram_doubles = (size_t)BC_NNLS_MAXP * BC_NNLS_MAXP + BC_NNLS_MAXP;
  const size_t bytes = gram_doubles * sizeof(double) + 4 * sizeof(long long);
  char* slab = nullptr;
  BC_HIP(hipMalloc((void**)&slab, bytes));
  hipError_t e = hipMemsetAsync(slab, 0, bytes, h->ctx->stream);
  if (e != hipSuccess) { (void)hipFree(slab); return bc_hip_fail(e, "hipMemsetAsync(nnls)", __FILE__, __LINE__); }
  h->nnls_slab = slab;
  h->d.gram = (double*)slab;
  h->d.gram_c = h->d.gram + (size_t)BC_NNLS_MAXP * BC_NNLS_MAXP;
  h->d.nnls_stats = (long long*)(slab + gram_doubles * sizeof(double));
  return BC_OK;
}

extern "C" int bc_snnls_device_refit(bc_snnls* h, int on) {
  if (!h) { bc_set_error("bc_snnls_device_refit: bad argument"); return BC_INVALID_ARGUMENT; }
  if (on) {
    const int rc = ensure_nnls(h, "bc_snnls_device_refit");
    if (rc) return rc;
  }
  h->dev_refit = on != 0;
  return BC_OK;
}

// one launch of k_refit and the status it left
static int run_refit(bc_snnls* h, long long f, int mode, const char* who, SnnlsState* st) {
  int rc = ensure_nnls(h, who);
  if (rc) return rc;
  if (h->nnz_upper > BC_NNLS_MAXP) {
    bc_set_error("%s: the device NNLS refit holds at most %d list entries (BC_NNLS_MAXP), the list has %lld", who, BC_NNLS_MAXP, h->nnz_upper);
    return BC_INVALID_ARGUMENT;
  }
  rc = ensure_capacity(h, h->nnz_upper + 1);
  if (rc) return rc;
  hipLaunchKernelGGL(k_refit, dim3(1), dim3(BC_FIN_THREADS), nnls_lds_bytes(0), h->ctx->stream, h->d, f, mode);
  BC_HIP(hipGetLastError());
  rc = fetch_state(h, st);
  if (rc) return rc;
  h->nnz_upper = st->nnz;
  if (st->last_status == BC_ST_LIST_LIMIT) {
    bc_set_error("%s: the device NNLS refit holds at most %d list entries (BC_NNLS_MAXP); column %lld would be one more", who, BC_NNLS_MAXP, f);
    return BC_INVALID_ARGUMENT;
  }
  return BC_OK;
}

extern "C" int bc_snnls_refit(bc_snnls* h, int64_t f) {
  if (!h) { bc_set_error("bc_snnls_refit: bad argument"); return BC_INVALID_ARGUMENT; }
  SnnlsState st;
  const int rc = run_refit(h, f < 0 ? -1 : (long long)f, f < 0 ? 1 : 0, "bc_snnls_refit", &st);
  if (rc) return rc;
  if (st.last_status == BC_NUMERICAL_PRECISION) bc_set_error("bc_snnls_refit: the NNLS refit did not converge (numerically rank-deficient active set)");
  if (st.last_status == BC_INVALID_ARGUMENT) bc_set_error("bc_snnls_refit: column %lld is not available on this rank", (long long)f);
  return st.last_status;
}

extern "C" int bc_snnls_optimize(bc_snnls* h, int* accepted) {
  if (!h || !accepted) { bc_set_error("bc_snnls_optimize: bad argument"); return BC_INVALID_ARGUMENT; }
  SnnlsState st;
  const int rc = run_refit(h, -1, 2, "bc_snnls_optimize", &st);
  if (rc) return rc;
  *accepted = st.last_status == BC_OK ? 1 : 0;
  return BC_OK;
}

extern "C" int bc_snnls_refit_stats(const bc_snnls* h, int64_t* refits, int64_t* solves, int64_t* rejected) {
  if (!h) { bc_set_error("bc_snnls_refit_stats: bad argument"); return BC_INVALID_ARGUMENT; }
  long long v[3] = {0, 0, 0};
  if (h->d.nnls_stats) {
    BC_HIP(hipMemcpyAsync(v, h->d.nnls_stats, sizeof(v), hipMemcpyDeviceToHost, h->ctx->stream));
    BC_HIP(hipStreamSynchronize(h->ctx->stream));
  }
  if (refits) *refits = v[0];
  if (solves) *solves = v[1];
  if (rejected) *rejected = v[2];
  return BC_OK;
}

// ------------------------------------------------------------------ fused loop
extern "C" int bc_snnls_build_begin(bc_snnls* h, int itrs) {
  if (!h || itrs < 0) { bc_set_error("bc_snnls_build_begin: bad argument"); return BC_INVALID_ARGUMENT; }
  if (h->alg == BC_ALG_OMP && !h->dev_refit) {
    bc_set_error("bc_snnls_build*: OrthoPursuit refits with a host NNLS every step; use the step-wise protocol");
    return BC_INVALID_ARGUMENT;
  }
  if (h->alg == BC_ALG_OMP && h->nnz_upper + itrs > BC_NNLS_MAXP) {
    bc_set_error("bc_snnls_build*: the device NNLS refit holds at most %d list entries (BC_NNLS_MAXP); %lld are listed and %d steps "
                 "may add as many", BC_NNLS_MAXP, h->nnz_upper, itrs);
    return BC_INVALID_ARGUMENT;
  }
  int rc = ensure_capacity(h, h->nnz_upper + itrs);
  if (!rc) rc = ensure_trace(h, h->iter_upper + itrs);
  if (rc) return rc;
  h->pref_suspended = false;
  h->consec_overflow = 0;
  h->exact_step = false;
  return launch_prep(h, 1);
}

extern "C" int bc_snnls_step_local(bc_snnls* h) {
  if (!h) return BC_INVALID_ARGUMENT;
  h->exact_step = false;
  if (h->alg == BC_ALG_OMP) return launch_sweep(h, true, false);      // k_step_finish<BC_ALG_OMP> consumes the candidate record
  return launch_sweep(h, !fuse_winner(h), true);
}

extern "C" int bc_snnls_step_local_exact(bc_snnls* h) {
  if (!h) return BC_INVALID_ARGUMENT;
  hipLaunchKernelGGL(k_clear_pf_overflow, dim3(1), dim3(1), 0, h->ctx->stream, h->d.st);
  BC_HIP(hipGetLastError());
  h->exact_step = true;
  return launch_sweep(h, true, false);
}

// which finish kernel serves the step in flight (`fused`: step_local ran the sweep only); bc_snnls_finish_form reports it
static int finish_form(const bc_snnls* h, bool fused, long long nrec) {
  if (h->alg == BC_ALG_OMP) return BC_FINISH_OMP;
  if (fused) return h->rs.bb.rec != nullptr ? BC_FINISH_ONE_ROUND_BB : BC_FINISH_ONE_ROUND_RESCORE;      // (bb: bc_prefilter_bb.h's sweep)
  return finish_pf_ok(h, nrec) ? BC_FINISH_ONE_ROUND : BC_FINISH_PLAIN;
}

#define FIN_KERNEL(...) reinterpret_cast<const void*>(&__VA_ARGS__)
static const void* const fin_kernels[BC_FINISH_OMP + 1][3] = {
    {nullptr, nullptr, nullptr},
    {FIN_KERNEL(k_step_finish<BC_ALG_GIGA>), FIN_KERNEL(k_step_finish<BC_ALG_FW>), nullptr},
    {FIN_KERNEL(k_step_finish_pf<BC_ALG_GIGA, 0>), FIN_KERNEL(k_step_finish_pf<BC_ALG_FW, 0>), nullptr},
    {FIN_KERNEL(k_step_finish_pf<BC_ALG_GIGA, 1>), FIN_KERNEL(k_step_finish_pf<BC_ALG_FW, 1>), nullptr},
    {FIN_KERNEL(k_step_finish_pf<BC_ALG_GIGA, 2>), FIN_KERNEL(k_step_finish_pf<BC_ALG_FW, 2>), nullptr},
    {nullptr, nullptr, FIN_KERNEL(k_step_finish<BC_ALG_OMP>)},
};

extern "C" int bc_snnls_step_finish(bc_snnls* h) {
  if (!h) return BC_INVALID_ARGUMENT;
  SnnlsDev d = h->d;
  const bool rec_based = h->exact_step || h->pref != nullptr;
  d.fuse_winner = (fuse_winner(h) && !rec_based && h->alg != BC_ALG_OMP) ? 1 : 0;
  d.blk_val = h->phi->blk_val;
  d.blk_idx = h->phi->blk_idx;
  d.nblk = h->phi->sweep_blocks;
  const bool fused = h->rs_pending;
  h->rs_pending = false;
  h->exact_step = false;
  const long long nrec = fused ? d.rec_len : (d.fuse_winner ? 0 : (long long)d.world * d.rec_len);
  if (h->alg == BC_ALG_OMP && (!h->dev_refit || !d.gram)) {
    bc_set_error("bc_snnls_step_finish: OrthoPursuit without bc_snnls_device_refit");
    return BC_INVALID_ARGUMENT;
  }
  const int form = finish_form(h, fused, nrec);
  const bool one_round = form != BC_FINISH_PLAIN && form != BC_FINISH_OMP;
  if (fused) {
    static unsigned attr_done_mask = 0;  // 42 KB static + up to 48 KB dynamic LDS: above the 64 KB default limit; per device
    if (!((attr_done_mask >> (h->ctx->device & 31)) & 1u)) {
      for (int f = BC_FINISH_ONE_ROUND_RESCORE; f <= BC_FINISH_ONE_ROUND_BB; ++f)
        for (int a = BC_ALG_GIGA; a <= BC_ALG_FW; ++a)
          BC_HIP(hipFuncSetAttribute(fin_kernels[f][a], hipFuncAttributeMaxDynamicSharedMemorySize, BC_RS_MAX_DYN_LDS));
      attr_done_mask |= 1u << (h->ctx->device & 31);
    }
  }
  // the one-round kernels take (list-length bound, rescoring arguments, rows); the others whether the S-vectors fit LDS
  int hint_or_vecs = one_round ? (int)h->nnz_upper : (d.s <= 1024 ? 1 : 0);
  long long n_rows = h->phi->n_rows;
  const size_t lds_doubles = one_round ? (size_t)5 * d.s + nrec + 2 * (size_t)(hint_or_vecs + 1)
                                       : (form == BC_FINISH_OMP ? BC_NNLS_WS_DOUBLES : 0) + (hint_or_vecs ? (size_t)5 * d.s : 0);
  void* args[] = {&d, &hint_or_vecs, &h->rs, &n_rows};
  int rc = bc_timer_begin(h->ctx, 5);
  if (rc) return rc;
  BC_HIP(hipLaunchKernel(fin_kernels[form][h->alg], dim3(1), dim3(BC_FIN_THREADS), args, lds_doubles * sizeof(double), h->ctx->stream));
  h->finish_form = form;
  h->nnz_upper += 1;
  h->iter_upper += 1;
  return bc_timer_end(h->ctx, 5);
}

extern "C" int bc_snnls_build_end(bc_snnls* h, int* reached_numeric_limit, int* iterations_consumed, int* pending_exact) {
  if (!h) return BC_INVALID_ARGUMENT;
  SnnlsState st;
  int rc = fetch_state(h, &st);
  if (rc) return rc;
  h->nnz_upper = st.nnz;
  h->iter_upper = st.iter;
  if (h->pref) {                                  // (the stream is idle: the two-level form's watch costs one small copy)
    rc = bc_pref_adapt(h->pref);
    if (rc) return rc;
  }
  if (reached_numeric_limit) *reached_numeric_limit = st.reached_limit;
  if (iterations_consumed) *iterations_consumed = (int)st.iter;
  if (pending_exact) *pending_exact = st.pf_overflow;
  if (st.pf_overflow) {
    // all ranks see the same replicated state, so they take this branch together
    if (++h->consec_overflow >= 3) h->pref_suspended = true;     // e.g. a design full of exact duplicates: stop trying
  } else {
    h->consec_overflow = 0;
  }
  return BC_OK;
}

extern "C" int bc_snnls_build(bc_snnls* h, int itrs, int* reached_numeric_limit) {
  if (!h) return BC_INVALID_ARGUMENT;
  if (h->d.world != 1 && !h->comm) {
    bc_set_error("bc_snnls_build: world > 1 without a bound bc_comm: the host must all-gather between step_local and step_finish");
    return BC_INVALID_ARGUMENT;
  }
  const long long iter0 = h->iter_upper;
  int rc = bc_snnls_build_begin(h, itrs);
  if (rc) return rc;
  int left = itrs, lim = 0;
  while (true) {
    for (int i = 0; i < left && !rc; ++i) {
      rc = bc_snnls_step_local(h);
      if (!rc) rc = exchange(h);
      if (!rc) rc = bc_snnls_step_finish(h);
      // a long call: let the two-level form's watch look every 64 steps (a stream synchronisation: ~0.5 us per step)
      if (!rc && h->pref && bc_pref_two_level(h->pref) && (i & 63) == 63 && i + 1 < left) rc = bc_pref_adapt(h->pref);
    }
    if (rc) return rc;
    int consumed = 0, pending = 0;
    rc = bc_snnls_build_end(h, &lim, &consumed, &pending);
    if (rc) return rc;
    if (!pending) break;
    // the pre-filter overflowed at step `consumed - iter0`: that step and everything enqueued after it were no-ops.
    // Redo it through the exact sweep, then go on with what is left.
    rc = bc_snnls_step_local_exact(h);
    if (!rc) rc = exchange(h);
    if (!rc) rc = bc_snnls_step_finish(h);
    if (rc) return rc;
    left = itrs - (int)(consumed - iter0) - 1;
    if (left <= 0) {
      rc = bc_snnls_build_end(h, &lim, nullptr, nullptr);
      if (rc) return rc;
      break;
    }
  }
  if (reached_numeric_limit) *reached_numeric_limit = lim;
  return BC_OK;
}

// ------------------------------------------------------------------ step-wise protocol
extern "C" int bc_snnls_select_local(bc_snnls* h) {
  if (!h) return BC_INVALID_ARGUMENT;
  int rc = launch_prep(h, 0);
  if (rc) return rc;
  h->exact_step = false;
  h->pref_suspended = false;
  return launch_sweep(h, true, false);
}

extern "C" int bc_snnls_select_local_exact(bc_snnls* h) {
  if (!h) return BC_INVALID_ARGUMENT;
  h->exact_step = true;
  const int rc = launch_sweep(h, true, false);
  h->exact_step = false;
  return rc;
}

extern "C" int bc_snnls_select_pick(bc_snnls* h, int64_t* f) {
  if (!h || !f) return BC_INVALID_ARGUMENT;
  BY_ALG(k_pick, h->d);
  SnnlsState st;
  int rc = fetch_state(h, &st);
  if (rc) return rc;
  *f = st.sel_f;
  if (st.last_status == BC_RETRY_EXACT) return BC_RETRY_EXACT;                   // no error text: the caller re-sweeps exactly
  if (st.last_status == BC_NUMERICAL_PRECISION) bc_set_error("cdirnrm < TOL");   // giga.py:28-29
  if (st.last_status == BC_INVALID_ARGUMENT) bc_set_error("bc_snnls_select: no selectable row");
  return st.last_status;
}

extern "C" int bc_snnls_select(bc_snnls* h, int64_t* f) {
  if (!h || !f) return BC_INVALID_ARGUMENT;
  if (h->d.world != 1 && !h->comm) {
    bc_set_error("bc_snnls_select: world > 1 without a bound bc_comm: use select_local / all-gather / select_pick");
    return BC_INVALID_ARGUMENT;
  }
  int rc = bc_snnls_select_local(h);
  if (!rc) rc = exchange(h);
  if (rc) return rc;
  rc = bc_snnls_select_pick(h, f);
  if (rc != BC_RETRY_EXACT) return rc;
  rc = bc_snnls_select_local_exact(h);          // a pre-filter overflowed on some rank: the same step, exact sweep
  if (!rc) rc = exchange(h);
  if (rc) return rc;
  return bc_snnls_select_pick(h, f);
}

extern "C" int bc_snnls_reweight(bc_snnls* h, int64_t f) {
  if (!h) return BC_INVALID_ARGUMENT;
  if (h->alg == BC_ALG_OMP) {
    bc_set_error("bc_snnls_reweight: OrthoPursuit reweights on the host (orthopursuit.py:37-42); use set_weights");
    return BC_INVALID_ARGUMENT;
  }
  int rc = ensure_capacity(h, h->nnz_upper + 1);
  if (rc) return rc;
  if (h->alg == BC_ALG_GIGA) LAUNCH1(k_reweight<BC_ALG_GIGA>, h->d, (long long)f);
  else LAUNCH1(k_reweight<BC_ALG_FW>, h->d, (long long)f);
  SnnlsState st;
  rc = fetch_state(h, &st);
  if (rc) return rc;
  h->nnz_upper = st.nnz;
  if (st.last_status == BC_NUMERICAL_PRECISION) bc_set_error("precision loss in the closed-form step");
  if (st.last_status == BC_INVALID_ARGUMENT) bc_set_error("bc_snnls_reweight: column %lld is not available on this rank", (long long)f);
  return st.last_status;
}

extern "C" int bc_snnls_set_weights(bc_snnls* h, int64_t n, const int64_t* idx, const double* val, const double* cols) {
  if (!h || n < 0 || (n > 0 && (!idx || !val))) { bc_set_error("bc_snnls_set_weights: bad argument"); return BC_INVALID_ARGUMENT; }
  bc_ctx* ctx = h->ctx;
  int rc = ensure_capacity(h, std::max<long long>(n, h->nnz_upper));
  if (rc) return rc;
  const int s = h->d.s;
  long long* didx = nullptr;
  double *dval = nullptr, *dcols = nullptr;
  hipError_t e = hipSuccess;
  if (n > 0) {
    e = hipMalloc((void**)&didx, n * sizeof(long long));
    if (e == hipSuccess) e = hipMalloc((void**)&dval, n * sizeof(double));
    if (e == hipSuccess && cols) e = hipMalloc((void**)&dcols, (size_t)n * s * sizeof(double));
    if (e == hipSuccess) e = hipMemcpyAsync(didx, idx, n * sizeof(long long), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dval, val, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && cols) e = hipMemcpyAsync(dcols, cols, (size_t)n * s * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_set_weights, dim3(1), dim3(BC_FIN_THREADS), 0, ctx->stream, h->d, (long long)n, didx, dval, dcols, h->idx2,
                       h->val2, h->cols2, h->colnorm2);
    e = hipGetLastError();
  }
  SnnlsState st;
  if (e == hipSuccess) rc = fetch_state(h, &st);
  if (didx) (void)hipFree(didx);
  if (dval) (void)hipFree(dval);
  if (dcols) (void)hipFree(dcols);
  if (e != hipSuccess) return bc_hip_fail(e, "bc_snnls_set_weights", __FILE__, __LINE__);
  if (rc) return rc;
  std::swap(h->d.idx, h->idx2);
  std::swap(h->d.val, h->val2);
  std::swap(h->d.cols, h->cols2);
  std::swap(h->d.colnorm, h->colnorm2);
  h->nnz_upper = n;
  if (st.last_status != BC_OK) {
    bc_set_error("bc_snnls_set_weights: a column was not supplied and is not available on this rank");
    return st.last_status;
  }
  return BC_OK;
}

extern "C" int bc_snnls_reset(bc_snnls* h) {
  if (!h) return BC_INVALID_ARGUMENT;
  hipLaunchKernelGGL(k_reset, dim3(1), dim3(BC_FIN_THREADS), 0, h->ctx->stream, h->d);
  BC_HIP(hipGetLastError());
  BC_HIP(hipStreamSynchronize(h->ctx->stream));
  h->nnz_upper = 0;
  h->iter_upper = 0;
  return BC_OK;
}

extern "C" int bc_snnls_set_flags(bc_snnls* h, int reached_numeric_limit) {
  if (!h) return BC_INVALID_ARGUMENT;
  hipLaunchKernelGGL(k_set_flag, dim3(1), dim3(1), 0, h->ctx->stream, h->d.st, reached_numeric_limit ? 1 : 0);
  BC_HIP(hipGetLastError());
  BC_HIP(hipStreamSynchronize(h->ctx->stream));
  return BC_OK;
}
