// The chain summary (include/beta_cores_diag.h): posterior mean and covariance, split-R-hat and the effective sample size of
// P x n x C x D draws, where they lie.  Four kernels on the library's stream:
//
//   k_diag_keep        a transposing copy of a chunk [p][t][c][j] (j fastest) into the retained layout [p][j][c][i] (i fastest),
//                      in which one coordinate's N = n C draws -- and so each of its 2 C sequences -- are contiguous.  A block
//                      moves a 32 x 32 tile of (t, j) of one chain through LDS (pitch 33), so both sides are coalesced.
//   k_diag_seq         one block per (problem, coordinate): the mean (and whether a draw is not finite), m_s, v_s, W, Bh, varplus,
//                      rhat, then the lag products pair by pair until P_k is not > 0 and Geyer's monotone sums (bc_diag_dev.h).
//                      The 2 C sequences are staged in LDS when 2 C h doubles and the block's work space fit BC_DG_MAX_LDS
//                      (144 KiB, below the 160 KiB a block may take: 128 KB at n = 1000, C = 16); they are read from memory
//                      otherwise.  The same arithmetic either way.
//   k_diag_cov         the D x D product of the centred draws on v_mfma_f64_16x16x4_f64 with VGPR accumulators.  Only the tiles on
//                      or above the diagonal; N is split over blocks in chunks of BC_DIAG_COV_CHUNK draws, and a block takes up
//                      to 32 tiles (8 per wave).  A block stages its chunk 32 draws at a time in LDS, centred as it is staged
//                      (x - mean: the second pass), zero beyond D and beyond the chunk.  Operand maps as bc_pm_tile's:
//                        A: lane l holds Xc[16 I + (l & 15)][4 kk + (l >> 4)]     B: lane l holds Xc[16 J + (l & 15)][the same draw]
//                        C/D: col = l & 15, row = (l >> 4) + 4 reg
//                      Every block writes its own partial tiles: no atomics.
//   k_diag_cov_reduce  cov[a][b] = (the chunks' partials added in chunk order) / (N - 1), mirrored below the diagonal.
//
// What bounds them: k_diag_seq reads its coordinate once and then works in LDS, h L / 2 multiply-adds per sequence at most (the
// loop ends at the first pair that is not positive: a few lags for a chain that mixes); k_diag_cov is N D^2 flops (half the
// tiles) on the matrix cores against N D doubles read G times for G tile groups.  profiles/diag_notes.md has the measurements.
#include "bc_diag.h"
#include "bc_diag_dev.h"
#include "bc_slab.h"
#include "bc_batch.h"
#include <algorithm>

typedef double bc_dg_d4 __attribute__((ext_vector_type(4)));

#define BC_DG_MAX_LDS ((size_t)144 * 1024)
#define BC_DG_KC 32                      // draws staged at a time by k_diag_cov
#define BC_DG_KLD (BC_DG_KC + 1)
#define BC_DG_GROUP 32                   // tiles per block of k_diag_cov: 8 per wave
#define BC_DG_WTILES (BC_DG_GROUP / 4)

struct KeepArgs {
  const double* src;      // [p][k][c][d]
  double* dst;            // [p][d][c][n]
  int k, c, d, n, i0, tt, tj;
};

__global__ __launch_bounds__(256) void k_diag_keep(KeepArgs a) {
  __shared__ double tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  size_t b = blockIdx.x;
  const int bj = (int)(b % a.tj);
  b /= a.tj;
  const int bt = (int)(b % a.tt);
  b /= a.tt;
  const int ch = (int)(b % a.c);
  const size_t p = b / a.c;
  for (int rr = ty; rr < 32; rr += 8) {
    const int t = bt * 32 + rr, j = bj * 32 + tx;
    if (t < a.k && j < a.d) tile[rr][tx] = a.src[((p * a.k + t) * a.c + ch) * a.d + j];
  }
  __syncthreads();
  for (int rr = ty; rr < 32; rr += 8) {
    const int j = bj * 32 + rr, t = bt * 32 + tx;
    if (j < a.d && t < a.k) a.dst[((p * a.d + j) * a.c + ch) * a.n + a.i0 + t] = tile[tx][rr];
  }
}

struct SeqArgs {
  const double* keep;     // [p][d][c][n]
  const int* marks;       // [p] or null: problems marked before this launch (read only)
  int* flag;              // [p]: set to 1 by a block that finds a draw that is not finite (zero before the launch)
  double *mean, *rhat, *ess, *moments, *rho;      // [p][d], [p][d], [p][d], [p][d][2], [p][d][L + 1]
  int* truncated;         // [p][d]
  long long max_lag;
  int n, c, d, L, staged;
};

__global__ __launch_bounds__(BC_DG_BLOCK) void k_diag_seq(SeqArgs a) {
  extern __shared__ double dg_lds[];
  const size_t b = blockIdx.x, p = b / a.d;
  if (a.marks && a.marks[p] != 0) return;             // (block-uniform: nothing writes the marks while this runs)
  const double* x = a.keep + b * ((size_t)a.n * a.c);
  const DgWs W = bc_dg_ws(dg_lds, a.c, a.staged != 0);
  double mean;
  const int bad = bc_dg_mean(x, a.n * a.c, W.red, &mean);
  if (threadIdx.x == 0) {
    a.mean[b] = mean;
    if (bad) a.flag[p] = 1;                           // (every block of the problem that finds one writes the same 1)
  }
  if (bad) return;                                    // (block-uniform)
  if (a.staged) bc_dg_stage(x, a.n, a.c, dg_lds + BC_DG_WS_DOUBLES(a.c));
  double o[3], ess;
  int tr;
  bc_dg_moments(x, a.n, a.c, W, o);
  bc_dg_ess(x, a.n, a.c, a.max_lag, W, o, a.rho + b * ((size_t)a.L + 1), &ess, &tr);
  if (threadIdx.x == 0) {
    a.moments[2 * b] = o[0];
    a.moments[2 * b + 1] = o[1];
    a.rhat[b] = o[2];
    a.ess[b] = ess;
    a.truncated[b] = tr;
  }
}

struct CovArgs {
  const double* keep;     // [p][d][N]
  const double* mean;     // [p][d]
  const int* marks;       // [p] or null
  double* part;           // [p][chunk][tile][16][16]
  int d, N, chunks, tiles, groups;
};

__global__ __launch_bounds__(256) void k_diag_cov(CovArgs a) {
  extern __shared__ double cv_lds[];                  // [16 nt16][BC_DG_KLD]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 15, kq = lane >> 4;
  size_t b = blockIdx.x;
  const int g = (int)(b % a.groups);
  b /= a.groups;
  const int ch = (int)(b % a.chunks);
  const size_t p = b / a.chunks;
  if (a.marks && a.marks[p] != 0) return;             // (block-uniform)
  const int d = a.d, N = a.N, nt16 = (d + 15) >> 4, dp = 16 * nt16;
  int tI[BC_DG_WTILES], tJ[BC_DG_WTILES];
  bc_dg_d4 acc[BC_DG_WTILES];
#pragma unroll
  for (int q = 0; q < BC_DG_WTILES; ++q) {
    const int tile = g * BC_DG_GROUP + q * 4 + wv;
    bc_dg_tile_ij(nt16, tile < a.tiles ? tile : 0, &tI[q], &tJ[q]);
    acc[q] = bc_dg_d4{0., 0., 0., 0.};
  }
  const double* __restrict__ x = a.keep + p * ((size_t)d * N);
  const double* __restrict__ mu = a.mean + p * (size_t)d;
  const int r0 = ch * BC_DIAG_COV_CHUNK, r1 = r0 + BC_DIAG_COV_CHUNK < N ? r0 + BC_DIAG_COV_CHUNK : N;
  for (int c0 = r0; c0 < r1; c0 += BC_DG_KC) {
    __syncthreads();                                  // (the draws before these have been read by every wave)
    for (int e = tid; e < dp * BC_DG_KC; e += 256) {
      const int row = e / BC_DG_KC, col = e - row * BC_DG_KC, gc = c0 + col;
      cv_lds[row * BC_DG_KLD + col] = (row < d && gc < r1) ? x[(size_t)row * N + gc] - mu[row] : 0.;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < BC_DG_WTILES; ++q) {
      if (g * BC_DG_GROUP + q * 4 + wv < a.tiles) {   // (wave-uniform: every lane issues the MFMAs)
        const double* pa = cv_lds + (16 * tI[q] + r) * BC_DG_KLD + kq;
        const double* pb = cv_lds + (16 * tJ[q] + r) * BC_DG_KLD + kq;
#pragma unroll
        for (int kk = 0; kk < BC_DG_KC / 4; ++kk) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[4 * kk], pb[4 * kk], acc[q], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < BC_DG_WTILES; ++q) {
    const int tile = g * BC_DG_GROUP + q * 4 + wv;
    if (tile < a.tiles) {
      double* dst = a.part + ((p * a.chunks + ch) * a.tiles + tile) * BC_DG_TILE_DOUBLES;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) dst[(kq + 4 * reg) * 16 + r] = acc[q][reg];
    }
  }
}

__global__ __launch_bounds__(256) void k_diag_cov_reduce(const double* part, const int* marks, double* cov, long long total, int d, int N, int chunks,
                                                         int tiles) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const long long p = e / ((long long)d * d);
  if (marks && marks[p] != 0) return;
  const int ab = (int)(e - p * (long long)d * d), ai = ab / d, bi = ab - ai * d;
  cov[e] = bc_dg_cov_entry(part + (size_t)p * chunks * tiles * BC_DG_TILE_DOUBLES, chunks, d, ai, bi, N);
}

// ------------------------------------------------------------------ host side
static int64_t clipped_lag(const bc_diag_shape& s) { return std::min<int64_t>(s.max_lag, s.n / 2 - 1); }
static int64_t cov_chunks(const bc_diag_shape& s) { return (s.n * s.c + BC_DIAG_COV_CHUNK - 1) / BC_DIAG_COV_CHUNK; }

// bc_diag_run's work space, one walk: the pieces' offsets and the total cannot disagree
struct RunLayout {
  size_t part, mean, rhat, ess, cov, moments, rho, truncated, flag, total;
  explicit RunLayout(const bc_diag_shape& s) {
    const size_t pd = (size_t)s.p * s.d;
    bc_slab sl;
    part = sl.take((size_t)s.p * cov_chunks(s) * bc_dg_tiles(s.d) * BC_DG_TILE_DOUBLES);
    mean = sl.take(pd);
    rhat = sl.take(pd);
    ess = sl.take(pd);
    cov = sl.take(pd * s.d);
    moments = sl.take(2 * pd);
    rho = sl.take(pd * ((size_t)clipped_lag(s) + 1));
    truncated = sl.take((pd + 1) / 2);
    flag = sl.take(((size_t)s.p + 1) / 2);
    total = sl.total;
  }
};

static bool in_limits(const bc_diag_shape& s) {
  return s.p >= 1 && s.n >= 4 && s.c >= 1 && s.c <= BC_HMC_MAX_CHAINS && s.d >= 1 && s.d <= BC_HMC_MAX_DIM && s.max_lag >= 1 &&
         s.n * s.c < ((int64_t)1 << 31) && s.p <= BC_DIAG_MAX_WORK_DOUBLES && s.n <= BC_DIAG_MAX_WORK_DOUBLES &&
         (double)s.p * (double)s.n * s.c * s.d <= (double)BC_DIAG_MAX_WORK_DOUBLES;      // (so that no product below overflows)
}

size_t bc_diag_keep_doubles(const bc_diag_shape& s) { return bc_even((size_t)s.p * s.n * s.c * s.d); }
size_t bc_diag_run_doubles(const bc_diag_shape& s) { return RunLayout(s).total; }

extern "C" int64_t bc_diag_work_doubles(int64_t p, int64_t n, int32_t c, int32_t d, int64_t max_lag) {
  bc_diag_shape s;
  s.p = p, s.n = n, s.c = c, s.d = d, s.max_lag = max_lag;
  if (!in_limits(s)) return -1;
  const size_t total = 2 * bc_diag_keep_doubles(s) + bc_diag_run_doubles(s);
  return total <= (size_t)BC_DIAG_MAX_WORK_DOUBLES ? (int64_t)total : -1;
}

int bc_diag_check(const char* who, const bc_diag_shape& s) {
  if (s.p < 1) BC_REFUSE("%s: needs at least one problem, got %lld", who, (long long)s.p);
  if (s.c < 1 || s.c > BC_HMC_MAX_CHAINS) BC_REFUSE("%s: 1 .. %d chains are served, got %d", who, BC_HMC_MAX_CHAINS, s.c);
  if (s.d < 1 || s.d > BC_HMC_MAX_DIM) BC_REFUSE("%s: 1 .. %d coordinates are served, got %d", who, BC_HMC_MAX_DIM, s.d);
  if (s.n < 4) BC_REFUSE("%s: needs at least 4 kept iterations (two per half), got %lld", who, (long long)s.n);
  if (s.max_lag < 1) BC_REFUSE("%s: max_lag must be at least 1, got %lld", who, (long long)s.max_lag);
  if (bc_diag_work_doubles(s.p, s.n, s.c, s.d, s.max_lag) < 0)
    BC_REFUSE("%s: %lld x %lld x %d x %d draws need more than the %lld doubles of work space that are served (or n C >= 2^31)", who,
              (long long)s.p, (long long)s.n, s.c, s.d, (long long)BC_DIAG_MAX_WORK_DOUBLES);
  return BC_OK;
}

bool bc_diag_out_ok(const bc_diag_out& o) { return o.mean && o.cov && o.rhat && o.ess && o.truncated && o.status; }

int bc_diag_keep_launch(bc_ctx* ctx, const double* src_dev, const bc_diag_shape& s, int64_t k, int64_t i0, double* keep_dev) {
  KeepArgs a;
  a.src = src_dev;
  a.dst = keep_dev;
  a.k = (int)k, a.c = s.c, a.d = s.d, a.n = (int)s.n, a.i0 = (int)i0;
  a.tt = (int)((k + 31) / 32), a.tj = (s.d + 31) / 32;
  const size_t blocks = (size_t)s.p * s.c * a.tt * a.tj;      // (at most p c k d <= the cap on the work space: far below the grid's 2^31)
  hipLaunchKernelGGL(k_diag_keep, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, a);
  BC_HIP(hipGetLastError());
  return BC_OK;
}

int bc_diag_run(bc_ctx* ctx, const double* keep_dev, double* work, const bc_diag_shape& s, const int* marks_dev, const bc_diag_out& out) {
  const RunLayout lay(s);
  const size_t P = (size_t)s.p, d = (size_t)s.d, pd = P * d, L1 = (size_t)clipped_lag(s) + 1;
  int* flag_dev = reinterpret_cast<int*>(work + lay.flag);
  int* trunc_dev = reinterpret_cast<int*>(work + lay.truncated);
  BC_HIP(hipMemsetAsync(flag_dev, 0, P * sizeof(int), ctx->stream));
  SeqArgs q;
  q.keep = keep_dev;
  q.marks = marks_dev;
  q.flag = flag_dev;
  q.mean = work + lay.mean, q.rhat = work + lay.rhat, q.ess = work + lay.ess, q.moments = work + lay.moments, q.rho = work + lay.rho;
  q.truncated = trunc_dev;
  q.max_lag = s.max_lag;
  q.n = (int)s.n, q.c = s.c, q.d = s.d, q.L = (int)L1 - 1;
  const size_t ws = BC_DG_WS_DOUBLES(s.c), seqs = 2 * (size_t)s.c * (size_t)(s.n / 2);
  const size_t lds_cap = std::min(BC_DG_MAX_LDS, (size_t)ctx->max_lds);
  q.staged = (ws + seqs) * sizeof(double) <= lds_cap;
  const size_t seq_lds = (ws + (q.staged ? seqs : 0)) * sizeof(double);
  // (per device, and cheap beside the launches: set at every run instead of remembering where it was set)
  BC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_diag_seq), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_cap));
  hipLaunchKernelGGL(k_diag_seq, dim3((unsigned)pd), dim3(BC_DG_BLOCK), seq_lds, ctx->stream, q);
  BC_HIP(hipGetLastError());
  CovArgs c;
  c.keep = keep_dev;
  c.mean = q.mean;
  c.marks = marks_dev;
  c.part = work + lay.part;
  c.d = s.d, c.N = (int)(s.n * s.c), c.chunks = (int)cov_chunks(s), c.tiles = bc_dg_tiles(s.d);
  c.groups = (c.tiles + BC_DG_GROUP - 1) / BC_DG_GROUP;
  const size_t cov_lds = (size_t)16 * ((s.d + 15) / 16) * BC_DG_KLD * sizeof(double);      // (at most 66 KiB, at D = 256)
  BC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_diag_cov), hipFuncAttributeMaxDynamicSharedMemorySize, (int)cov_lds));
  hipLaunchKernelGGL(k_diag_cov, dim3((unsigned)(P * c.chunks * c.groups)), dim3(256), cov_lds, ctx->stream, c);
  BC_HIP(hipGetLastError());
  const long long total = (long long)(pd * d);
  hipLaunchKernelGGL(k_diag_cov_reduce, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, c.part, marks_dev, work + lay.cov, total,
                     c.d, c.N, c.chunks, c.tiles);
  BC_HIP(hipGetLastError());
  std::vector<int> flag(P), marks(P, 0);
  BC_HIP(hipMemcpyAsync(flag.data(), flag_dev, P * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  if (marks_dev) BC_HIP(hipMemcpyAsync(marks.data(), marks_dev, P * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  BC_HIP(hipStreamSynchronize(ctx->stream));
  for (size_t p = 0; p < P; ++p) flag[p] |= marks[p];
  return bc_batch_unmarked_runs(flag.data(), P, out.status, [&](size_t p, size_t e) {
    const size_t m = e - p;
    BC_HIP(hipMemcpy(out.mean + p * d, work + lay.mean + p * d, m * d * sizeof(double), hipMemcpyDeviceToHost));
    BC_HIP(hipMemcpy(out.cov + p * d * d, work + lay.cov + p * d * d, m * d * d * sizeof(double), hipMemcpyDeviceToHost));
    BC_HIP(hipMemcpy(out.rhat + p * d, work + lay.rhat + p * d, m * d * sizeof(double), hipMemcpyDeviceToHost));
    BC_HIP(hipMemcpy(out.ess + p * d, work + lay.ess + p * d, m * d * sizeof(double), hipMemcpyDeviceToHost));
    BC_HIP(hipMemcpy(out.truncated + p * d, trunc_dev + p * d, m * d * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (out.rho) BC_HIP(hipMemcpy(out.rho + p * d * L1, work + lay.rho + p * d * L1, m * d * L1 * sizeof(double), hipMemcpyDeviceToHost));
    if (out.moments) BC_HIP(hipMemcpy(out.moments + 2 * p * d, work + lay.moments + 2 * p * d, 2 * m * d * sizeof(double), hipMemcpyDeviceToHost));
    return BC_OK;
  });
}

extern "C" int bc_chain_summary(bc_ctx* ctx, const double* samples, int64_t p, int64_t n, int32_t c, int32_t d, int64_t max_lag, double* out_mean,
                                double* out_cov, double* out_rhat, double* out_ess, int32_t* out_ess_truncated, int32_t* out_status,
                                double* out_rho, double* out_moments) {
  const bc_diag_out out = {out_mean, out_cov, out_rhat, out_ess, out_ess_truncated, out_status, out_rho, out_moments};
  if (!ctx || !samples || !bc_diag_out_ok(out))
    BC_REFUSE("bc_chain_summary: bad argument (context, samples, mean, cov, rhat, ess, ess_truncated and status are required)");
  bc_diag_shape s;
  s.p = p, s.n = n, s.c = c, s.d = d, s.max_lag = max_lag;
  int rc = bc_diag_check("bc_chain_summary", s);
  if (!rc) rc = bc_ctx_refuse_busy(ctx, "bc_chain_summary", BC_HOLD_ALL);
  if (rc) return rc;
  BC_HIP(hipSetDevice(ctx->device));
  const size_t keep = bc_diag_keep_doubles(s);
  rc = bc_scratch_grow(ctx, &ctx->diag, 2 * keep + bc_diag_run_doubles(s));      // the upload | the retained layout | the run's work space
  if (rc) return rc;
  double* w = ctx->diag.p;
  BC_HIP(hipMemcpyAsync(w, samples, (size_t)p * n * c * d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  rc = bc_diag_keep_launch(ctx, w, s, n, 0, w + keep);
  if (rc) return rc;
  return bc_diag_run(ctx, w + keep, w + 2 * keep, s, nullptr, out);
}
