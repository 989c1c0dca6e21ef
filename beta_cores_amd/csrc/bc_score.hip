// The held-out scorer (include/beta_cores_score.h): k_lr_score and the stand-alone entry bc_lr_score.  The in-run entries, which
// point the same kernel at a pending chunk's sample buffer, are in bc_hmc_small.hip beside the run they belong to.
//
// k_lr_score.  For held-out rows z = y*x (Nt x D), their labels y and T parameter vectors (T x D, device memory):
//
//   s_nt = z_n . theta_t        ll[t] = sum_n ll(-s_nt)        correct[t] = #{n : the rule of bc_score_dev.h holds}
//
// The contraction is v_mfma_f64_16x16x4_f64 over tiles of 16 rows x 16 thetas, D zero-padded to a multiple of 4:
//
//   A: lane l holds Z[row l & 15][k = 4 j + (l >> 4)]     B: lane l holds Theta[theta l & 15][the same k]      step j
//   C/D: col = lane & 15 (the theta), row = (lane >> 4) + 4 reg -- the f64 map, not the map of the other dtypes
//
// so a lane works for ONE theta throughout and its B operands never change: they are loaded once into registers (4 NKB doubles,
// NKB the count of 16-column blocks D fits: the template parameter).  A wave owns one group of 16 thetas and walks ALL rows; the
// eight waves of a block own eight consecutive groups and share the rows, which the block stages in LDS 64 rows at a time (32 at
// D > 128; row pitch 16 NKB + 4 doubles, the pitch of k_lr_rows_mc's tiles).  T is tiled over the grid: ceil(T / 128) blocks.
// Rows are never split over blocks, so there is no second stage: a theta's sums are made by one wave in one fixed order
// (bc_score_dev.h has the order and the per-element arithmetic, which tests/score_harness.cpp compiles for the host).
// What bounds it: 2 T Nt D flops on the matrix cores against T Nt evaluations of exp and log1p on the fp64 VALU; at D = 16 the
// latter is nearly all of the time (profiles/score_notes.md has the measurements).
#define BC_SCORE_FN __device__
#include "bc_internal.h"
#include "bc_score_dev.h"
#include "bc_slab.h"
#include "../../include/beta_cores_score.h"
#include <cmath>

typedef double bc_d4 __attribute__((ext_vector_type(4)));

#define BC_SC_WAVES 8
#define BC_SC_TILES(NKB) ((NKB) == 16 ? 2 : 4)      // row tiles per staged chunk

struct ScoreArgs {
  const void* z;            // [nt][d] of the kernel's ZT
  const double* y;          // [nt]
  const double* theta;      // [t][d]
  int* correct;             // [t]
  double* ll;               // [t]
  long long nt, t;
  int d;
};

template <int NKB, typename ZT>
__global__ __launch_bounds__(64 * BC_SC_WAVES) void k_lr_score(ScoreArgs a) {
  extern __shared__ double sc_lds[];
  constexpr int DP = 16 * NKB, LD = DP + 4, NK = 4 * NKB, TPC = BC_SC_TILES(NKB), RC = 16 * TPC;
  double* zs = sc_lds;                     // [RC][LD]: the staged rows, zero-padded
  double* ys = sc_lds + (size_t)RC * LD;   // [RC]: their labels
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r16 = lane & 15, h = lane >> 4, d = a.d, nk = (d + 3) >> 2;
  const long long t = ((long long)blockIdx.x * BC_SC_WAVES + wv) * 16 + r16;
  const bool live = t - r16 < a.t;         // (wave-uniform: the wave's group holds at least one theta)
  double th[NK];
#pragma unroll
  for (int j = 0; j < NK; ++j) {
    const int k = 4 * j + h;
    th[j] = (t < a.t && k < d) ? a.theta[(size_t)t * d + k] : 0.;
  }
  const ZT* __restrict__ zrows = reinterpret_cast<const ZT*>(a.z);
  double acc = 0.;
  int cnt = 0;
  for (long long c0 = 0; c0 < a.nt; c0 += RC) {
    __syncthreads();                       // (the chunk before this one has been read by every wave)
    for (int e = tid; e < RC * DP; e += 64 * BC_SC_WAVES) {
      const int row = e / DP, col = e - row * DP;
      const long long gr = c0 + row;
      zs[row * LD + col] = (gr < a.nt && col < d) ? (double)zrows[(size_t)gr * d + col] : 0.;
    }
    if (tid < RC) ys[tid] = c0 + tid < a.nt ? a.y[c0 + tid] : 0.;
    __syncthreads();
    if (live) {
#pragma unroll
      for (int tile = 0; tile < TPC; ++tile) {
        const long long r0 = c0 + 16 * tile;
        if (r0 < a.nt) {                   // (block-uniform)
          const double* za = zs + (16 * tile + r16) * LD + h;
          bc_d4 m4 = bc_d4{0., 0., 0., 0.};
#pragma unroll
          for (int j = 0; j < NK; ++j)
            if (j < nk) m4 = __builtin_amdgcn_mfma_f64_16x16x4f64(za[4 * j], th[j], m4, 0, 0, 0);
          double s[4], y[4];
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            s[reg] = m4[reg];
            y[reg] = ys[16 * tile + h + 4 * reg];
          }
          bc_score_lane_tile(s, y, r0, h, a.nt, &acc, &cnt);
        }
      }
    }
  }
  if (!live) return;                       // (no barrier below)
  const double a0 = __shfl(acc, r16, BC_WAVE), a1 = __shfl(acc, r16 + 16, BC_WAVE), a2 = __shfl(acc, r16 + 32, BC_WAVE),
               a3 = __shfl(acc, r16 + 48, BC_WAVE);
  cnt += __shfl_xor(cnt, 16, BC_WAVE);
  cnt += __shfl_xor(cnt, 32, BC_WAVE);
  if (h == 0 && t < a.t) {
    a.ll[t] = bc_score_combine(a0, a1, a2, a3);
    a.correct[t] = cnt;
  }
}

// ------------------------------------------------------------------ host side
static int nkb_of(int d) { return d <= 16 ? 1 : d <= 32 ? 2 : d <= 64 ? 4 : d <= 128 ? 8 : 16; }
static size_t lds_of(int nkb) { return ((size_t)16 * BC_SC_TILES(nkb) * (16 * nkb + 4) + 16 * BC_SC_TILES(nkb)) * sizeof(double); }

template <int NKB, typename ZT>
static int launch_one(bc_ctx* ctx, dim3 grid, const ScoreArgs& a) {
  static unsigned attr_done_mask = 0;      // (the attribute is per device: one bit per device ordinal, as k_lr_rows_mc keeps it)
  const size_t lds = lds_of(NKB);
  if (!((attr_done_mask >> (ctx->device & 31)) & 1u)) {
    BC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_lr_score<NKB, ZT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr_done_mask |= 1u << (ctx->device & 31);
  }
  hipLaunchKernelGGL((k_lr_score<NKB, ZT>), grid, dim3(64 * BC_SC_WAVES), lds, ctx->stream, a);
  BC_HIP(hipGetLastError());
  return BC_OK;
}

template <int NKB>
static int launch_nkb(bc_ctx* ctx, bool f32, dim3 grid, const ScoreArgs& a) {
  return f32 ? launch_one<NKB, float>(ctx, grid, a) : launch_one<NKB, double>(ctx, grid, a);
}

int bc_score_check(const bc_ctx* ctx, const bc_data* zt, const bc_data* yt, int64_t t, int32_t d_run, const char* who) {
  if (!ctx || !zt || !yt) { bc_set_error("%s: bad argument (context, held-out rows and labels are required)", who); return BC_INVALID_ARGUMENT; }
  if (zt->ctx != ctx || yt->ctx != ctx) { bc_set_error("%s: the held-out rows and labels must live on this context", who); return BC_INVALID_ARGUMENT; }
  if (zt->dz < 1 || zt->dz > BC_HMC_MAX_DIM) { bc_set_error("%s: rows must have 1 .. %d columns, got %d", who, BC_HMC_MAX_DIM, zt->dz); return BC_INVALID_ARGUMENT; }
  if (zt->n_rows < 1) { bc_set_error("%s: needs at least one held-out row, got %lld", who, (long long)zt->n_rows); return BC_INVALID_ARGUMENT; }
  if (yt->n_rows != zt->n_rows || yt->dz != 1) {
    bc_set_error("%s: the labels must be %lld x 1 (one per held-out row), got %lld x %d", who, (long long)zt->n_rows, (long long)yt->n_rows, yt->dz);
    return BC_INVALID_ARGUMENT;
  }
  if (yt->elem != 8) return bc_refuse_f32(yt, who);
  if (d_run > 0 && zt->dz != d_run) { bc_set_error("%s: the held-out rows have %d columns, the run's problems %d", who, zt->dz, d_run); return BC_INVALID_ARGUMENT; }
  if (t < 1 || t > ((int64_t)1 << 37)) { bc_set_error("%s: needs 1 .. 2^37 parameter vectors, got %lld", who, (long long)t); return BC_INVALID_ARGUMENT; }
  return BC_OK;
}

int bc_score_launch(bc_ctx* ctx, const bc_data* zt, const bc_data* yt, const double* theta_dev, int64_t t, int* correct_dev, double* ll_dev) {
  ScoreArgs a;
  a.z = zt->z;
  a.y = yt->z;
  a.theta = theta_dev;
  a.correct = correct_dev;
  a.ll = ll_dev;
  a.nt = zt->n_rows;
  a.t = t;
  a.d = zt->dz;
  const int64_t groups = (t + 15) / 16;
  const dim3 grid((unsigned)((groups + BC_SC_WAVES - 1) / BC_SC_WAVES));
  const bool f32 = zt->elem == 4;
  int rc = bc_timer_begin(ctx, 6);      // (timed with the class of the logistic rows passes)
  if (rc) return rc;
  switch (nkb_of(a.d)) {
    case 1: rc = launch_nkb<1>(ctx, f32, grid, a); break;
    case 2: rc = launch_nkb<2>(ctx, f32, grid, a); break;
    case 4: rc = launch_nkb<4>(ctx, f32, grid, a); break;
    case 8: rc = launch_nkb<8>(ctx, f32, grid, a); break;
    default: rc = launch_nkb<16>(ctx, f32, grid, a); break;
  }
  if (rc) return rc;
  return bc_timer_end(ctx, 6);
}

extern "C" int bc_lr_score(bc_ctx* ctx, const bc_data* zt, const bc_data* yt, const double* theta, int64_t t, int32_t* out_correct,
                           double* out_ll) {
  if (!ctx || !zt || !yt || !theta || !out_correct || !out_ll) {
    bc_set_error("bc_lr_score: bad argument (context, held-out rows, labels, theta and both outputs are required)");
    return BC_INVALID_ARGUMENT;
  }
  int rc = bc_score_check(ctx, zt, yt, t, 0, "bc_lr_score");
  if (rc) return rc;
  const size_t n_th = (size_t)t * zt->dz;
  for (size_t k = 0; k < n_th; ++k)
    if (!std::isfinite(theta[k])) {
      bc_set_error("bc_lr_score: theta[%zu][%zu] = %g is not finite", k / zt->dz, k % zt->dz, theta[k]);
      return BC_INVALID_ARGUMENT;
    }
  rc = bc_ctx_refuse_busy(ctx, "bc_lr_score", BC_HOLD_HMC | BC_HOLD_HMC_SMALL);
  if (rc) return rc;
  BC_HIP(hipSetDevice(ctx->device));
  bc_slab sl;
  sl.take(n_th);                                                                    // theta | ll | correct (ints)
  const size_t o_ll = sl.take((size_t)t), o_c = sl.take(((size_t)t + 1) / 2);
  rc = bc_scratch_grow(ctx, &ctx->score, sl.total);
  if (rc) return rc;
  double* th_dev = ctx->score.p;
  double* ll_dev = ctx->score.p + o_ll;
  int* c_dev = reinterpret_cast<int*>(ctx->score.p + o_c);
  BC_HIP(hipMemcpyAsync(th_dev, theta, n_th * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  rc = bc_score_launch(ctx, zt, yt, th_dev, t, c_dev, ll_dev);
  if (rc) return rc;
  BC_HIP(hipMemcpyAsync(out_ll, ll_dev, (size_t)t * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  BC_HIP(hipMemcpyAsync(out_correct, c_dev, (size_t)t * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  BC_HIP(hipStreamSynchronize(ctx->stream));
  return BC_OK;
}
