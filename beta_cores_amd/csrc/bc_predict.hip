// The held-out scorer of the linear-regression family (include/beta_cores_predict.h): k_linreg_predict, k_linreg_predict_sum and
// the entry bc_linreg_predict.
//
// k_linreg_predict.  For held-out rows [phi_n, y_n] (Nt x (D + 1)) and T posteriors N(mu_t, F_t F_t^T) with noise_t, scale_t:
//
//   m = phi . mu      V = phi F      q = sum_j V_j^2      var = noise + scale q      term = -1/2 ((y - m)^2 / var + log var + log 2 pi)
//
// The contraction V is v_mfma_f64_16x16x4_f64 over tiles of 16 rows x 16 columns of F, D zero-padded to a multiple of 4, in the
// layout of k_lr_score (bc_score.hip) with the columns of F in the theta role:
//
//   A: lane l holds Phi[row l & 15][k = 4 j + (l >> 4)]     B: lane l holds F[the same k][column 16 g + (l & 15)]     step j
//   C/D: col = lane & 15 (the column of F), row = (lane >> 4) + 4 reg -- the f64 map
//
// The grid is (row chunks x T): a block owns BC_PRED_ROWS_PER_BLOCK rows of one posterior, so T = 1 fills the machine from
// 50 000 rows on, and stages them in LDS 64 at a time (32 at D > 128, where the whole row of up to 512 columns is staged).  The
// wave w owns the column groups w, w + 8, ...; a lane owns one column of each.
//   D <= 128 (WIDE = false): one group per wave at most, and the lane's B operands -- a whole column of F, 4 NKB doubles -- are
//     loaded once per block and stay in registers, as in k_lr_score: F costs D^2 loads per block.
//   D > 128 (WIDE = true): a column no longer fits, so F is walked in k-panels of 128 inside the block: per staged chunk, group
//     and panel the lane loads the panel's 32 operands (from L2: a posterior's F is at most 2 MiB and every block running beside
//     this one reads the same one) and carries ONE accumulator per tile through the panels, so q is complete inside the block.
// k_linreg_predict_pack first writes F in the order the lanes read it ([group][panel][step][lane], zero outside D x D), so that an
// operand load is one address and a constant stride, without a predicate (the row-major form kept 32 offsets live and spilled).
// The squares are summed per row across the wave's 16 lanes, then across the waves through LDS in wave order; the mean is eight
// fma chains per row on the vector ALU (a 129th column at D = 128 would open a ninth group for eight waves).  One thread per
// staged row then forms var, the term and the squared residual, and adds them to its own sums; a block writes its (ll, sse)
// partial, and k_linreg_predict_sum adds each posterior's partials in ascending chunk order.  No floating-point atomics.
// bc_predict_dev.h has every order and the per-row arithmetic, which tests/predict_harness.cpp compiles for the host.
// What bounds it: 2 T Nt D^2 flops on the fp64 matrix cores against the rows' bytes (profiles/predict_notes.md).
#define BC_PREDICT_FN __device__
#include "bc_internal.h"
#include "bc_predict_dev.h"
#include "bc_slab.h"
#include "../../include/beta_cores_predict.h"
#include <cmath>

typedef double bc_pd4 __attribute__((ext_vector_type(4)));

#define BC_PRED_THREADS (64 * BC_PRED_WAVES)
#define BC_PRED_MAX_BLOCKS ((long long)1 << 22)      // blocks per launch: (blocks x 512 threads) stays below 2^32

struct PredictArgs {
  const void* z;            // [nt][d + 1] of the kernel's ZT
  const double* mu;         // [t][d]
  const double* f;          // [t][groups][panels][steps][64]: F packed by k_linreg_predict_pack
  const double* noise;      // [t]
  const double* scale;      // [t]
  double* part;             // [t][chunks][2]: ll | sse
  double* mean;             // [t][nt] or null
  double* var;              // [t][nt] or null
  long long nt, chunks;
  long long t0;             // the first posterior of this launch
  int d;
};

template <int NKB, bool WIDE, typename ZT>
__global__ __launch_bounds__(BC_PRED_THREADS) void k_linreg_predict(PredictArgs a) {
  extern __shared__ double pr_lds[];
  constexpr int KP = 16 * NKB, NK = 4 * NKB, RC = WIDE ? 32 : 64, TPC = RC / 16;
  static_assert(!WIDE || KP == BC_PRED_PANEL, "the wide instance walks panels of BC_PRED_PANEL");
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r16 = lane & 15, h = lane >> 4, d = a.d, dz = d + 1;
  const int ng = BC_PRED_GROUPS(d), dp = WIDE ? 32 * ((d + 31) >> 5) : KP, LD = dp + 4, np = WIDE ? (d + KP - 1) / KP : 1;
  double* zs = pr_lds;                       // [RC][LD]: the staged features, zero-padded to dp columns
  double* ys = zs + (size_t)RC * LD;         // [RC]: their targets
  double* ms = ys + RC;                      // [RC]: their means
  double* qw = ms + RC;                      // [WAVES][RC]: the waves' sums of squares
  double* mus = qw + BC_PRED_WAVES * RC;     // [dp]: mu, zero-padded
  const long long t = a.t0 + blockIdx.x / a.chunks, chunk = blockIdx.x % a.chunks;
  const double* __restrict__ F = a.f + (size_t)t * ng * np * (NK * 64);      // packed in lane order by k_linreg_predict_pack
  const double* __restrict__ mu = a.mu + (size_t)t * d;
  const ZT* __restrict__ zrows = reinterpret_cast<const ZT*>(a.z);
  const double noise = a.noise[t], scale = a.scale[t];
  for (int e = tid; e < dp; e += BC_PRED_THREADS) mus[e] = e < d ? mu[e] : 0.;
  double b[NK];
  auto load_b = [&](int g, int p) {          // the lane's operands of group g, k-panel p: one address, constant strides
    const double* __restrict__ piece = F + (size_t)(g * np + p) * (NK * 64) + lane;
#pragma unroll
    for (int j = 0; j < NK; ++j) b[j] = piece[64 * j];
  };
  if (!WIDE && wv < ng) load_b(wv, 0);       // (wave-uniform; a wave without a group never reads b)
  const long long row0 = chunk * BC_PRED_ROWS_PER_BLOCK;
  const long long row1 = row0 + BC_PRED_ROWS_PER_BLOCK < a.nt ? row0 + BC_PRED_ROWS_PER_BLOCK : a.nt;
  double acc_ll = 0., acc_sse = 0.;
  for (long long c0 = row0; c0 < row1; c0 += RC) {
    __syncthreads();                         // (the chunk before this one has been read by every thread)
    for (int e = tid; e < RC * dp; e += BC_PRED_THREADS) {
      const int row = e / dp, col = e - row * dp;
      const long long gr = c0 + row;
      zs[row * LD + col] = (gr < row1 && col < d) ? (double)zrows[(size_t)gr * dz + col] : 0.;
    }
    if (tid < RC) ys[tid] = c0 + tid < row1 ? (double)zrows[(size_t)(c0 + tid) * dz + d] : 0.;
    __syncthreads();
    if (tid < RC * BC_PRED_MEAN_PARTS) {     // (wave-uniform: RC * 8 is a multiple of 64)
      const int row = tid >> 3, part = tid & 7;
      const double* zr = zs + row * LD;
      double s = 0.;
      for (int k = part; k < d; k += BC_PRED_MEAN_PARTS) s = fma(zr[k], mus[k], s);
      s += __shfl_xor(s, 1, BC_WAVE);
      s += __shfl_xor(s, 2, BC_WAVE);
      s += __shfl_xor(s, 4, BC_WAVE);
      if (part == 0) ms[row] = s;
    }
    auto row_sums = [&](int tile, const double* q4) {      // q4[reg]: the lane's squares of the row 16 tile + h + 4 reg
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        double x = q4[reg];
        x += __shfl_xor(x, 1, BC_WAVE);
        x += __shfl_xor(x, 2, BC_WAVE);
        x += __shfl_xor(x, 4, BC_WAVE);
        x += __shfl_xor(x, 8, BC_WAVE);
        if (r16 == 0) qw[wv * RC + 16 * tile + h + 4 * reg] = x;
      }
    };
    if constexpr (!WIDE) {                   // one group per wave at most: a tile's squares are complete at once (0 + v^2 = v^2)
#pragma unroll
      for (int tile = 0; tile < TPC; ++tile) {
        bc_pd4 m4 = bc_pd4{0., 0., 0., 0.};
        if (wv < ng && c0 + 16 * tile < row1) {      // (wave-uniform)
          const double* za = zs + (16 * tile + r16) * LD + h;
#pragma unroll
          for (int jb = 0; jb < NKB; ++jb) {         // by 16 columns; the staged rows and the packed F are zero from D on
            if (jb >= ng) break;
#pragma unroll
            for (int j = 4 * jb; j < 4 * jb + 4; ++j) m4 = __builtin_amdgcn_mfma_f64_16x16x4f64(za[4 * j], b[j], m4, 0, 0, 0);
          }
        }
        double q4[4];
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) q4[reg] = m4[reg] * m4[reg];
        row_sums(tile, q4);
        __builtin_amdgcn_sched_barrier(0);   // (keeps the next tile's LDS reads from piling up in registers)
      }
    } else {
      double qacc[TPC][4];
#pragma unroll
      for (int tile = 0; tile < TPC; ++tile)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) qacc[tile][reg] = 0.;
      for (int g = wv; g < ng; g += BC_PRED_WAVES) {      // (wave-uniform)
        bc_pd4 m4[TPC];
#pragma unroll
        for (int tile = 0; tile < TPC; ++tile) m4[tile] = bc_pd4{0., 0., 0., 0.};
        for (int p = 0; p < np; ++p) {
          load_b(g, p);
          const int nq = (dp - KP * p) >> 5;     // the panel's quarters that hold columns
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int tile = 0; tile < TPC; ++tile) {
            if (c0 + 16 * tile < row1) {     // (block-uniform)
              const double* za = zs + (16 * tile + r16) * LD + KP * p + h;
#pragma unroll
              for (int qt = 0; qt < 4; ++qt) {       // by 32 columns: the staged rows are zero from D up to dp, the packed F from D on
                if (qt >= nq) break;
#pragma unroll
                for (int j = 8 * qt; j < 8 * qt + 8; ++j) m4[tile] = __builtin_amdgcn_mfma_f64_16x16x4f64(za[4 * j], b[j], m4[tile], 0, 0, 0);
              }
            }
            __builtin_amdgcn_sched_barrier(0);
          }
        }
#pragma unroll
        for (int tile = 0; tile < TPC; ++tile)
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) qacc[tile][reg] += m4[tile][reg] * m4[tile][reg];
      }
#pragma unroll
      for (int tile = 0; tile < TPC; ++tile) row_sums(tile, qacc[tile]);
    }
    __syncthreads();
    if (tid < RC && c0 + tid < row1) {
      double var, r2;
      const double q = bc_predict_wave_q(qw + tid, RC);
      const double term = bc_predict_row(ys[tid], ms[tid], q, noise, scale, &var, &r2);
      acc_ll += term;
      acc_sse += r2;
      if (a.mean) {
        a.mean[(size_t)t * a.nt + c0 + tid] = ms[tid];
        a.var[(size_t)t * a.nt + c0 + tid] = var;
      }
    }
  }
  if (wv == 0) {                             // (the threads from RC on hold zeros)
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
      acc_ll += __shfl_xor(acc_ll, s, BC_WAVE);
      acc_sse += __shfl_xor(acc_sse, s, BC_WAVE);
    }
    if (lane == 0) {
      double* o = a.part + ((size_t)t * a.chunks + chunk) * 2;
      o[0] = acc_ll;
      o[1] = acc_sse;
    }
  }
}

// dst[t][group g][panel p][step j][lane l] = F[t][k = kp p + 4 j + (l >> 4)][column 16 g + (l & 15)], zero outside D x D: the B
// operands in the order the lanes of k_linreg_predict read them (whole k-panels, whole column groups, no predicate)
__global__ __launch_bounds__(256) void k_linreg_predict_pack(const double* __restrict__ src, double* __restrict__ dst, long long n, int d, int kp,
                                                             int np, int ng) {
  const int nk = kp >> 2;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
    const int l = (int)(e & 63);
    long long r = e >> 6;
    const int j = (int)(r % nk);
    r /= nk;
    const int p = (int)(r % np);
    r /= np;
    const int g = (int)(r % ng);
    const long long i = r / ng;
    const int k = kp * p + 4 * j + (l >> 4), c = 16 * g + (l & 15);
    dst[e] = (k < d && c < d) ? src[((size_t)i * d + k) * d + c] : 0.;
  }
}

// out_ll[t], out_sse[t]: the posterior's block partials in ascending chunk order (one thread per posterior)
__global__ __launch_bounds__(64) void k_linreg_predict_sum(const double* __restrict__ part, long long chunks, long long t, double* __restrict__ ll,
                                                           double* __restrict__ sse) {
  const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
  if (i < t) bc_predict_chunks(part + (size_t)i * chunks * 2, chunks, ll + i, sse + i);
}

// ------------------------------------------------------------------ host side
static size_t pred_lds(int d, bool wide, int nkb) {
  const int rc = wide ? 32 : 64, dp = wide ? 32 * ((d + 31) >> 5) : 16 * nkb;
  return ((size_t)rc * (dp + 4) + (size_t)rc * (2 + BC_PRED_WAVES) + dp) * sizeof(double);
}

template <int NKB, bool WIDE, typename ZT>
static int launch_one(bc_ctx* ctx, unsigned blocks, const PredictArgs& a) {
  static unsigned attr_done_mask = 0;      // (the attribute is per device: one bit per device ordinal, as k_lr_score keeps it)
  const size_t lds = pred_lds(a.d, WIDE, NKB), lds_max = pred_lds(WIDE ? BC_PRED_MAX_DIM : 16 * NKB, WIDE, NKB);
  if (lds > (size_t)ctx->max_lds) {
    bc_set_error("bc_linreg_predict: rows of %d features stage %zu bytes of LDS, the device allows %d", a.d, lds, ctx->max_lds);
    return BC_INVALID_ARGUMENT;
  }
  if (!((attr_done_mask >> (ctx->device & 31)) & 1u)) {
    BC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_linreg_predict<NKB, WIDE, ZT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)(lds_max < (size_t)ctx->max_lds ? lds_max : (size_t)ctx->max_lds)));
    attr_done_mask |= 1u << (ctx->device & 31);
  }
  hipLaunchKernelGGL((k_linreg_predict<NKB, WIDE, ZT>), dim3(blocks), dim3(BC_PRED_THREADS), lds, ctx->stream, a);
  BC_HIP(hipGetLastError());
  return BC_OK;
}

template <typename ZT>
static int launch_d(bc_ctx* ctx, unsigned blocks, const PredictArgs& a) {
  const int d = a.d;
  if (d <= 16) return launch_one<1, false, ZT>(ctx, blocks, a);
  if (d <= 32) return launch_one<2, false, ZT>(ctx, blocks, a);
  if (d <= 64) return launch_one<4, false, ZT>(ctx, blocks, a);
  if (d <= BC_PRED_PANEL) return launch_one<8, false, ZT>(ctx, blocks, a);
  return launch_one<8, true, ZT>(ctx, blocks, a);
}

// the first entry of v[n] that is not finite or lies below lo (lo_open: at or below); per: the entries of one posterior
static int refuse_entry(const char* what, const double* v, size_t n, size_t per, double lo, bool lo_open) {
  for (size_t k = 0; k < n; ++k)
    if (!std::isfinite(v[k]) || (lo_open ? v[k] <= lo : v[k] < lo)) {
      const char* why = !std::isfinite(v[k]) ? "not finite" : lo_open ? "not positive" : "negative";
      if (per > 1) bc_set_error("bc_linreg_predict: %s of posterior %zu, entry %zu = %g is %s", what, k / per, k % per, v[k], why);
      else bc_set_error("bc_linreg_predict: %s[%zu] = %g is %s", what, k, v[k], why);
      return BC_INVALID_ARGUMENT;
    }
  return BC_OK;
}

extern "C" int bc_linreg_predict(bc_ctx* ctx, const bc_data* zt, const double* mu, const double* factor, const double* noise, const double* scale,
                                 int64_t t, double* out_ll, double* out_sse, double* out_mean, double* out_var) {
  const char* missing = !ctx ? "ctx" : !zt ? "zt" : !mu ? "mu" : !factor ? "factor" : !noise ? "noise" : !scale ? "scale" : !out_ll ? "out_ll"
                        : !out_sse ? "out_sse" : nullptr;
  if (missing) { bc_set_error("bc_linreg_predict: bad argument (%s is NULL)", missing); return BC_INVALID_ARGUMENT; }
  if (!out_mean != !out_var) {
    bc_set_error("bc_linreg_predict: %s is NULL but %s is not (the per-row outputs are given together)", out_mean ? "out_var" : "out_mean",
                 out_mean ? "out_mean" : "out_var");
    return BC_INVALID_ARGUMENT;
  }
  if (zt->ctx != ctx) { bc_set_error("bc_linreg_predict: zt must live on this context"); return BC_INVALID_ARGUMENT; }
  const int d = zt->dz - 1;
  if (d < 1 || d > BC_PRED_MAX_DIM) {
    bc_set_error("bc_linreg_predict: zt must have D + 1 columns with 1 <= D <= %d, got %d columns", BC_PRED_MAX_DIM, zt->dz);
    return BC_INVALID_ARGUMENT;
  }
  const int64_t nt = zt->n_rows;
  if (nt < 1) { bc_set_error("bc_linreg_predict: zt needs at least one row, got %lld", (long long)nt); return BC_INVALID_ARGUMENT; }
  if (t < 1 || t > ((int64_t)1 << 31)) { bc_set_error("bc_linreg_predict: t must be 1 .. 2^31 posteriors, got %lld", (long long)t); return BC_INVALID_ARGUMENT; }
  const size_t T = (size_t)t, n_mu = T * d, n_f = n_mu * d;
  int rc = refuse_entry("mu", mu, n_mu, (size_t)d, -INFINITY, false);
  if (!rc) rc = refuse_entry("factor", factor, n_f, (size_t)d * d, -INFINITY, false);
  if (!rc) rc = refuse_entry("noise", noise, T, 1, 0., true);
  if (!rc) rc = refuse_entry("scale", scale, T, 1, 0., false);
  if (rc) return rc;
  rc = bc_ctx_refuse_busy(ctx, "bc_linreg_predict", BC_HOLD_HMC | BC_HOLD_HMC_SMALL);
  if (rc) return rc;
  BC_HIP(hipSetDevice(ctx->device));
  const long long chunks = (nt + BC_PRED_ROWS_PER_BLOCK - 1) / BC_PRED_ROWS_PER_BLOCK;
  if (chunks > BC_PRED_MAX_BLOCKS) { bc_set_error("bc_linreg_predict: zt has %lld rows, at most %lld are served", (long long)nt, BC_PRED_MAX_BLOCKS * BC_PRED_ROWS_PER_BLOCK); return BC_INVALID_ARGUMENT; }
  const size_t n_row = out_mean ? T * (size_t)nt : 0;
  bc_slab sl;                                                  // mu | factor | packed factor | noise | scale | partials | ll | sse | mean | var
  const int ng = BC_PRED_GROUPS(d), kp = d <= 16 ? 16 : d <= 32 ? 32 : d <= 64 ? 64 : BC_PRED_PANEL, np = (d + kp - 1) / kp;
  const size_t n_fp = T * (size_t)ng * np * kp * 16;           // (kp: the instance's k-panel, as launch_d picks it)
  const size_t o_mu = sl.take(n_mu), o_f = sl.take(n_f), o_fp = sl.take(n_fp), o_no = sl.take(T), o_sc = sl.take(T), o_part = sl.take(T * (size_t)chunks * 2),
               o_ll = sl.take(T), o_sse = sl.take(T), o_mean = sl.take(n_row), o_var = sl.take(n_row);
  rc = bc_scratch_grow(ctx, &ctx->predict, sl.total);
  if (rc) return rc;
  double* base = ctx->predict.p;
  BC_HIP(hipMemcpyAsync(base + o_mu, mu, n_mu * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  BC_HIP(hipMemcpyAsync(base + o_f, factor, n_f * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  BC_HIP(hipMemcpyAsync(base + o_no, noise, T * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  BC_HIP(hipMemcpyAsync(base + o_sc, scale, T * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  PredictArgs a;
  a.z = zt->z;
  a.mu = base + o_mu;
  a.f = base + o_fp;
  a.noise = base + o_no;
  a.scale = base + o_sc;
  a.part = base + o_part;
  a.mean = out_mean ? base + o_mean : nullptr;
  a.var = out_mean ? base + o_var : nullptr;
  a.nt = nt;
  a.chunks = chunks;
  a.d = d;
  rc = bc_timer_begin(ctx, 6);          // (timed with the class of k_lr_score)
  if (rc) return rc;
  {
    const size_t want = (n_fp + 255) / 256;
    hipLaunchKernelGGL(k_linreg_predict_pack, dim3((unsigned)(want < 4096 ? want : 4096)), dim3(256), 0, ctx->stream, base + o_f, base + o_fp,
                       (long long)n_fp, d, kp, np, ng);
    BC_HIP(hipGetLastError());
  }
  const long long per_launch = BC_PRED_MAX_BLOCKS / chunks;    // posteriors per launch (>= 1)
  for (long long t0 = 0; t0 < t; t0 += per_launch) {
    const long long tb = t - t0 < per_launch ? t - t0 : per_launch;
    a.t0 = t0;
    rc = zt->elem == 4 ? launch_d<float>(ctx, (unsigned)(tb * chunks), a) : launch_d<double>(ctx, (unsigned)(tb * chunks), a);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(k_linreg_predict_sum, dim3((unsigned)((t + 63) / 64)), dim3(64), 0, ctx->stream, a.part, chunks, (long long)t, base + o_ll,
                     base + o_sse);
  BC_HIP(hipGetLastError());
  rc = bc_timer_end(ctx, 6);
  if (rc) return rc;
  BC_HIP(hipMemcpyAsync(out_ll, base + o_ll, T * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  BC_HIP(hipMemcpyAsync(out_sse, base + o_sse, T * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (out_mean) {
    BC_HIP(hipMemcpyAsync(out_mean, base + o_mean, n_row * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    BC_HIP(hipMemcpyAsync(out_var, base + o_var, n_row * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  }
  BC_HIP(hipStreamSynchronize(ctx->stream));
  return BC_OK;
}
