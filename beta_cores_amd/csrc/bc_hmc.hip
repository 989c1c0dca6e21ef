// Multi-chain HMC of the logistic posterior of resident rows (include/beta_cores_hmc.h): the multi-chain rows pass
// k_lr_rows_mc, the per-chain update kernels around bc_hmc_dev.h, and the entry points that chain them.
//
// The rows pass.  For rows z = y*x and C parameter vectors Theta (C x D):
//
//   m_nc = -z_n . theta_c        value_c = sum_n w_n ll(m_nc)        grad_c = sum_n w_n p(m_nc) z_n
//
// with ll, p of lr_terms (bc_lr_terms.h).  K5 streams 8 D bytes per row for 4 D flops; C chains read the same rows, so one pass
// for 16 chains does 64 D flops per row for the same bytes -- work for the fp64 matrix cores.  Both contractions are
// v_mfma_f64_16x16x4_f64 over tiles of 16 rows x 16 chains (chains padded to 16 with zero columns):
//
//   M = Z_tile . Theta^T     A: lane l holds Z[row l & 15][k = 4 j + (l >> 4)], B: Theta[chain l & 15][the same k], step j
//   G += Z_tile^T . (w o P)  the result of the first product has col = lane & 15 (the chain), row = (lane >> 4) + 4 reg: register
//                            `reg` of P IS the B operand of the second product's k-block of rows 4 reg .. 4 reg + 3, so P never
//                            moves between lanes; A: lane l holds Z[row 4 reg + (l >> 4)][column 16 kb + (l & 15)]
//
// Z is needed in two layouts, so a wave stages its tile in LDS (row pitch 16 NKB + 4 doubles: both read patterns touch every
// bank pair once); the next tile's rows are already in flight in registers while the current one is worked on.  Theta of the
// block's 16 chains stays in LDS for the whole block.
//
// Work split and reduction order.  The rows are cut into RANGES of `rows_per_range` consecutive rows, a function of the row
// count and the device only.  One wave owns one (range, group of 16 chains): it walks the range's tiles in row order, and
// accumulates value and gradient in that order.  The waves of a block take consecutive ranges of the same chain group (they
// share Theta); blockIdx.y is the group.  Partials are [ranges][C][1 + D], summed over ranges in block order by k_lr_reduce.
// Nothing in a chain's chain of operations depends on C or on the chain's neighbours: its bits do not either.
#include "bc_internal.h"
#include "bc_lr_terms.h"
#include "bc_hmc_dev.h"
#include "bc_slab.h"
#include "../../include/beta_cores_hmc.h"
#include <cmath>
#include <cstring>

typedef double bc_d4 __attribute__((ext_vector_type(4)));

// The per-element terms of the pass.  The shipped build uses lr_terms: ll and p have K5's bits.  -DBC_MC_TABLE_TERMS=1 is a
// DIAGNOSTIC build that answers one question -- what would the table-driven, division-free bodies of bc_k1_math.h buy? -- and
// is not shipped: its ll and p differ from lr_terms' in the last bits (profiles/hmc_notes.md has the measurement).
#ifdef BC_MC_TABLE_TERMS
#include "bc_k1_math.h"
__device__ const unsigned long long g_mc_tab_bits[BC_K1_TAB_DOUBLES] = BC_K1_TABLE_INIT;
#define BC_MC_TAB_DOUBLES BC_K1_TAB_DOUBLES
__device__ __forceinline__ void mc_terms(double m, double& ll, double& p, const double* tab) {
  if (m < 100.) {
    double u, f;
    const double l = bc_log1p_exp_neg_tab_uf(fabs(m), tab, &u, &f);
    const double rf = bc_rcp_1_2(f);
    ll = -(fmax(m, 0.) + l);
    p = m >= 0. ? rf : u * rf;
  } else {
    ll = -m;
    p = 1.;
  }
}
#else
#define BC_MC_TAB_DOUBLES 0
__device__ __forceinline__ void mc_terms(double m, double& ll, double& p, const double*) {
  double cu;
  lr_terms(m, ll, p, cu);
}
#endif

#define BC_MC_RANGES_PER_CU 8      // ranges wanted per CU: one block of eight waves when one chain group runs

struct McArgs {
  const void* z;            // [n_rows][d] of the kernel's ZT
  const double* w;          // [n_rows] or null (all ones)
  const double* theta;      // [c][d]
  double* part;             // [n_ranges][c][1 + d]: value | grad
  long long n_rows, rows_per_range, n_ranges;
  int d, c;
};

// NKB: 16-column blocks of the gradient (D <= 16 NKB).  BC_MC_WAVES(NKB) waves, dynamic LDS (1 + waves) * 16 * (16 NKB + 4) doubles:
// eight waves (two per SIMD: a wave walks a serial chain per tile, the second wave fills its gaps) where their tiles and Theta fit
// the 160 KiB of a CU, three at D > 128 (three tiles of 260 doubles a row and Theta fill 130 KiB).
#define BC_MC_WAVES(NKB) ((NKB) == 16 ? 3 : 8)
template <int NKB, bool VALUE, typename ZT>
__global__ __launch_bounds__(64 * BC_MC_WAVES(NKB)) void k_lr_rows_mc(McArgs a) {
  extern __shared__ double mc_lds[];
  constexpr int DP = 16 * NKB, LD = DP + 4, PER = 4 * NKB;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nw = blockDim.x >> 6;
  const int d = a.d, grp = blockIdx.y;
  double* ths = mc_lds;                               // [16][LD]: Theta of this block's chains, zero-padded
  double* zs = mc_lds + (size_t)16 * LD * (1 + wv);   // [16][LD]: this wave's tile
  for (int e = tid; e < 16 * LD; e += blockDim.x) {
    const int cc = e / LD, k = e - cc * LD, ch = grp * 16 + cc;
    ths[e] = (ch < a.c && k < d) ? a.theta[(size_t)ch * d + k] : 0.;
  }
  const double* tab = mc_lds + (size_t)16 * LD * (1 + nw);      // (diagnostic build only)
#ifdef BC_MC_TABLE_TERMS
  for (int i = tid; i < BC_MC_TAB_DOUBLES; i += blockDim.x) mc_lds[(size_t)16 * LD * (1 + nw) + i] = __builtin_bit_cast(double, g_mc_tab_bits[i]);
#endif
  __syncthreads();
  const long long range = (long long)blockIdx.x * nw + wv;
  if (range >= a.n_ranges) return;                    // (no barrier below)
  const ZT* __restrict__ zrows = reinterpret_cast<const ZT*>(a.z);
  const long long start = range * a.rows_per_range;
  long long end = start + a.rows_per_range;
  if (end > a.n_rows) end = a.n_rows;
  const int r16 = lane & 15, h = lane >> 4;
  bc_d4 acc[NKB];
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb) acc[kb] = bc_d4{0., 0., 0., 0.};
  double val = 0.;
  double pf[PER], pw[4];
  // element e = 64 i + lane of the zero-padded 16 x DP tile; rows past the range's end: z = 0 with weight 0
#define BC_MC_LOAD(R0)                                                                   \
  do {                                                                                   \
    _Pragma("unroll") for (int i = 0; i < PER; ++i) {                                    \
      const int e = i * 64 + lane, row = e / DP, col = e % DP;                           \
      const long long gr = (R0) + row;                                                   \
      pf[i] = (gr < end && col < d) ? (double)zrows[(size_t)gr * d + col] : 0.;          \
    }                                                                                    \
    _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                      \
      const long long gr = (R0) + 4 * q + h;                                             \
      pw[q] = gr < end ? (a.w ? a.w[gr] : 1.) : 0.;                                      \
    }                                                                                    \
  } while (0)
  BC_MC_LOAD(start);
  const int nk = (d + 3) >> 2;
  const double* za = zs + r16 * LD + h;
  const double* tb = ths + r16 * LD + h;
  for (long long r0 = start; r0 < end; r0 += 16) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int e = i * 64 + lane;
      zs[(e / DP) * LD + (e % DP)] = pf[i];
    }
    double wq[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) wq[q] = pw[q];
    // the tile is written and read by this wave only: LDS serves a wave's requests in order, the fence orders the compiler
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (r0 + 16 < end) BC_MC_LOAD(r0 + 16);           // (wave-uniform)
    bc_d4 m4 = bc_d4{0., 0., 0., 0.};
    for (int j = 0; j < nk; ++j) m4 = __builtin_amdgcn_mfma_f64_16x16x4f64(za[4 * j], tb[4 * j], m4, 0, 0, 0);
    double wp[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      double ll, p;
      mc_terms(-m4[q], ll, p, tab);
      wp[q] = wq[q] * p;
      if (VALUE) val = fma(wq[q], ll, val);
    }
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        acc[kb] = __builtin_amdgcn_mfma_f64_16x16x4f64(zs[(4 * q + h) * LD + kb * 16 + r16], wp[q], acc[kb], 0, 0, 0);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
#undef BC_MC_LOAD
  if (VALUE) {      // rows 4 q + h of every tile went to lane group h: (h0 + h1) + (h2 + h3), the same bits in all four
    val += __shfl_xor(val, 16, BC_WAVE);
    val += __shfl_xor(val, 32, BC_WAVE);
  }
  const int ch = grp * 16 + r16;
  if (ch < a.c) {
    double* out = a.part + ((size_t)range * a.c + ch) * (size_t)(1 + d);
    if (h == 0) out[0] = val;
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int k = kb * 16 + h + 4 * reg;
        if (k < d) out[1 + k] = acc[kb][reg];
      }
    }
  }
}

// ------------------------------------------------------------------ the per-chain update kernels (one block per chain)
#define BC_HMC_BLOCK 256

struct HmcState {
  int c, d;
  double half_d_log_2pi;
  double *theta, *thp, *r, *g, *gp;      // [c][d]: position, proposal, momentum, gradient, the proposal's gradient
  double *lj, *ljp, *h0;                 // [c]: log-joint, the proposal's, H0
  double* red;                           // [c][1 + d]: the rows pass, reduced
  const double* im;                      // [d]
};

// the log-joint and gradient at the start; a chain whose are not finite marks the run
__global__ __launch_bounds__(BC_HMC_BLOCK) void k_hmc_init(HmcState s, int* __restrict__ flag) {
  __shared__ double ws[BC_HMC_WS_DOUBLES(BC_HMC_MAX_DIM)];
  const int ch = blockIdx.x;
  const size_t o = (size_t)ch * s.d;
  if (bc_hmc_logjoint_chain(s.red + (size_t)ch * (1 + s.d), s.theta + o, s.d, s.half_d_log_2pi, s.lj + ch, s.g + o, ws) && threadIdx.x == 0)
    *flag = 1;
}

__global__ __launch_bounds__(BC_HMC_BLOCK) void k_hmc_start(HmcState s, const int* __restrict__ flag, const double* __restrict__ e, double eps) {
  __shared__ double ws[BC_HMC_WS_DOUBLES(BC_HMC_MAX_DIM)];
  if (*(volatile const int*)flag != 0) return;      // (block-uniform)
  const int ch = blockIdx.x;
  const size_t o = (size_t)ch * s.d;
  bc_hmc_start_chain(s.theta + o, s.lj + ch, s.g + o, e + o, s.im, eps, s.d, s.r + o, s.thp + o, s.h0 + ch, ws);
}

__global__ __launch_bounds__(BC_HMC_BLOCK) void k_hmc_inner(HmcState s, const int* __restrict__ flag, double eps) {
  if (*(volatile const int*)flag != 0) return;
  const int ch = blockIdx.x;
  const size_t o = (size_t)ch * s.d;
  bc_hmc_inner_chain(s.red + (size_t)ch * (1 + s.d), eps, s.im, s.d, s.r + o, s.thp + o);
}

// out_*: this iteration's slices: samples [c][d], log-joints [c], accept flags [c]
__global__ __launch_bounds__(BC_HMC_BLOCK) void k_hmc_last(HmcState s, const int* __restrict__ flag, double eps, const double* __restrict__ logu,
                                                           double* __restrict__ out_samples, double* __restrict__ out_lj, int* __restrict__ out_acc) {
  __shared__ double ws[BC_HMC_WS_DOUBLES(BC_HMC_MAX_DIM)];
  if (*(volatile const int*)flag != 0) return;
  const int ch = blockIdx.x;
  const size_t o = (size_t)ch * s.d;
  const int acc = bc_hmc_last_chain(s.red + (size_t)ch * (1 + s.d), eps, s.im, s.d, s.half_d_log_2pi, s.h0 + ch, logu[ch], s.r + o, s.thp + o,
                                    s.gp + o, s.ljp + ch, s.theta + o, s.lj + ch, s.g + o, ws);
  for (int k = threadIdx.x; k < s.d; k += blockDim.x) out_samples[o + k] = s.theta[o + k];      // (element k: written by this thread, if at all)
  if (threadIdx.x == 0) {
    out_lj[ch] = s.lj[ch];
    out_acc[ch] = acc;
  }
}

// ------------------------------------------------------------------ host side
static const bc_run_kind HMC_RUN = {"bc_hmc", "iterations"};
struct bc_hmc : bc_run {          // (the run in progress: active, chunk_pending, failed, done of total iterations, the clock)
  bc_scratch dev;                 // the chains' state (HmcState) | inverse mass | flag
  bc_scratch part;                // the rows pass's partials
  bc_stage stage;                 // a chunk's draws: normals [k][c][d] | log-uniforms [k][c]
  bc_scratch out;                 // a chunk's results: samples [k][c][d] | log-joints [k][c] | accept flags [k][c] (ints)
  const bc_data* data = nullptr;
  const bc_data* w = nullptr;
  HmcState st;
  int* d_flag = nullptr;
  int32_t n_leapfrog = 0, pending_k = 0;
  size_t o_l = 0, o_a = 0;        // where the pending chunk's log-joints and accept flags begin in `out` (set by _chunk_begin)
};

bool bc_hmc_active(const bc_ctx* ctx) { return ctx->hmc && ctx->hmc->active; }

void bc_hmc_free(bc_ctx* ctx) {
  bc_hmc* h = ctx->hmc;
  if (!h) return;
  bc_scratch_free(&h->dev);
  bc_scratch_free(&h->part);
  bc_stage_free(&h->stage);
  bc_scratch_free(&h->out);
  h->clock.free();
  delete h;
  ctx->hmc = nullptr;
}

static int nkb_of(int d) { return d <= 16 ? 1 : d <= 32 ? 2 : d <= 64 ? 4 : d <= 128 ? 8 : 16; }
static int waves_of(int nkb) { return BC_MC_WAVES(nkb); }
static size_t lds_of(int nkb) { return ((size_t)(1 + waves_of(nkb)) * 16 * (16 * nkb + 4) + BC_MC_TAB_DOUBLES) * sizeof(double); }

// the ranges: a function of the row count and the device only (never of the chain count)
static long long ranges_of(const bc_ctx* ctx, long long n, long long* rows_per_range) {
  const long long want = (long long)ctx->n_cu * BC_MC_RANGES_PER_CU;
  long long r = (n + want - 1) / want;
  r = ((r + 15) / 16) * 16;
  if (r < 16) r = 16;
  *rows_per_range = r;
  return (n + r - 1) / r;
}

template <int NKB, bool VALUE, typename ZT>
static int launch_mc_one(bc_ctx* ctx, dim3 grid, const McArgs& a) {
  static unsigned attr_done_mask = 0;      // (the attribute is per device: one bit per device ordinal, as K1 / K4 keep it)
  const size_t lds = lds_of(NKB);
  if (!((attr_done_mask >> (ctx->device & 31)) & 1u)) {
    BC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_lr_rows_mc<NKB, VALUE, ZT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)lds));
    attr_done_mask |= 1u << (ctx->device & 31);
  }
  hipLaunchKernelGGL((k_lr_rows_mc<NKB, VALUE, ZT>), grid, dim3(64 * waves_of(NKB)), lds, ctx->stream, a);
  BC_HIP(hipGetLastError());
  return BC_OK;
}

template <int NKB>
static int launch_mc(bc_ctx* ctx, bool value, bool f32, dim3 grid, const McArgs& a) {
  if (f32) return value ? launch_mc_one<NKB, true, float>(ctx, grid, a) : launch_mc_one<NKB, false, float>(ctx, grid, a);
  return value ? launch_mc_one<NKB, true, double>(ctx, grid, a) : launch_mc_one<NKB, false, double>(ctx, grid, a);
}

// red[c][1 + d] = the likelihood's value (0 unless `value`) and gradient at theta_dev [c][d]; enqueued only.
// part must hold ranges * c * (1 + d) doubles.
static int rows_pass(bc_ctx* ctx, const bc_data* data, const bc_data* w, const double* theta_dev, int c, bool value, double* part,
                     double* red) {
  const int d = data->dz;
  const long long n = data->n_rows;
  const int elems = c * (1 + d);
  if (n == 0) {
    BC_HIP(hipMemsetAsync(red, 0, (size_t)elems * sizeof(double), ctx->stream));
    return BC_OK;
  }
  McArgs a;
  a.z = data->z;
  a.w = w ? w->z : nullptr;
  a.theta = theta_dev;
  a.part = part;
  a.n_rows = n;
  a.n_ranges = ranges_of(ctx, n, &a.rows_per_range);
  a.d = d;
  a.c = c;
  const int nkb = nkb_of(d), nw = waves_of(nkb);
  const dim3 grid((unsigned)((a.n_ranges + nw - 1) / nw), (unsigned)((c + 15) / 16));
  const bool f32 = data->elem == 4;
  int rc = bc_timer_begin(ctx, 6);      // (timed with K5's class: the logistic rows pass + its reduction)
  if (rc) return rc;
  switch (nkb) {
    case 1: rc = launch_mc<1>(ctx, value, f32, grid, a); break;
    case 2: rc = launch_mc<2>(ctx, value, f32, grid, a); break;
    case 4: rc = launch_mc<4>(ctx, value, f32, grid, a); break;
    case 8: rc = launch_mc<8>(ctx, value, f32, grid, a); break;
    default: rc = launch_mc<16>(ctx, value, f32, grid, a); break;
  }
  if (!rc) rc = bc_lr_reduce_launch(ctx, part, a.n_ranges, elems, red);
  const int rc_timer = bc_timer_end(ctx, 6);      // (after a failed launch too: the timer must not stay armed)
  return rc ? rc : rc_timer;
}

static int check_problem(bc_ctx* ctx, const bc_data* data, const bc_data* w, int32_t c, const char* who) {
  if (data->ctx != ctx || (w && w->ctx != ctx)) BC_REFUSE("%s: rows or weights belong to another context", who);
  if (c < 1 || c > BC_HMC_MAX_CHAINS) BC_REFUSE("%s: 1 .. %d chains are served, got %d", who, BC_HMC_MAX_CHAINS, c);
  const int d = data->dz;
  if (d < 1 || d > BC_HMC_MAX_DIM) BC_REFUSE("%s: rows must have 1 .. %d columns, got %d", who, BC_HMC_MAX_DIM, d);
  if (w && (w->dz != 1 || w->n_rows != data->n_rows))
    BC_REFUSE("%s: weights must be %lld x 1, got %lld x %d", who, (long long)data->n_rows, (long long)w->n_rows, w->dz);
  if (w && bc_refuse_f32(w, who)) return BC_INVALID_ARGUMENT;
  if (lds_of(nkb_of(d)) > (size_t)ctx->max_lds)
    BC_REFUSE("%s: D = %d needs %zu bytes of LDS, the device offers %d", who, d, lds_of(nkb_of(d)), ctx->max_lds);
  return BC_OK;
}

// lays the state slab out for c chains of d coordinates (growing it if need be) and points h->st into it
static int layout_state(bc_ctx* ctx, bc_hmc* h, const bc_data* data, int c) {
  const int d = data->dz;
  const size_t cd = (size_t)c * d;
  bc_slab sl;
  const size_t o_theta = sl.take(cd), o_thp = sl.take(cd), o_r = sl.take(cd), o_g = sl.take(cd), o_gp = sl.take(cd);
  const size_t o_lj = sl.take(c), o_ljp = sl.take(c), o_h0 = sl.take(c), o_red = sl.take((size_t)c * (1 + d)), o_im = sl.take(d);
  const size_t o_flag = sl.take(2);      // (two doubles: the flag ints)
  int rc = bc_scratch_grow(ctx, &h->dev, sl.total);
  long long rpr = 0;
  const long long ranges = data->n_rows > 0 ? ranges_of(ctx, data->n_rows, &rpr) : 0;
  if (!rc) rc = bc_scratch_grow(ctx, &h->part, (size_t)ranges * c * (1 + d) + 2);
  if (rc) return rc;
  HmcState& s = h->st;
  s.c = c;
  s.d = d;
  s.half_d_log_2pi = 0.5 * d * log(2. * M_PI);
  double* p = h->dev.p;
  s.theta = p + o_theta;
  s.thp = p + o_thp;
  s.r = p + o_r;
  s.g = p + o_g;
  s.gp = p + o_gp;
  s.lj = p + o_lj;
  s.ljp = p + o_ljp;
  s.h0 = p + o_h0;
  s.red = p + o_red;
  s.im = p + o_im;
  h->d_flag = reinterpret_cast<int*>(p + o_flag);
  return BC_OK;
}

static bc_hmc* hmc_of(bc_ctx* ctx) {
  if (!ctx->hmc) ctx->hmc = new bc_hmc();
  return ctx->hmc;
}

extern "C" int bc_logistic_logjoint_batch(bc_ctx* ctx, const bc_data* data, const bc_data* w, const double* theta, int32_t c,
                                          double* out_value, double* out_grad) {
  if (!ctx || !data || !theta || !out_grad)
    BC_REFUSE("bc_logistic_logjoint_batch: bad argument (context, rows, theta and gradients are required)");
  int rc = check_problem(ctx, data, w, c, "bc_logistic_logjoint_batch");
  if (rc) return rc;
  rc = bc_ctx_refuse_busy(ctx, "bc_logistic_logjoint_batch", BC_HOLD_HMC | BC_HOLD_HMC_SMALL);
  if (rc) return rc;
  BC_HIP(hipSetDevice(ctx->device));
  bc_hmc* h = hmc_of(ctx);
  rc = layout_state(ctx, h, data, c);
  if (rc) return rc;
  const int d = data->dz;
  const size_t n_th = (size_t)c * d;
  BC_HIP(hipMemcpyAsync(h->st.theta, theta, n_th * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  BC_HIP(hipMemsetAsync(h->d_flag, 0, 2 * sizeof(int), ctx->stream));
  rc = rows_pass(ctx, data, w, h->st.theta, c, out_value != nullptr, h->part.p, h->st.red);
  if (rc) return rc;
  hipLaunchKernelGGL(k_hmc_init, dim3((unsigned)c), dim3(BC_HMC_BLOCK), 0, ctx->stream, h->st, h->d_flag);
  BC_HIP(hipGetLastError());
  if (out_value) BC_HIP(hipMemcpyAsync(out_value, h->st.lj, (size_t)c * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  BC_HIP(hipMemcpyAsync(out_grad, h->st.g, n_th * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  BC_HIP(hipStreamSynchronize(ctx->stream));
  return BC_OK;
}

extern "C" int bc_hmc_auto_chunk(int32_t c, int32_t d) {
  if (c <= 0 || d <= 0) return 1;
  const double per_iter = 8. * ((double)c * (double)d + (double)c);
  const double k = floor((double)BC_HMC_STAGE_BYTES / per_iter);
  return k < 1. ? 1 : k > 1048576. ? 1048576 : (int)k;
}

extern "C" int bc_hmc_begin(bc_ctx* ctx, const bc_data* data, const bc_data* w, const double* start, int32_t c, const double* inv_mass,
                            int32_t n_leapfrog, int64_t n_iter) {
  if (!ctx || !data || !start || !inv_mass) BC_REFUSE("bc_hmc_begin: bad argument (context, rows, start and inv_mass are required)");
  int rc = check_problem(ctx, data, w, c, "bc_hmc_begin");
  if (rc) return rc;
  if (n_leapfrog < 1 || n_iter < 1)
    BC_REFUSE("bc_hmc_begin: needs n_leapfrog >= 1 and n_iter >= 1 (n_leapfrog = %d, n_iter = %lld)", n_leapfrog, (long long)n_iter);
  const int d = data->dz;
  for (int k = 0; k < d; ++k)
    if (!(inv_mass[k] > 0.) || !std::isfinite(inv_mass[k]))
      BC_REFUSE("bc_hmc_begin: inv_mass[%d] = %g is not finite and positive", k, inv_mass[k]);
  rc = bc_ctx_refuse_busy(ctx, "bc_hmc_begin", BC_HOLD_ALL, BC_HOLD_HMC);
  if (rc) return rc;
  BC_HIP(hipSetDevice(ctx->device));
  bc_hmc* h = hmc_of(ctx);
  rc = h->clock.create();
  if (!rc) rc = layout_state(ctx, h, data, c);
  if (rc) return rc;
  BC_HIP(hipStreamSynchronize(ctx->stream));
  // (pageable sources: the copies below have read them when they return)
  BC_HIP(hipMemcpyAsync(h->st.theta, start, (size_t)c * d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  BC_HIP(hipMemcpyAsync(const_cast<double*>(h->st.im), inv_mass, (size_t)d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  BC_HIP(hipMemsetAsync(h->d_flag, 0, 2 * sizeof(int), ctx->stream));
  rc = rows_pass(ctx, data, w, h->st.theta, c, true, h->part.p, h->st.red);
  if (rc) return rc;
  hipLaunchKernelGGL(k_hmc_init, dim3((unsigned)c), dim3(BC_HMC_BLOCK), 0, ctx->stream, h->st, h->d_flag);
  BC_HIP(hipGetLastError());
  h->data = data;
  h->w = w;
  h->n_leapfrog = n_leapfrog;
  h->pending_k = 0;
  bc_run_opened(h, n_iter);
  return BC_OK;
}

extern "C" int bc_hmc_chunk_begin(bc_ctx* ctx, const double* normals, const double* log_u, int32_t k, double step_size) {
  bc_hmc* h = ctx ? ctx->hmc : nullptr;
  int rc = bc_run_admit(h, HMC_RUN, normals && log_u, k);
  if (rc) return rc;
  if (!(step_size > 0.) || !std::isfinite(step_size)) BC_REFUSE("bc_hmc_chunk_begin: the step size must be finite and positive, got %g", step_size);
  // ---- nothing of this chunk has been enqueued up to here
  BC_HIP(hipSetDevice(ctx->device));
  const HmcState& s = h->st;
  const size_t cd = (size_t)s.c * s.d, n_e = (size_t)k * cd, n_u = (size_t)k * s.c;
  bc_slab st, out;
  st.take(n_e);
  const size_t o_u = st.take(n_u);
  out.take(n_e);
  h->o_l = out.take(n_u);
  h->o_a = out.take((n_u + 1) / 2);      // (ints)
  rc = bc_stage_reserve(ctx, &h->stage, st.total);
  if (!rc) rc = bc_scratch_grow(ctx, &h->out, out.total);
  if (rc) return rc;
  memcpy(h->stage.pin.p, normals, n_e * sizeof(double));
  memcpy(h->stage.pin.p + o_u, log_u, n_u * sizeof(double));
  BC_HIP(hipMemcpyAsync(h->stage.dev.p, h->stage.pin.p, st.total * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  rc = h->clock.start(ctx->stream);
  if (rc) return rc;
  h->chunk_pending = true;      // from here on something is enqueued: _chunk_end must wait even if a launch below fails
  h->pending_k = k;
  const double* d_e = h->stage.dev.p;
  const double* d_u = h->stage.dev.p + o_u;
  double* o_s = h->out.p;
  double* o_l = h->out.p + h->o_l;
  int* o_a = reinterpret_cast<int*>(h->out.p + h->o_a);
  for (int t = 0; t < k; ++t) {
    hipLaunchKernelGGL(k_hmc_start, dim3((unsigned)s.c), dim3(BC_HMC_BLOCK), 0, ctx->stream, s, h->d_flag, d_e + (size_t)t * cd, step_size);
    BC_HIP(hipGetLastError());
    for (int l = 1; l <= h->n_leapfrog; ++l) {
      const bool last = l == h->n_leapfrog;
      rc = rows_pass(ctx, h->data, h->w, s.thp, s.c, last, h->part.p, s.red);
      if (rc) return rc;
      if (!last) hipLaunchKernelGGL(k_hmc_inner, dim3((unsigned)s.c), dim3(BC_HMC_BLOCK), 0, ctx->stream, s, h->d_flag, step_size);
      else
        hipLaunchKernelGGL(k_hmc_last, dim3((unsigned)s.c), dim3(BC_HMC_BLOCK), 0, ctx->stream, s, h->d_flag, step_size, d_u + (size_t)t * s.c, o_s + (size_t)t * cd,
                           o_l + (size_t)t * s.c, o_a + (size_t)t * s.c);
      BC_HIP(hipGetLastError());
    }
  }
  rc = h->clock.stop(ctx->stream);
  if (rc) return rc;
  h->done += k;
  return BC_OK;
}

extern "C" int bc_hmc_chunk_end(bc_ctx* ctx, double* out_samples, double* out_logjoint, int32_t* out_accept) {
  bc_hmc* h = ctx ? ctx->hmc : nullptr;
  int rc = bc_run_pending(h, "bc_hmc_chunk_end");
  if (rc) return rc;
  // (checked first: the chunk stays pending, a second call with the outputs can still fetch it)
  if (!out_samples || !out_logjoint || !out_accept) BC_REFUSE("bc_hmc_chunk_end: the three outputs are required");
  rc = bc_run_wait_chunk(ctx, h);
  if (rc) return rc;
  int flag = 0;
  BC_HIP(hipMemcpy(&flag, h->d_flag, sizeof(int), hipMemcpyDeviceToHost));
  if (flag != 0) {
    h->failed = true;
    bc_set_error("bc_hmc: the log-joint or its gradient at a chain's start is not finite (a weight or a start point that is not finite)");
    return BC_NUMERICAL_PRECISION;
  }
  const HmcState& s = h->st;
  const size_t n_u = (size_t)h->pending_k * s.c;
  BC_HIP(hipMemcpy(out_samples, h->out.p, n_u * s.d * sizeof(double), hipMemcpyDeviceToHost));
  BC_HIP(hipMemcpy(out_logjoint, h->out.p + h->o_l, n_u * sizeof(double), hipMemcpyDeviceToHost));
  BC_HIP(hipMemcpy(out_accept, h->out.p + h->o_a, n_u * sizeof(int32_t), hipMemcpyDeviceToHost));
  return BC_OK;
}

extern "C" int bc_hmc_end(bc_ctx* ctx) {
  bc_hmc* h = ctx ? ctx->hmc : nullptr;
  bool pending = false;
  const int rc = bc_run_end(ctx, h, HMC_RUN, &pending);
  if (rc) return rc;
  h->data = h->w = nullptr;
  return BC_OK;
}

extern "C" int bc_hmc_device_ms(bc_ctx* ctx, double* out_ms) {
  return bc_device_ms("bc_hmc_device_ms", ctx, ctx && ctx->hmc ? &ctx->hmc->clock : nullptr, out_ms);
}

extern "C" int bc_hmc_logistic(bc_ctx* ctx, const bc_data* data, const bc_data* w, const double* start, int32_t c, const double* inv_mass,
                               int32_t n_leapfrog, double step_size, int64_t n_iter, const double* normals, const double* log_u,
                               int32_t chunk_steps, double* out_samples, double* out_logjoint, int32_t* out_accept) {
  if (!normals || !log_u || !out_samples || !out_logjoint || !out_accept || chunk_steps < 0) BC_REFUSE("bc_hmc_logistic: bad argument");
  int rc = bc_hmc_begin(ctx, data, w, start, c, inv_mass, n_leapfrog, n_iter);
  if (rc) return rc;
  const int d = data->dz;
  const int64_t chunk = chunk_steps > 0 ? chunk_steps : bc_hmc_auto_chunk(c, d);
  for (int64_t i0 = 0; i0 < n_iter && !rc; i0 += chunk) {
    const int32_t k = (int32_t)(n_iter - i0 < chunk ? n_iter - i0 : chunk);
    rc = bc_hmc_chunk_begin(ctx, normals + (size_t)i0 * c * d, log_u + (size_t)i0 * c, k, step_size);
    if (ctx->hmc->chunk_pending) {
      const int rc2 = bc_hmc_chunk_end(ctx, out_samples + (size_t)i0 * c * d, out_logjoint + (size_t)i0 * c, out_accept + (size_t)i0 * c);
      if (!rc) rc = rc2;
    }
  }
  if (rc) return bc_close_failed_run(rc, [&] { return bc_hmc_end(ctx); });
  return bc_hmc_end(ctx);
}
