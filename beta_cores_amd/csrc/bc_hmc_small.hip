// Batched HMC of many small logistic posteriors (include/beta_cores_hmc_small.h): a thread block holds ONE problem's rows in LDS
// and runs a whole chunk of iterations of its chains there -- momentum draw, every leapfrog step with its rows pass, the accept
// step -- without returning to global memory in between.
//
// k_hmc_small, one launch per chunk.  A block serves one problem and CPB of its chains (1, 2 or 4: a divisor of C); each chain is
// worked by its own BC_SM_BLOCK threads (a "slot"), the slots share the rows and the weights.  Grid = P * C / CPB blocks of
// CPB * BC_SM_BLOCK threads, dynamic LDS = the largest problem's need:
//
//   rows [n][ld] | w [n] || per slot: w p [n] | ll [n] | part [nseg][1 + D] | theta g theta' r g' im [6][D] | red [1 + D] |
//                                     ws [2 D + 2] | lj lj' H0 -
//
// The rows pass is bc_hmc_small_rows_pass (bc_hmc_small_dev.h: row stride, bank behaviour and summation order are described
// there); the leapfrog and accept arithmetic is bc_hmc_dev.h's, unchanged, with `red` and the work space in LDS: both headers
// are compiled here with BC_HMC_TID / BC_HMC_NT = the thread's index within its slot / BC_SM_BLOCK, and BC_HMC_SYNC the block's
// barrier (the slots of a block run the same sequence of barriers: trip counts depend on the chunk only, and the accept branch
// holds none).  A chain's arithmetic is the same text for every CPB, so its bits do not depend on how chains are packed.
// Blocks never wait for each other: no flags between blocks, no cooperative launch; a block whose problem was marked at the
// start returns at once.  At these sizes a leapfrog step is a few dependent LDS round trips and barriers, not flops, so the fp64
// VALU serves it; packing chains buys occupancy where one problem's rows fill most of a CU's LDS (at D = 128 one block per CU:
// four waves on four SIMDs with nothing to hide a barrier or an LDS round trip behind; with four chains, sixteen).
//
// The same kernel serves the start pass (mode BC_SM_INIT: log-joint and gradient at the start, marks a problem whose are not
// finite) and the pass on its own (BC_SM_PASS: bc_hmc_small_logjoint, the test seam).
//
// The per-chain warm-up (include/beta_cores_hmc_adapt.h) is the instantiation AD = 1 of the same kernel; the instantiations
// AD = 0 are the text they were.  There a chain reads its OWN inverse mass and step: the scalars of bc_hmc_adapt_dev.h stay in
// registers of thread 0 of the slot, the step of the next iteration is handed to the slot through the fourth scalar of the
// chain's LDS state (unused otherwise), and the running mean and M2 of the window live in global memory, element k touched by
// thread k alone, once per iteration.  The flags and coefficients of an iteration come from the plan, the same for every chain,
// so the one barrier the stage adds per iteration is block-uniform; the LDS layout and the capacity rule are unchanged.  With
// a.plan = null the launch is a chunk of kept iterations at the chains' frozen steps and masses.
#define BC_SM_BLOCK 256
#define BC_HMC_FN __device__
#define BC_HMC_TID ((int)(threadIdx.x & (BC_SM_BLOCK - 1)))
#define BC_HMC_NT BC_SM_BLOCK
#define BC_HMC_SYNC() do { __threadfence_block(); __syncthreads(); } while (0)
#include "bc_internal.h"
#include "bc_hmc_dev.h"
#include "bc_hmc_small_dev.h"
#include "bc_hmc_adapt_dev.h"
#include "bc_hmc_adapt_plan.h"
#include "bc_slab.h"
#include "bc_batch.h"
#include "bc_diag.h"
#include "../../include/beta_cores_hmc_small.h"
#include "../../include/beta_cores_score.h"
#include "../../include/beta_cores_hmc_adapt.h"
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#define BC_SM_INIT 0
#define BC_SM_CHUNK 1
#define BC_SM_PASS 2
// the doubles of LDS a chain's state needs (the capacity rule is lds_doubles below)
#define BC_SM_STATE_DOUBLES(d) (6 * (size_t)(d) + (1 + (size_t)(d)) + BC_HMC_WS_DOUBLES((size_t)(d)) + 4)

struct SmArgs {
  const double* rows;           // packed rows [sum n][d]
  const double* w;              // [sum n]
  const long long* row_ptr;     // [P + 1]
  double *theta, *g, *lj;       // the chains' state: [P * C][d], [P * C][d], [P * C]
  const double* im;             // [P][d]
  const double* step;           // [P]
  int* flag;                    // [P]: 1 = the problem's start is not finite
  const double* e;              // the chunk's normals
  const double* logu;           // the chunk's log-uniforms
  long long e_stride, u_stride; // per problem (0: shared)
  double* out_s;                // [P][k][C][d]
  double* out_l;                // [P][k][C]
  int* out_a;                   // [P][k][C]
  double half_d_log_2pi;
  int d, c, k, n_leapfrog, mode, value;
  // ---- the per-chain warm-up (AD = 1 only)
  double* ad_st;                // [P * C][BC_HMC_ADAPT_STATE]
  double* ad_im;                // [P * C][d]: the chains' own inverse masses
  double *ad_mean, *ad_m2;      // [P * C][d]: the window's running mean and M2
  const double* plan;           // the chunk's [k][4] = eta | sg | zeta | flags, or null: kept iterations at the frozen state
  double *out_step, *out_alpha; // [P][k][C]
  double delta, log10;
};

template <int CPB, int AD = 0>
__global__ __launch_bounds__(CPB * BC_SM_BLOCK) void k_hmc_small(SmArgs a) {
  extern __shared__ double sm_lds[];
  const int tid = BC_HMC_TID, nt = BC_HMC_NT, slot = threadIdx.x / BC_SM_BLOCK;
  const int groups = a.c / CPB, p = blockIdx.x / groups, ch = (blockIdx.x - p * groups) * CPB + slot;
  const int bid = p * a.c + ch;                        // the chain's index in the state and the outputs
  if (a.mode == BC_SM_CHUNK && a.flag[p] != 0) return;      // (block-uniform; written by an earlier launch)
  const int d = a.d, ld = BC_HMC_SMALL_LD(d);
  const long long r0 = a.row_ptr[p];
  const int n = (int)(a.row_ptr[p + 1] - r0);
  double* zs = sm_lds;
  double* w = zs + (size_t)n * ld;
  double* wp = w + n + (size_t)slot * (BC_HMC_SMALL_CHAIN_DOUBLES(n, d) + BC_SM_STATE_DOUBLES(d));
  double* ll = wp + n;
  double* part = ll + n;
  double* th = part + (size_t)BC_HMC_SMALL_NSEG(n) * (d + 1);
  double* g = th + d;
  double* thp = g + d;
  double* r = thp + d;
  double* gp = r + d;
  double* im = gp + d;
  double* red = im + d;
  double* ws = red + 1 + d;
  double* sc = ws + BC_HMC_WS_DOUBLES(d);      // lj | lj' | H0
  const double* __restrict__ src = a.rows + (size_t)r0 * d;
  for (int e = threadIdx.x; e < n * d; e += blockDim.x) {      // (the rows and the weights: filled by all slots together)
    const int i = e / d, k = e - i * d;
    zs[(size_t)i * ld + k] = src[e];
  }
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    if (ld > d) zs[(size_t)i * ld + d] = 0.;
    w[i] = a.w[r0 + i];
  }
  const size_t o = (size_t)bid * d;
  for (int k = tid; k < d; k += nt) {
    th[k] = a.theta[o + k];
    if (a.mode == BC_SM_CHUNK) {
      g[k] = a.g[o + k];
      im[k] = AD ? a.ad_im[o + k] : a.im[(size_t)p * d + k];
    }
  }
  if (tid == 0) {
    red[0] = 0.;
    sc[0] = a.mode == BC_SM_CHUNK ? a.lj[bid] : 0.;
  }
  bc_hmc_adapt_scalars st = {0., 0., 0., 0., 0., 0.};      // thread 0's; t and nw, which follow the plan, in every thread
  if (AD) {
    const double* sg = a.ad_st + (size_t)bid * BC_HMC_ADAPT_STATE;
    st.x = sg[0], st.xbar = sg[1], st.hbar = sg[2], st.mu = sg[3], st.t = sg[4], st.nw = sg[5];
    if (tid == 0) sc[3] = bc_hmc_adapt_exp(a.plan ? st.x : bc_hmc_adapt_frozen_log_step(st.x, st.xbar, st.t));
  }
  BC_HMC_SYNC();
  if (a.mode != BC_SM_CHUNK) {
    bc_hmc_small_rows_pass(zs, w, n, d, th, a.value, wp, ll, part, red);
    const int bad = bc_hmc_logjoint_chain(red, th, d, a.half_d_log_2pi, sc, g, ws);
    for (int k = tid; k < d; k += nt) a.g[o + k] = g[k];      // (element k: written by this thread)
    if (tid == 0) {
      a.lj[bid] = sc[0];
      if (bad && a.mode == BC_SM_INIT) a.flag[p] = 1;      // (every chain of the problem that finds it writes the same 1)
    }
    return;
  }
  double eps = AD ? sc[3] : a.step[p];
  const double* __restrict__ en = a.e + (size_t)p * a.e_stride;
  const double* __restrict__ un = a.logu + (size_t)p * a.u_stride;
  const size_t ob = (size_t)p * a.k * a.c;
  for (int t = 0; t < a.k; ++t) {
    const size_t tc = (size_t)t * a.c + ch;
    bc_hmc_start_chain(th, sc, g, en + tc * d, im, eps, d, r, thp, sc + 2, ws);
    for (int l = 1; l <= a.n_leapfrog; ++l) {
      const bool last = l == a.n_leapfrog;
      bc_hmc_small_rows_pass(zs, w, n, d, thp, last ? 1 : 0, wp, ll, part, red);
      if (!last) {
        bc_hmc_inner_chain(red, eps, im, d, r, thp);
        BC_HMC_SYNC();
      }
    }
    const int acc = bc_hmc_last_chain(red, eps, im, d, a.half_d_log_2pi, sc + 2, un[tc], r, thp, gp, sc + 1, th, sc, g, ws);
    for (int k = tid; k < d; k += nt) a.out_s[(ob + tc) * d + k] = th[k];
    if (tid == 0) {
      a.out_l[ob + tc] = sc[0];
      a.out_a[ob + tc] = acc;
    }
    if (AD && a.plan) {      // the adaptation stage (block-uniform: the plan and the chunk decide)
      const double* pl = a.plan + 4 * (size_t)t;
      const int fl = (int)pl[3];
      st.t += 1.;
      if (tid == 0) {
        const double alpha = bc_hmc_adapt_alpha(ws[2 * d + 1]);
        a.out_step[ob + tc] = eps;
        a.out_alpha[ob + tc] = alpha;
        bc_hmc_adapt_step_size(alpha, a.delta, pl[0], pl[1], pl[2], &st);
      }
      if (fl & BC_HMC_ADAPT_FOLD) {
        st.nw += 1.;
        bc_hmc_adapt_fold(th, d, st.nw, a.ad_mean + o, a.ad_m2 + o);
      }
      if (fl & BC_HMC_ADAPT_WEND) {
        bc_hmc_adapt_window_end(d, st.nw, a.ad_mean + o, a.ad_m2 + o, im);
        st.t = st.nw = 0.;
        if (tid == 0) bc_hmc_adapt_restart(a.log10, &st);
      }
      if (tid == 0) sc[3] = bc_hmc_adapt_exp(st.x);
      BC_HMC_SYNC();      // (the next step and a new inverse mass are read by the whole slot)
      eps = sc[3];
    }
  }
  for (int k = tid; k < d; k += nt) {
    a.theta[o + k] = th[k];
    a.g[o + k] = g[k];
    if (AD && a.plan) a.ad_im[o + k] = im[k];
  }
  if (tid == 0) {
    a.lj[bid] = sc[0];
    if (AD && a.plan) {
      double* sg = a.ad_st + (size_t)bid * BC_HMC_ADAPT_STATE;
      sg[0] = st.x, sg[1] = st.xbar, sg[2] = st.hbar, sg[3] = st.mu, sg[4] = st.t, sg[5] = st.nw;
    }
  }
}

// ------------------------------------------------------------------ host side
static const bc_run_kind HMC_SMALL_RUN = {"bc_hmc_small", "iterations"};
struct bc_hmc_small : bc_run {    // (the run in progress: active, chunk_pending, done of total iterations, the clock; `failed` is never set)
  bc_scratch prob;                // rows | w | row_ptr (int64)
  bc_scratch state;               // theta | g | lj | inverse masses | flags (ints)
  bc_stage stage;                 // a chunk's draws and steps: normals | log-uniforms | step [P]
  bc_scratch out;                 // a chunk's results: samples | log-joints | accept flags (ints)
  bc_scratch score;               // a chunk's held-out scores (bc_score_chunk): ll [P k C] | correct [P k C] (ints)
  bool scored = false;            // bc_score_chunk has enqueued the pending chunk's scores
  bc_diag_attached diag;          // the chain summary attached to the run (bc_diag_attach), and its buffers
  SmArgs a;
  size_t lds = 0;
  int cpb = 1;                    // chains per block of the run's launches
  int32_t n_problems = 0, pending_k = 0;
  size_t o_l = 0, o_a = 0;        // where the pending chunk's log-joints and accept flags begin in `out` (set by _chunk_begin)
  // ---- the per-chain warm-up (include/beta_cores_hmc_adapt.h)
  bc_scratch adapt;               // per chain: scalars [BC_HMC_ADAPT_STATE] | inverse mass [d] | mean [d] | M2 [d]
  std::vector<double> plan;       // [warm_total][4] = eta | sg | zeta | flags
  bool adapt_on = false;          // bc_hmc_adapt_begin has been called on this run
  bool pending_adapt = false;     // the pending chunk is a warm-up chunk: its steps and alphas lie behind the accept flags
  int32_t warm_total = 0, warm_done = 0;
  size_t o_st = 0, o_al = 0;      // where they begin in `out`
};

bool bc_hmc_small_active(const bc_ctx* ctx) { return ctx->hmc_small && ctx->hmc_small->active; }

void bc_hmc_small_free(bc_ctx* ctx) {
  bc_hmc_small* h = ctx->hmc_small;
  if (!h) return;
  bc_scratch_free(&h->prob);
  bc_scratch_free(&h->state);
  bc_stage_free(&h->stage);
  bc_scratch_free(&h->out);
  bc_scratch_free(&h->score);
  bc_scratch_free(&h->diag.keep);
  bc_scratch_free(&h->diag.work);
  bc_scratch_free(&h->adapt);
  h->clock.free();
  delete h;
  ctx->hmc_small = nullptr;
}

// the doubles of LDS a block of cpb chains needs for a problem of n rows and d columns; with cpb = 1: the capacity rule
static size_t lds_doubles(int64_t n, int d, int cpb = 1) {
  return BC_HMC_SMALL_ROWS_DOUBLES(n, d) + (size_t)cpb * (BC_HMC_SMALL_CHAIN_DOUBLES(n, d) + BC_SM_STATE_DOUBLES(d));
}

static const void* kernel_of(int cpb) {
  return cpb == 4 ? reinterpret_cast<const void*>(&k_hmc_small<4>)
                  : cpb == 2 ? reinterpret_cast<const void*>(&k_hmc_small<2>) : reinterpret_cast<const void*>(&k_hmc_small<1>);
}

static const void* adapt_kernel_of(int cpb) {
  return cpb == 4 ? reinterpret_cast<const void*>(&k_hmc_small<4, 1>)
                  : cpb == 2 ? reinterpret_cast<const void*>(&k_hmc_small<2, 1>) : reinterpret_cast<const void*>(&k_hmc_small<1, 1>);
}

// Chains per block: of 1, 2, 4 (divisors of c whose block fits the LDS for the largest problem) the smallest that keeps the most
// waves resident per CU, as the runtime's occupancy query counts them for the launch's block size and LDS.  Where a problem's
// rows fill most of a CU's LDS that is 4; where several one-chain blocks fit a CU anyway it is 1 (measurements:
// profiles/hmc_many_notes.md).  Packing changes no chain's bits.  BC_HMC_SMALL_CHAINS_PER_BLOCK = 1, 2 or 4 forces a count
// (lowered to one that divides c and fits).
static int chains_per_block(const bc_ctx* ctx, int64_t max_n, int d, int c) {
  int forced = 0;
  if (const char* e = getenv("BC_HMC_SMALL_CHAINS_PER_BLOCK")) forced = atoi(e);
  int best = 1, best_waves = -1;
  for (int cpb = 1; cpb <= 4; cpb <<= 1) {
    const size_t lds = lds_doubles(max_n, d, cpb) * sizeof(double);
    if (c % cpb != 0 || lds > (size_t)ctx->max_lds) continue;
    if (forced == 1 || forced == 2 || forced == 4) {
      if (cpb <= forced) best = cpb;
      continue;
    }
    int blocks = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, kernel_of(cpb), cpb * BC_SM_BLOCK, lds) != hipSuccess) {
      (void)hipGetLastError();
      continue;
    }
    if (blocks * cpb > best_waves) {
      best_waves = blocks * cpb;
      best = cpb;
    }
  }
  return best;
}

#define BC_SM_MAX_ROWS ((int64_t)1 << 24)
static bool fits(const bc_ctx* ctx, int64_t n, int32_t d) {
  if (n < 1 || d < 1 || d > BC_HMC_MAX_DIM || n > BC_SM_MAX_ROWS) return false;
  return lds_doubles(n, d) * sizeof(double) <= (size_t)ctx->max_lds;
}

extern "C" int bc_hmc_small_fits(bc_ctx* ctx, int64_t n, int32_t d) { return ctx && fits(ctx, n, d) ? 1 : 0; }

static bc_hmc_small* small_of(bc_ctx* ctx) {
  if (!ctx->hmc_small) ctx->hmc_small = new bc_hmc_small();
  return ctx->hmc_small;
}

// the checks of a batch, before anything is touched; *max_n: the largest problem
static int check_batch(bc_ctx* ctx, const int64_t* row_ptr, int32_t n_problems, int32_t d, int32_t c, const char* who, int64_t* max_n) {
  if (n_problems < 1) BC_REFUSE("%s: needs at least one problem, got %d", who, n_problems);
  if (c < 1 || c > BC_HMC_MAX_CHAINS) BC_REFUSE("%s: 1 .. %d chains are served, got %d", who, BC_HMC_MAX_CHAINS, c);
  if (d < 1 || d > BC_HMC_MAX_DIM) BC_REFUSE("%s: rows must have 1 .. %d columns, got %d", who, BC_HMC_MAX_DIM, d);
  if ((int64_t)n_problems * c > (int64_t)1 << 30) BC_REFUSE("%s: %d problems x %d chains are too many blocks for one launch", who, n_problems, c);
  const int rc = bc_batch_walk(who, row_ptr, n_problems, BC_SM_MAX_ROWS, "rows", max_n);
  if (rc) return rc;
  if (!fits(ctx, *max_n, d))      // (this unit's own limit: a problem's rows lie in its block's LDS; the largest problem decides)
    BC_REFUSE("%s: a problem of %lld rows x %d needs %zu bytes of LDS, a block has %d", who, (long long)*max_n, d,
              lds_doubles(*max_n, d) * sizeof(double), ctx->max_lds);
  return BC_OK;
}

// uploads the batch and the C x D vectors per problem, lays the state out and fills h->a except the chunk's fields; enqueued only
static int stage_batch(bc_ctx* ctx, bc_hmc_small* h, const double* rows, const double* w, const int64_t* row_ptr, int32_t P, int32_t d,
                       const double* theta, int32_t c, const double* inv_mass, int64_t max_n) {
  const size_t n_all = (size_t)row_ptr[P];
  bc_slab pr, st;
  const size_t o_rows = pr.take(n_all * d), o_w = pr.take(n_all), o_ptr = pr.take_unpadded((size_t)P + 2);      // (row_ptr: P + 1 int64)
  int rc = bc_scratch_grow(ctx, &h->prob, pr.total);
  const size_t pc = (size_t)P * c;
  const size_t o_theta = st.take(pc * d), o_g = st.take(pc * d), o_lj = st.take(pc), o_im = st.take((size_t)P * d);
  const size_t o_flag = st.take(((size_t)P + 1) / 2);      // (P + 1 ints)
  st.take(2);
  if (!rc) rc = bc_scratch_grow(ctx, &h->state, st.total);
  if (rc) return rc;
  // (per device, and cheap beside the uploads below: set at every begin instead of remembering where it was set)
  for (int cpb = 1; cpb <= 4; cpb <<= 1) BC_HIP(hipFuncSetAttribute(kernel_of(cpb), hipFuncAttributeMaxDynamicSharedMemorySize, ctx->max_lds));
  BC_HIP(hipStreamSynchronize(ctx->stream));
  // (pageable sources: the copies below have read them when they return)
  double* prob = h->prob.p;
  BC_HIP(hipMemcpyAsync(prob + o_rows, rows, n_all * d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  BC_HIP(hipMemcpyAsync(prob + o_w, w, n_all * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  BC_HIP(hipMemcpyAsync(prob + o_ptr, row_ptr, ((size_t)P + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
  SmArgs& a = h->a;
  memset(&a, 0, sizeof(a));
  a.rows = prob + o_rows;
  a.w = prob + o_w;
  a.row_ptr = reinterpret_cast<const long long*>(prob + o_ptr);
  double* s = h->state.p;
  a.theta = s + o_theta;
  a.g = s + o_g;
  a.lj = s + o_lj;
  a.im = s + o_im;
  a.flag = reinterpret_cast<int*>(s + o_flag);
  BC_HIP(hipMemcpyAsync(a.theta, theta, pc * d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  if (inv_mass) BC_HIP(hipMemcpyAsync(const_cast<double*>(a.im), inv_mass, (size_t)P * d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  BC_HIP(hipMemsetAsync(a.flag, 0, ((size_t)P + 1) * sizeof(int), ctx->stream));
  a.half_d_log_2pi = 0.5 * d * log(2. * M_PI);
  a.d = d;
  a.c = c;
  h->cpb = chains_per_block(ctx, max_n, d, c);
  h->n_problems = P;
  h->lds = lds_doubles(max_n, d, h->cpb) * sizeof(double);
  return BC_OK;
}

static int launch(bc_ctx* ctx, const bc_hmc_small* h, const SmArgs& a, bool adapt = false) {
  const dim3 grid((unsigned)((size_t)h->n_problems * (a.c / h->cpb))), block(h->cpb * BC_SM_BLOCK);
  if (adapt) {
    if (h->cpb == 4) hipLaunchKernelGGL((k_hmc_small<4, 1>), grid, block, h->lds, ctx->stream, a);
    else if (h->cpb == 2) hipLaunchKernelGGL((k_hmc_small<2, 1>), grid, block, h->lds, ctx->stream, a);
    else hipLaunchKernelGGL((k_hmc_small<1, 1>), grid, block, h->lds, ctx->stream, a);
  } else if (h->cpb == 4) hipLaunchKernelGGL(k_hmc_small<4>, grid, block, h->lds, ctx->stream, a);
  else if (h->cpb == 2) hipLaunchKernelGGL(k_hmc_small<2>, grid, block, h->lds, ctx->stream, a);
  else hipLaunchKernelGGL(k_hmc_small<1>, grid, block, h->lds, ctx->stream, a);
  BC_HIP(hipGetLastError());
  return BC_OK;
}

extern "C" int bc_hmc_small_logjoint(bc_ctx* ctx, const double* rows, const double* w, const int64_t* row_ptr, int32_t n_problems, int32_t d,
                                     const double* theta, int32_t c, double* out_value, double* out_grad) {
  if (!ctx || !rows || !w || !row_ptr || !theta || !out_grad)
    BC_REFUSE("bc_hmc_small_logjoint: bad argument (context, rows, weights, row_ptr, theta and gradients are required)");
  int64_t max_n = 0;
  int rc = check_batch(ctx, row_ptr, n_problems, d, c, "bc_hmc_small_logjoint", &max_n);
  if (!rc) rc = bc_ctx_refuse_busy(ctx, "bc_hmc_small_logjoint", BC_HOLD_ALL, BC_HOLD_HMC_SMALL);
  if (rc) return rc;
  BC_HIP(hipSetDevice(ctx->device));
  bc_hmc_small* h = small_of(ctx);
  rc = stage_batch(ctx, h, rows, w, row_ptr, n_problems, d, theta, c, nullptr, max_n);
  if (rc) return rc;
  SmArgs a = h->a;
  a.mode = BC_SM_PASS;
  a.value = out_value != nullptr;
  rc = launch(ctx, h, a);
  if (rc) return rc;
  const size_t pc = (size_t)n_problems * c;
  if (out_value) BC_HIP(hipMemcpyAsync(out_value, a.lj, pc * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  BC_HIP(hipMemcpyAsync(out_grad, a.g, pc * d * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  BC_HIP(hipStreamSynchronize(ctx->stream));
  return BC_OK;
}

extern "C" int bc_hmc_small_begin(bc_ctx* ctx, const double* rows, const double* w, const int64_t* row_ptr, int32_t n_problems, int32_t d,
                                  const double* start, int32_t c, const double* inv_mass, int32_t n_leapfrog, int64_t n_iter) {
  if (!ctx || !rows || !w || !row_ptr || !start || !inv_mass)
    BC_REFUSE("bc_hmc_small_begin: bad argument (context, rows, weights, row_ptr, start and inv_mass are required)");
  int64_t max_n = 0;
  int rc = check_batch(ctx, row_ptr, n_problems, d, c, "bc_hmc_small_begin", &max_n);
  if (rc) return rc;
  if (n_leapfrog < 1 || n_iter < 1)
    BC_REFUSE("bc_hmc_small_begin: needs n_leapfrog >= 1 and n_iter >= 1 (n_leapfrog = %d, n_iter = %lld)", n_leapfrog, (long long)n_iter);
  for (size_t k = 0; k < (size_t)n_problems * d; ++k)
    if (!(inv_mass[k] > 0.) || !std::isfinite(inv_mass[k]))
      BC_REFUSE("bc_hmc_small_begin: inv_mass[%zu][%zu] = %g is not finite and positive", k / d, k % d, inv_mass[k]);
  rc = bc_ctx_refuse_busy(ctx, "bc_hmc_small_begin", BC_HOLD_ALL, BC_HOLD_HMC_SMALL);
  if (rc) return rc;
  BC_HIP(hipSetDevice(ctx->device));
  bc_hmc_small* h = small_of(ctx);
  rc = h->clock.create();
  if (!rc) rc = stage_batch(ctx, h, rows, w, row_ptr, n_problems, d, start, c, inv_mass, max_n);
  if (rc) return rc;
  SmArgs a = h->a;
  a.mode = BC_SM_INIT;
  a.value = 1;
  rc = launch(ctx, h, a);
  if (rc) return rc;
  h->a.n_leapfrog = n_leapfrog;
  h->pending_k = 0;
  h->diag.on = false;             // (a summary left attached to an earlier run is dropped)
  h->adapt_on = h->pending_adapt = false;
  bc_run_opened(h, n_iter);
  return BC_OK;
}

// The chunk begin behind bc_hmc_small_chunk_begin (`step`: P steps, one per problem) and the two of beta_cores_hmc_adapt.h
// (step = null; warm: a warm-up chunk, whose plan rows travel where the steps do, else kept iterations at the frozen state).
static const bc_run_kind HMC_ADAPT_RUN = {"bc_hmc_adapt", "iterations"}, HMC_ADAPTED_RUN = {"bc_hmc_adapted", "iterations"};
static int chunk_begin(bc_ctx* ctx, const bc_run_kind& kd, const double* normals, const double* log_u, int64_t problem_stride, int32_t k,
                       const double* step, bool warm) {
  bc_hmc_small* h = ctx ? ctx->hmc_small : nullptr;
  const bool adapt = step == nullptr;
  // (said here for the two of beta_cores_hmc_adapt.h: which call ends the pending chunk depends on what it is, not on this one)
  if (adapt && h && h->active && h->chunk_pending) BC_REFUSE("%s_chunk_begin: a chunk is pending (end it first)", kd.name);
  int rc = bc_run_admit(h, kd, normals && log_u, k);
  if (rc) return rc;
  if (adapt && !h->adapt_on) BC_REFUSE("%s_chunk_begin: the run has no per-chain warm-up (call bc_hmc_adapt_begin first)", kd.name);
  if (adapt && warm && (int64_t)h->warm_done + k > h->warm_total)
    BC_REFUSE("%s_chunk_begin: %d warm-up iterations after %d exceed the plan's %d", kd.name, k, h->warm_done, h->warm_total);
  const size_t P = (size_t)h->n_problems, c = (size_t)h->a.c, d = (size_t)h->a.d;
  const size_t kcd = (size_t)k * c * d, kc = (size_t)k * c;
  if (problem_stride != 0 && (problem_stride < 0 || (size_t)problem_stride < kcd))
    BC_REFUSE("%s_chunk_begin: problem_stride must be 0 or at least k C D = %zu, got %lld", kd.name, kcd, (long long)problem_stride);
  for (size_t p = 0; !adapt && p < P; ++p)
    if (!(step[p] > 0.) || !std::isfinite(step[p]))
      BC_REFUSE("%s_chunk_begin: step[%zu] = %g is not finite and positive", kd.name, p, step[p]);
  // ---- nothing of this chunk has been enqueued up to here
  BC_HIP(hipSetDevice(ctx->device));
  const bool shared = problem_stride == 0;
  const size_t n_e = shared ? kcd : P * kcd, n_u = shared ? kc : P * kc;
  const size_t n_st = adapt ? (warm ? 4 * (size_t)k : 0) : P;      // the steps, or the chunk's rows of the plan
  bc_slab st, out;
  st.take(n_e);
  const size_t o_u = st.take(n_u), o_st = st.take(n_st), need = st.total;
  out.take(P * kcd);
  h->o_l = out.take(P * kc);
  h->o_a = out.take((P * kc + 1) / 2);      // (ints)
  if (adapt && warm) {
    h->o_st = out.take(P * kc);
    h->o_al = out.take(P * kc);
  }
  rc = bc_stage_reserve(ctx, &h->stage, need);
  if (!rc) rc = bc_scratch_grow(ctx, &h->out, out.total);
  if (rc) return rc;
  double* pin = h->stage.pin.p;
  const double* dev = h->stage.dev.p;
  if (shared) memcpy(pin, normals, kcd * sizeof(double));
  else
    for (size_t p = 0; p < P; ++p) memcpy(pin + p * kcd, normals + p * (size_t)problem_stride, kcd * sizeof(double));
  memcpy(pin + o_u, log_u, n_u * sizeof(double));
  if (!adapt) memcpy(pin + o_st, step, P * sizeof(double));
  else if (warm) memcpy(pin + o_st, h->plan.data() + 4 * (size_t)h->warm_done, n_st * sizeof(double));
  BC_HIP(hipMemcpyAsync(h->stage.dev.p, pin, need * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  h->chunk_pending = true;      // from here on something is enqueued: _chunk_end must wait even if the launch below fails
  h->scored = false;
  h->diag.folded = false;
  h->pending_k = k;
  h->pending_adapt = adapt && warm;
  SmArgs a = h->a;
  a.mode = BC_SM_CHUNK;
  a.k = k;
  a.e = dev;
  a.logu = dev + o_u;
  a.step = adapt ? nullptr : dev + o_st;
  a.plan = adapt && warm ? dev + o_st : nullptr;
  a.out_step = adapt && warm ? h->out.p + h->o_st : nullptr;
  a.out_alpha = adapt && warm ? h->out.p + h->o_al : nullptr;
  a.e_stride = shared ? 0 : (long long)kcd;
  a.u_stride = shared ? 0 : (long long)kc;
  a.out_s = h->out.p;
  a.out_l = h->out.p + h->o_l;
  a.out_a = reinterpret_cast<int*>(h->out.p + h->o_a);
  rc = h->clock.start(ctx->stream);
  if (!rc) rc = launch(ctx, h, a, adapt);
  if (!rc) rc = h->clock.stop(ctx->stream);
  if (rc) return rc;
  h->done += k;
  if (adapt && warm) h->warm_done += k;
  return BC_OK;
}

extern "C" int bc_hmc_small_chunk_begin(bc_ctx* ctx, const double* normals, const double* log_u, int64_t problem_stride, int32_t k,
                                        const double* step) {
  if (!step) BC_REFUSE("bc_hmc_small_chunk_begin: bad argument, or no run is open");
  return chunk_begin(ctx, HMC_SMALL_RUN, normals, log_u, problem_stride, k, step, false);
}

// the chunk end behind the three headers.  out_samples may be null for bc_score_chunk_end and bc_hmc_adapt_chunk_end (their callers
// check); out_correct / out_ll: both or neither
static int chunk_end(bc_ctx* ctx, bc_hmc_small* h, double* out_samples, double* out_logjoint, int32_t* out_accept, int32_t* out_status,
                     int32_t* out_correct, double* out_ll) {
  h->scored = false;
  const int rc = bc_run_wait_chunk(ctx, h);
  if (rc) return rc;
  const size_t P = (size_t)h->n_problems, c = (size_t)h->a.c, d = (size_t)h->a.d;
  std::vector<int> flag(P);
  BC_HIP(hipMemcpy(flag.data(), h->a.flag, P * sizeof(int), hipMemcpyDeviceToHost));
  const size_t kc = (size_t)h->pending_k * c, kcd = kc * d;
  const int* acc_dev = reinterpret_cast<const int*>(h->out.p + h->o_a);
  const int* cor_dev = out_ll ? reinterpret_cast<const int*>(h->score.p + bc_even(P * kc)) : nullptr;
  return bc_batch_unmarked_runs(flag.data(), P, out_status, [&](size_t p, size_t q) {
    if (out_samples) BC_HIP(hipMemcpy(out_samples + p * kcd, h->out.p + p * kcd, (q - p) * kcd * sizeof(double), hipMemcpyDeviceToHost));
    BC_HIP(hipMemcpy(out_logjoint + p * kc, h->out.p + h->o_l + p * kc, (q - p) * kc * sizeof(double), hipMemcpyDeviceToHost));
    BC_HIP(hipMemcpy(out_accept + p * kc, acc_dev + p * kc, (q - p) * kc * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (out_ll) {
      BC_HIP(hipMemcpy(out_ll + p * kc, h->score.p + p * kc, (q - p) * kc * sizeof(double), hipMemcpyDeviceToHost));
      BC_HIP(hipMemcpy(out_correct + p * kc, cor_dev + p * kc, (q - p) * kc * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    return BC_OK;
  });
}

extern "C" int bc_hmc_small_chunk_end(bc_ctx* ctx, double* out_samples, double* out_logjoint, int32_t* out_accept, int32_t* out_status) {
  bc_hmc_small* h = ctx ? ctx->hmc_small : nullptr;
  const int rc = bc_run_pending(h, "bc_hmc_small_chunk_end");
  if (rc) return rc;
  // (checked first: the chunk stays pending, a second call with the outputs can still fetch it)
  if (!out_samples || !out_logjoint || !out_accept || !out_status) BC_REFUSE("bc_hmc_small_chunk_end: the four outputs are required");
  return chunk_end(ctx, h, out_samples, out_logjoint, out_accept, out_status, nullptr, nullptr);
}

// ---- include/beta_cores_score.h: the held-out scores of the pending chunk, computed where its samples lie (k_lr_score, bc_score.hip)
extern "C" int bc_score_chunk(bc_ctx* ctx, const bc_data* zt, const bc_data* yt) {
  bc_hmc_small* h = ctx ? ctx->hmc_small : nullptr;
  if (!h || !h->active || !h->chunk_pending) BC_REFUSE("bc_score_chunk: no chunk of a batched small-problem run is pending");
  const int64_t t = (int64_t)h->n_problems * h->pending_k * h->a.c;
  int rc = bc_score_check(ctx, zt, yt, t, h->a.d, "bc_score_chunk");
  if (rc) return rc;
  BC_HIP(hipSetDevice(ctx->device));
  rc = bc_scratch_grow(ctx, &h->score, bc_even((size_t)t) + ((size_t)t + 1) / 2);
  if (rc) return rc;
  // (the stream orders this behind the chunk's launch; a marked problem's slice holds no samples: its scores are never copied)
  rc = bc_score_launch(ctx, zt, yt, h->out.p, t, reinterpret_cast<int*>(h->score.p + bc_even((size_t)t)), h->score.p);
  if (rc) return rc;
  h->scored = true;
  return BC_OK;
}

extern "C" int bc_score_chunk_end(bc_ctx* ctx, double* out_samples, double* out_logjoint, int32_t* out_accept, int32_t* out_status,
                                  int32_t* out_correct, double* out_ll) {
  bc_hmc_small* h = ctx ? ctx->hmc_small : nullptr;
  const int rc = bc_run_pending(h, "bc_score_chunk_end");
  if (rc) return rc;
  // (checked first: the chunk stays pending, a second call -- of either chunk end -- can still fetch it)
  if (!out_logjoint || !out_accept || !out_status) BC_REFUSE("bc_score_chunk_end: log-joints, accept flags and status are required");
  if ((out_correct == nullptr) != (out_ll == nullptr)) BC_REFUSE("bc_score_chunk_end: out_correct and out_ll are given together or not at all");
  if (out_ll && !h->scored) BC_REFUSE("bc_score_chunk_end: no score was enqueued for this chunk (call bc_score_chunk first)");
  return chunk_end(ctx, h, out_samples, out_logjoint, out_accept, out_status, out_correct, out_ll);
}

// ---- include/beta_cores_diag.h: the chain summary of the run's kept chunks, retained where they lie (the kernels: bc_diag.hip)
static bc_diag_shape diag_shape(const bc_hmc_small* h) {
  bc_diag_shape s;
  s.p = h->n_problems, s.n = h->diag.n_keep, s.c = h->a.c, s.d = h->a.d, s.max_lag = h->diag.max_lag;
  return s;
}

extern "C" int bc_diag_attach(bc_ctx* ctx, int64_t n_keep, int64_t max_lag) {
  bc_hmc_small* h = ctx ? ctx->hmc_small : nullptr;
  if (!h || !h->active) BC_REFUSE("bc_diag_attach: no batched small-problem run is open");
  if (h->diag.on) BC_REFUSE("bc_diag_attach: a summary is already attached to this run");
  bc_diag_attached& g = h->diag;
  const int64_t keep0 = g.n_keep, lag0 = g.max_lag;
  g.n_keep = n_keep, g.max_lag = max_lag;
  const bc_diag_shape s = diag_shape(h);
  int rc = bc_diag_check("bc_diag_attach", s);
  if (!rc) {
    BC_HIP(hipSetDevice(ctx->device));
    rc = bc_scratch_grow(ctx, &g.keep, bc_diag_keep_doubles(s));
  }
  if (rc) {
    g.n_keep = keep0, g.max_lag = lag0;
    return rc;
  }
  g.kept = 0;
  g.folded = false;
  g.on = true;
  return BC_OK;
}

extern "C" int bc_diag_chunk(bc_ctx* ctx) {
  bc_hmc_small* h = ctx ? ctx->hmc_small : nullptr;
  if (!h || !h->active || !h->chunk_pending) BC_REFUSE("bc_diag_chunk: no chunk of a batched small-problem run is pending");
  bc_diag_attached& g = h->diag;
  if (!g.on) BC_REFUSE("bc_diag_chunk: no summary is attached to this run (call bc_diag_attach first)");
  if (g.folded) BC_REFUSE("bc_diag_chunk: this chunk has been folded in already");
  if (g.kept + h->pending_k > g.n_keep)
    BC_REFUSE("bc_diag_chunk: %d iterations after %lld exceed the summary's %lld", h->pending_k, (long long)g.kept, (long long)g.n_keep);
  BC_HIP(hipSetDevice(ctx->device));
  // (the stream orders this behind the chunk's launch and in front of the next chunk's; a marked problem's slice holds no samples:
  // its summary is never copied)
  const int rc = bc_diag_keep_launch(ctx, h->out.p, diag_shape(h), h->pending_k, g.kept, g.keep.p);
  if (rc) return rc;
  g.kept += h->pending_k;
  g.folded = true;
  return BC_OK;
}

extern "C" int bc_diag_end(bc_ctx* ctx, double* out_mean, double* out_cov, double* out_rhat, double* out_ess, int32_t* out_ess_truncated,
                           int32_t* out_status, double* out_rho, double* out_moments) {
  bc_hmc_small* h = ctx ? ctx->hmc_small : nullptr;
  if (!h || !h->diag.on) BC_REFUSE("bc_diag_end: no summary is attached (call bc_diag_attach on an open batched small-problem run first)");
  const bc_diag_out out = {out_mean, out_cov, out_rhat, out_ess, out_ess_truncated, out_status, out_rho, out_moments};
  if (!bc_diag_out_ok(out)) BC_REFUSE("bc_diag_end: mean, cov, rhat, ess, ess_truncated and status are required");
  bc_diag_attached& g = h->diag;
  if (h->active && h->chunk_pending) BC_REFUSE("bc_diag_end: a chunk is pending (end it first)");
  if (g.kept != g.n_keep) BC_REFUSE("bc_diag_end: %lld of %lld iterations have been folded in", (long long)g.kept, (long long)g.n_keep);
  int rc = bc_ctx_refuse_busy(ctx, "bc_diag_end", BC_HOLD_ALL & ~BC_HOLD_HMC_SMALL);
  if (rc) return rc;
  BC_HIP(hipSetDevice(ctx->device));
  const bc_diag_shape s = diag_shape(h);
  rc = bc_scratch_grow(ctx, &g.work, bc_diag_run_doubles(s));
  if (rc) return rc;
  g.on = false;
  return bc_diag_run(ctx, g.keep.p, g.work.p, s, h->a.flag, out);
}

// ---- include/beta_cores_hmc_adapt.h: the per-chain warm-up of the open run (the stage: k_hmc_small<CPB, 1>)
extern "C" int bc_hmc_adapt_plan(int32_t n_warmup, int32_t init_buffer, int32_t term_buffer, int32_t base_window, double gamma, double t0,
                                 double kappa, int32_t* out_flags, double* out_coef) {
  if (n_warmup > 0 && (!out_flags || !out_coef)) BC_REFUSE("bc_hmc_adapt_plan: the flags and the coefficients are required");
  if (bc_hmc_adapt_plan_fill(n_warmup, init_buffer, term_buffer, base_window, gamma, t0, kappa, out_flags, out_coef))
    BC_REFUSE("bc_hmc_adapt_plan: needs n_warmup >= 0, buffers >= 0, base_window >= 1, gamma > 0, t0 >= 0 and kappa > 0, all finite "
              "(n_warmup = %d, buffers %d / %d, base_window = %d, gamma = %g, t0 = %g, kappa = %g)", n_warmup, init_buffer, term_buffer,
              base_window, gamma, t0, kappa);
  return BC_OK;
}

extern "C" int bc_hmc_adapt_begin(bc_ctx* ctx, const double* log_step, double delta, double gamma, double t0, double kappa, int32_t n_warmup,
                                  int32_t init_buffer, int32_t term_buffer, int32_t base_window) {
  bc_hmc_small* h = ctx ? ctx->hmc_small : nullptr;
  if (!h || !h->active || !log_step) BC_REFUSE("bc_hmc_adapt_begin: bad argument, or no batched small-problem run is open");
  if (h->adapt_on) BC_REFUSE("bc_hmc_adapt_begin: the run's warm-up has been begun already");
  if (h->chunk_pending || h->done != 0) BC_REFUSE("bc_hmc_adapt_begin: must be called before the run's first chunk");
  if (!(delta > 0.) || !(delta < 1.)) BC_REFUSE("bc_hmc_adapt_begin: delta must lie in (0, 1), got %g", delta);
  if (n_warmup < 1 || (int64_t)n_warmup > h->total)
    BC_REFUSE("bc_hmc_adapt_begin: n_warmup must be 1 .. the run's %lld iterations, got %d", (long long)h->total, n_warmup);
  const size_t P = (size_t)h->n_problems, c = (size_t)h->a.c, d = (size_t)h->a.d, pc = P * c;
  for (size_t p = 0; p < P; ++p)
    if (!std::isfinite(log_step[p])) BC_REFUSE("bc_hmc_adapt_begin: log_step[%zu] = %g is not finite", p, log_step[p]);
  std::vector<int32_t> flags((size_t)n_warmup);
  std::vector<double> coef(3 * (size_t)n_warmup);
  const int rc_plan = bc_hmc_adapt_plan(n_warmup, init_buffer, term_buffer, base_window, gamma, t0, kappa, flags.data(), coef.data());
  if (rc_plan) return rc_plan;
  // ---- the arguments are good
  BC_HIP(hipSetDevice(ctx->device));
  h->plan.resize(4 * (size_t)n_warmup);
  for (size_t i = 0; i < (size_t)n_warmup; ++i) {
    for (int j = 0; j < 3; ++j) h->plan[4 * i + j] = coef[3 * i + j];
    h->plan[4 * i + 3] = (double)flags[i];
  }
  bc_slab sl;
  const size_t o_sc = sl.take(pc * BC_HMC_ADAPT_STATE), o_im = sl.take(pc * d), o_mean = sl.take(pc * d), o_m2 = sl.take(pc * d);
  int rc = bc_scratch_grow(ctx, &h->adapt, sl.total);
  if (rc) return rc;
  for (int cpb = 1; cpb <= 4; cpb <<= 1)
    BC_HIP(hipFuncSetAttribute(adapt_kernel_of(cpb), hipFuncAttributeMaxDynamicSharedMemorySize, ctx->max_lds));
  // every chain starts from its problem's step and inverse mass (the masses are read back: the run keeps them on the device only)
  std::vector<double> host(sl.total, 0.), im(P * d);
  BC_HIP(hipMemcpyAsync(im.data(), h->a.im, P * d * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  BC_HIP(hipStreamSynchronize(ctx->stream));
  const double log10 = log(10.);
  for (size_t b = 0; b < pc; ++b) {
    double* st = host.data() + o_sc + b * BC_HMC_ADAPT_STATE;
    st[0] = log_step[b / c];
    st[3] = log10 + st[0];
    memcpy(host.data() + o_im + b * d, im.data() + (b / c) * d, d * sizeof(double));
  }
  BC_HIP(hipMemcpyAsync(h->adapt.p, host.data(), sl.total * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  BC_HIP(hipStreamSynchronize(ctx->stream));      // (a pageable source)
  h->a.ad_st = h->adapt.p + o_sc;
  h->a.ad_im = h->adapt.p + o_im;
  h->a.ad_mean = h->adapt.p + o_mean;
  h->a.ad_m2 = h->adapt.p + o_m2;
  h->a.delta = delta;
  h->a.log10 = log10;
  h->warm_total = n_warmup;
  h->warm_done = 0;
  h->adapt_on = true;
  return BC_OK;
}

extern "C" int bc_hmc_adapt_chunk_begin(bc_ctx* ctx, const double* normals, const double* log_u, int64_t problem_stride, int32_t k) {
  return chunk_begin(ctx, HMC_ADAPT_RUN, normals, log_u, problem_stride, k, nullptr, true);
}

extern "C" int bc_hmc_adapted_chunk_begin(bc_ctx* ctx, const double* normals, const double* log_u, int64_t problem_stride, int32_t k) {
  return chunk_begin(ctx, HMC_ADAPTED_RUN, normals, log_u, problem_stride, k, nullptr, false);
}

extern "C" int bc_hmc_adapt_chunk_end(bc_ctx* ctx, double* out_samples, double* out_logjoint, int32_t* out_accept, int32_t* out_status,
                                      double* out_step, double* out_alpha) {
  bc_hmc_small* h = ctx ? ctx->hmc_small : nullptr;
  int rc = bc_run_pending(h, "bc_hmc_adapt_chunk_end");
  if (rc) return rc;
  // (checked first: the chunk stays pending, a second call can still fetch it)
  if (!h->pending_adapt) BC_REFUSE("bc_hmc_adapt_chunk_end: the pending chunk is not a warm-up chunk of bc_hmc_adapt_chunk_begin");
  if (!out_logjoint || !out_accept || !out_status || !out_step || !out_alpha)
    BC_REFUSE("bc_hmc_adapt_chunk_end: log-joints, accept flags, status, steps and alphas are required");
  rc = chunk_end(ctx, h, out_samples, out_logjoint, out_accept, out_status, nullptr, nullptr);
  if (rc) return rc;
  const size_t P = (size_t)h->n_problems, kc = (size_t)h->pending_k * h->a.c;
  for (size_t p = 0; p < P; ++p) {
    if (out_status[p] != BC_OK) continue;      // (a marked problem: nothing is copied)
    BC_HIP(hipMemcpy(out_step + p * kc, h->out.p + h->o_st + p * kc, kc * sizeof(double), hipMemcpyDeviceToHost));
    BC_HIP(hipMemcpy(out_alpha + p * kc, h->out.p + h->o_al + p * kc, kc * sizeof(double), hipMemcpyDeviceToHost));
  }
  return BC_OK;
}

extern "C" int bc_hmc_adapt_state(bc_ctx* ctx, double* out_step, double* out_inv_mass) {
  bc_hmc_small* h = ctx ? ctx->hmc_small : nullptr;
  if (!h || !h->active || !out_step || !out_inv_mass) BC_REFUSE("bc_hmc_adapt_state: bad argument, or no batched small-problem run is open");
  if (!h->adapt_on) BC_REFUSE("bc_hmc_adapt_state: the run has no per-chain warm-up (call bc_hmc_adapt_begin first)");
  if (h->chunk_pending) BC_REFUSE("bc_hmc_adapt_state: a chunk is pending (end it first)");
  BC_HIP(hipSetDevice(ctx->device));
  const size_t pc = (size_t)h->n_problems * h->a.c, d = (size_t)h->a.d;
  std::vector<double> st(pc * BC_HMC_ADAPT_STATE);
  BC_HIP(hipMemcpyAsync(st.data(), h->a.ad_st, st.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  BC_HIP(hipMemcpyAsync(out_inv_mass, h->a.ad_im, pc * d * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  BC_HIP(hipStreamSynchronize(ctx->stream));
  // (the text the kernel evaluates at the start of a kept chunk, on the host: the same operations, the same bits)
  for (size_t b = 0; b < pc; ++b) {
    const double* sb = st.data() + b * BC_HMC_ADAPT_STATE;
    out_step[b] = bc_hmc_adapt_exp(bc_hmc_adapt_frozen_log_step(sb[0], sb[1], sb[4]));
  }
  return BC_OK;
}

extern "C" int bc_hmc_small_end(bc_ctx* ctx) {
  bc_hmc_small* h = ctx ? ctx->hmc_small : nullptr;
  bool pending = false;
  const int rc = bc_run_end(ctx, h, HMC_SMALL_RUN, &pending);
  if (!rc) h->scored = h->pending_adapt = false;
  return rc;
}

extern "C" int bc_hmc_small_device_ms(bc_ctx* ctx, double* out_ms) {
  return bc_device_ms("bc_hmc_small_device_ms", ctx, ctx && ctx->hmc_small ? &ctx->hmc_small->clock : nullptr, out_ms);
}
