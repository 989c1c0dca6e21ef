// K1: per-datapoint (beta-)log-likelihood projection, fused with row-centring (projector.py:26,55),
// row norms (giga.py:10) and per-tile column sums (K2, hilbert.py:17 / bcores.py:77).
//
//   Phi[i, s] = f(z_i, theta_s) - mean_s f(z_i, theta_.)
//
// The contraction P[s, i] = sum_d Theta[s, d] * Z[i, d] is a dense (S x D)(D x 128) product
// per 128-row tile; it runs on the fp64 matrix cores (v_mfma_f64_16x16x4_f64) with Theta as the
// A operand and the Z tile as the B operand, so that the accumulator of a lane holds, for ONE
// data row, samples {g + 4*reg + 16*tile}: the model formula, the row mean and the row norm are
// then computed in registers with two cross-lane adds, and the tile is stored straight into
// the [S][128] layout the K3 sweep streams.  Z and Theta are staged through LDS in D-chunks
// (coalesced global loads, register prefetch of the next chunk while the MFMAs of the current
// one run).  Algorithmic traffic per tile: 8*128*Dz B read + 8*128*S B written.
//
// Formula sources (expression order kept, -ffp-contract=off):
//   model_linreg.py:4-10 / model_neurlinr.py:90-97,102-110 / model_lr.py:72-86 / gaussian.py:7-15,34-62
#include "bc_internal.h"
#include "bc_np_exp.h"
#include "bc_np_pow2.h"
#include "bc_layout.h"
#include "bc_k1_math.h"
#include "../../include/beta_cores_f32.h"
#include "../../include/beta_cores_betagrad.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

// the kernels (k_project, k_project_r) and their launch tables: instantiated for float64 rows here, for float32 rows in
// bc_project_f32.hip
#include "bc_project_k1.h"

// S > 256, second stage: centre the rows of one tile (subtract the mean over all s_total samples; constant
// rows get NumPy's rounded mean, see bc_np_sum_const_*), write them back, emit the row norms and the tile's column partial sums.
__global__ __launch_bounds__(256) void k_center_tiles(double* __restrict__ tiles, double* __restrict__ norms,
                                                     double* __restrict__ tile_part, long long n_rows, int S) {
  __shared__ double lds[32 * (BC_TILE + 1)];
  const long long t = blockIdx.x;
  double* tp = tiles + (size_t)t * S * BC_TILE;
  const int tid = threadIdx.x, r = tid & (BC_TILE - 1), half = tid >> 7;   // two threads per row: even / odd chunks of 32 samples
  const bool live = t * BC_TILE + r < n_rows;
  __shared__ double psum[256], pmin[256], pmax[256];
  double sum = 0., vmin = INFINITY, vmax = -INFINITY;
  for (int s = half; s < S; s += 2) {
    const double v = tp[(size_t)s * BC_TILE + r];
    sum += v;
    vmin = fmin(vmin, v);
    vmax = fmax(vmax, v);
  }
  psum[tid] = sum; pmin[tid] = vmin; pmax[tid] = vmax;
  __syncthreads();
  const double tot = psum[r] + psum[128 + r];
  const double mn = fmin(pmin[r], pmin[128 + r]), mx = fmax(pmax[r], pmax[128 + r]);
  const double mean = ((mn == mx) ? bc_np_sum_const_any(mx, S) : tot) / (double)S;   // constant row: NumPy's rounding of the mean
  __syncthreads();
  double sq = 0.;
  for (int s0 = 0; s0 < S; s0 += 32) {
    const int kc = (S - s0) < 32 ? (S - s0) : 32;
    for (int k = half; k < kc; k += 2) {
      double v = tp[(size_t)(s0 + k) * BC_TILE + r];
      v = live ? v - mean : 0.;
      tp[(size_t)(s0 + k) * BC_TILE + r] = v;
      lds[k * (BC_TILE + 1) + r] = v;
      sq = fma(v, v, sq);
    }
    __syncthreads();
    if (tid < kc) {
      double acc = 0.0;
      for (int rr = 0; rr < BC_TILE; ++rr) acc += lds[tid * (BC_TILE + 1) + rr];
      tile_part[(size_t)t * S + s0 + tid] = acc;
    }
    __syncthreads();
  }
  psum[tid] = sq;
  __syncthreads();
  if (tid < BC_TILE) norms[t * BC_TILE + tid] = sqrt(psum[tid] + psum[128 + tid]);
}

// x^T Siginv x per row, in the reference's order: (x * (x.dot(Siginv))).sum(axis=1)   (gaussian.py:10).
// Siginv is staged in LDS when it fits (use_lds), otherwise read through the caches (wave-uniform loads).
template <typename ZT>      // the rows' storage type (float rows are widened as they are read)
__global__ __launch_bounds__(256) void k_row_quadform(const ZT* __restrict__ z, long long n_rows, int d,
                                                     const double* __restrict__ siginv, double* __restrict__ out,
                                                     int use_lds) {
  extern __shared__ double sl[];   // Siginv [d][d] when use_lds
  const double* __restrict__ sg = siginv;
  if (use_lds) {
    for (int i = threadIdx.x; i < d * d; i += blockDim.x) sl[i] = siginv[i];
    __syncthreads();
    sg = sl;
  }
  for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < n_rows; r += (long long)gridDim.x * blockDim.x) {
    const ZT* x = z + (size_t)r * d;
    double tot = 0.;
    for (int aa = 0; aa < d; ++aa) {
      double t = 0.;
      for (int bb = 0; bb < d; ++bb) t = fma((double)x[bb], sg[bb * d + aa], t);
      tot += (double)x[aa] * t;
    }
    out[r] = tot;
  }
}

// ------------------------------------------------------------------ host side
static int bc_project_wide(bc_ctx* ctx, const bc_data* data, int model, const double* theta, int32_t s,
                           const double* params, int32_t n_params, int64_t row_offset, bc_phi** inout);

static int grow_pinned(bc_ctx* ctx, size_t need) {
  if (need <= ctx->proj_pinned_cap) return BC_OK;
  BC_HIP(hipStreamSynchronize(ctx->stream));
  if (ctx->proj_pinned) (void)hipHostFree(ctx->proj_pinned);
  ctx->proj_pinned = nullptr;
  ctx->proj_pinned_cap = 0;
  BC_HIP(hipHostMalloc((void**)&ctx->proj_pinned, need * sizeof(double), hipHostMallocDefault));
  ctx->proj_pinned_cap = need;
  return BC_OK;
}

// model constants, evaluated in the same expression order as the Python sources
int bc_proj_model_constants(int model, const double* p, int np, int d, double* c, const double** siginv) {
  const double pi = 3.141592653589793;
  *siginv = nullptr;
  memset(c, 0, 8 * sizeof(double));
  switch (model) {
    case BC_MODEL_LINREG_LL: {
      if (np != 1) return BC_INVALID_ARGUMENT;
      const double sigsq = p[0];
      c[0] = -1. / 2. * log(2. * pi * sigsq);
      c[1] = 1. / (2. * sigsq);
      return BC_OK;
    }
    case BC_MODEL_LINREG_BETA: {
      if (np != 2) return BC_INVALID_ARGUMENT;
      const double sigsq = p[0], beta = p[1];
      c[0] = 1. / pow(2 * pi * sigsq, beta / 2.);
      c[1] = -(beta + 1.) / beta;
      c[2] = -beta / (2. * sigsq);
      c[3] = 1. / sqrt(1. + beta);
      return BC_OK;
    }
    case BC_MODEL_LOGISTIC_LL:
      return np == 0 ? BC_OK : BC_INVALID_ARGUMENT;
    case BC_MODEL_LOGISTIC_BETA: {
      // params = [beta] or [beta, value of the beta-likelihood at m = 0 with the caller's np.power bits] (see
      // bc_model_value_np); without the second one the library evaluates that value itself with the restated np.power
      if (np != 1 && np != 2) return BC_INVALID_ARGUMENT;
      const double beta = p[0];
      if (!(beta <= BC_K1_POWTAB_MAX_BETA)) {
        bc_set_error("bc_project: the logistic beta-likelihood takes 0 < beta <= %g on the device (got %g)", BC_K1_POWTAB_MAX_BETA, beta);
        return BC_INVALID_ARGUMENT;
      }
      c[0] = (beta + 1.) / beta;
      {
        double k[6];
        bc_powtab_coefs(-beta, &k);        // (1 + t)^-beta to t^6: c[1] = -beta, c[4..7], c[2]
        c[1] = k[0];
        c[4] = k[1];
        c[5] = k[2];
        c[6] = k[3];
        c[7] = k[4];
        c[2] = k[5];
      }
      if (np == 2) {
        c[3] = p[1];
      } else {
        // no constant from the caller: the reference's expression at m = 0 with np.power's bits at base 2 restated
        // (bc_np_pow2.h: what NumPy computes on AVX-512 hosts, the hosts the goldens come from)
        int cov1 = 0, cov2 = 0;
        double p1 = bc_np_pow2(-beta, &cov1), p2 = bc_np_pow2(-beta - 1., &cov2);
        if (!cov1) p1 = pow(2., -beta);
        if (!cov2) p2 = pow(2., -beta - 1.);
        c[3] = -(((beta + 1.) / beta) * p1 - (p2 + p2));
      }
      return BC_OK;
    }
    case BC_MODEL_GAUSS_LL: {
      if (np != 1 + d * d) return BC_INVALID_ARGUMENT;
      const double logdet = p[0];
      c[0] = -(double)d / 2 * log(2 * pi) - 1. / 2. * logdet;
      *siginv = p + 1;
      return BC_OK;
    }
    case BC_MODEL_GAUSS_BETA:
    case BC_MODEL_GAUSS_BETA_GRAD: {
      if (np != 2 + d * d) return BC_INVALID_ARGUMENT;
      const double beta = p[0], logdet = p[1], dd = (double)d;
      c[0] = 1. / beta;
      c[1] = -.5 * beta;
      c[2] = pow(1 + beta, -.5 * dd - 1);
      c[3] = log(pow(2 * pi, -.5 * dd) * pow(exp(logdet), -.5));
      c[4] = 1. / pow(beta, 2);
      c[5] = 1. / (2. * beta);
      c[6] = pow(1 + beta, -.5 * dd - 1.) * log(1. + beta);
      *siginv = p + 2;
      return BC_OK;
    }
    case BC_MODEL_LINREG_BETA_GRAD: {      // (k0 + k1 q) exp(k2 q) - k3: bc_k1_math.h
      if (np != 2) return BC_INVALID_ARGUMENT;
      bc_linreg_beta_grad_consts(p[0], p[1], c);
      return BC_OK;
    }
    case BC_MODEL_LOGISTIC_BETA_GRAD: {    // params as LOGISTIC_BETA takes them: [beta] or [beta, its constant at m = 0 (ignored)]
      if (np != 1 && np != 2) return BC_INVALID_ARGUMENT;
      const double beta = p[0];
      if (!(beta <= BC_K1_POWTAB_MAX_BETA)) {      // the value model's range, kept
        bc_set_error("bc_project: the logistic beta-gradient takes 0 < beta <= %g on the device (got %g)", BC_K1_POWTAB_MAX_BETA, beta);
        return BC_INVALID_ARGUMENT;
      }
      bc_logistic_beta_grad_consts(beta, c);
      return BC_OK;
    }
  }
  return BC_INVALID_ARGUMENT;
}

// rows [row0, row0 + rows) of `data` as the kernels' untyped base pointer
static const void* data_rows_at(const bc_data* data, int64_t row0) {
  return reinterpret_cast<const char*>(data->z) + (size_t)row0 * data->dz * data->elem;
}

// the K1 launch tables: float64 rows here, float32 rows in bc_project_f32.hip
static int k1_launch(bc_ctx* ctx, const bc_data* data, const ProjArgs& a, int kind, long long count, int model, int ntsel) {
  return data->elem == 4 ? bc_k1_launch_f32(ctx, a, kind, count, model, ntsel) : bc_k1_launch<double>(ctx, a, kind, count, model, ntsel);
}

// x^T Siginv x of rows [row0, row0 + rows) -> out[0 .. rows)
static int launch_quadform(bc_ctx* ctx, const bc_data* data, int64_t row0, int64_t rows, int d, const double* siginv_dev, double* out) {
  const int use_lds = (size_t)d * d * sizeof(double) <= 60 * 1024;
  long long blocks = (rows + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  const size_t lds = use_lds ? (size_t)d * d * sizeof(double) : 0;
  const void* z = data_rows_at(data, row0);
  if (data->elem == 4)
    hipLaunchKernelGGL(k_row_quadform<float>, dim3((unsigned)blocks), dim3(256), lds, ctx->stream, (const float*)z, (long long)rows, d, siginv_dev, out, use_lds);
  else
    hipLaunchKernelGGL(k_row_quadform<double>, dim3((unsigned)blocks), dim3(256), lds, ctx->stream, (const double*)z, (long long)rows, d, siginv_dev, out, use_lds);
  BC_HIP(hipGetLastError());
  return BC_OK;
}

// ---- a projection in two steps, the plan and the launches that use it: struct ProjPlan, bc_project_plan.h
bool bc_proj_model_has_y(int model) { return model == BC_MODEL_LINREG_LL || model == BC_MODEL_LINREG_BETA || model == BC_MODEL_LINREG_BETA_GRAD; }
// the beta-gradients of the regression models: materialising projections only (include/beta_cores_betagrad.h)
bool bc_proj_model_store_only(int model) { return model == BC_MODEL_LINREG_BETA_GRAD || model == BC_MODEL_LOGISTIC_BETA_GRAD; }

// the zero-padded Theta [NRsel][dk] (and saux [NRsel]) a single pass over s samples of dimension d reads, and the K1
// instantiation (NTsel sample tiles) that reads it
void bc_proj_theta_layout(int s, int d, bool raw, int* NTsel_out, int* NRsel_out, int* dk_out) {
  const int nt = (s + 15) / 16;
  static const int no_tail = getenv("BC_K1_NOTAIL") ? atoi(getenv("BC_K1_NOTAIL")) : 0;
  const bool tail = !raw && s > 96 && s <= 100 && !no_tail;      // 6 MFMA tiles + one sample quad
  const int NTsel = raw ? 16 : tail ? 6 : nt <= 4 ? 4 : nt <= 7 ? 7 : nt <= 13 ? 13 : 16;
  const int NRsel = NTsel * 16 + (tail ? 4 : 0);                 // rows of the zero-padded Theta / saux
  const int KC = NTsel <= 7 ? 32 : 16;
  *NTsel_out = NTsel;
  *NRsel_out = NRsel;
  *dk_out = ((d + KC - 1) / KC) * KC;
}

// the model's constants and, where the host has evaluated them for exactly this model and these parameters, the constants of
// the all-zero-feature rows, into the launch arguments (every plan starts here: plan_stage, bc_vi_plan_create)
int bc_proj_plan_constants(bc_ctx* ctx, int model, const double* params, int32_t n_params, int d, ProjArgs* a, const double** siginv) {
  if (bc_proj_model_constants(model, params, n_params, d, a->c, siginv) != BC_OK) {
    bc_set_error("bc_project: model %d expects a different number of parameters than %d (d = %d)", model, n_params, d);
    return BC_INVALID_ARGUMENT;
  }
  if (ctx->n_const_rows > 0 && ctx->const_model == model && ctx->const_n_params == n_params &&
      memcmp(ctx->const_params, params, (size_t)n_params * sizeof(double)) == 0) {
    a->ck = ctx->const_rows.p;                  // host-evaluated constants for exactly this model and these parameters
    a->cv = ctx->const_rows.p + ctx->n_const_rows;
    a->nck = (int)ctx->n_const_rows;
  }
  return BC_OK;
}

// where a plan's Theta is, and what a launch needs to know of it (the tail of every plan)
void bc_proj_plan_bind(ProjPlan* pl, int model, int32_t s, int d, int dk, int NTsel, int NRsel, bool raw, const double* theta_dev,
                      const double* siginv_dev) {
  ProjArgs& a = pl->a;
  a.theta = theta_dev;
  a.saux = theta_dev + (size_t)NRsel * dk;
  a.d = d;
  a.dk = dk;
  a.s = s;
  a.model = model;
  pl->model = model;
  pl->s = s;
  pl->d = d;
  pl->ntsel = NTsel;
  pl->raw = raw;
  pl->siginv_dev = siginv_dev;
}

// `extra` (optional): further host arrays shipped in the same transfer (bc_vi_gradient: the coreset rows and their
// weights); extra_dev[i] receives the device address of extra_src[i].  ONE pinned staging area, ONE device buffer, ONE
// hipMemcpyAsync per plan: a copy call costs ~5 us of host time, a gradient step of the 1M-row configuration 350.
int bc_proj_plan_stage(bc_ctx* ctx, int model, const double* theta, int32_t s, const double* params, int32_t n_params,
                      int dz, bool raw, ProjPlan* pl, int n_extra, const double* const* extra_src, const size_t* extra_n,
                      double** extra_dev) {
  if (s <= 0 || s > 256) { bc_set_error("bc_project: internal: a single pass handles 1..256 samples"); return BC_INVALID_ARGUMENT; }
  const int d = dz - (bc_proj_model_has_y(model) ? 1 : 0);
  if (d <= 0) { bc_set_error("bc_project: data rows too short for this model"); return BC_INVALID_ARGUMENT; }
  ProjArgs& a = pl->a;
  memset(&a, 0, sizeof(a));
#ifdef BC_K1_STAMPS
  a.stamps = getenv("BC_K1_STAMP_PTR") ? (unsigned long long*)strtoull(getenv("BC_K1_STAMP_PTR"), nullptr, 10) : nullptr;
#endif
  const double* siginv = nullptr;
  if (bc_proj_plan_constants(ctx, model, params, n_params, d, &a, &siginv) != BC_OK) return BC_INVALID_ARGUMENT;
  int NTsel, NRsel, dk;
  bc_proj_theta_layout(s, d, raw, &NTsel, &NRsel, &dk);
  const size_t th_n = (size_t)NRsel * dk, sa_n = (size_t)NRsel, sg_n = siginv ? (size_t)d * d : 0;
  const size_t head_n = (th_n + sa_n + sg_n + 1) & ~(size_t)1;
  size_t total = head_n;
  for (int i = 0; i < n_extra; ++i) total += (extra_n[i] + 1) & ~(size_t)1;      // 16-byte aligned pieces
  int rc = bc_scratch_grow(ctx, &ctx->proj_theta, total);
  if (!rc) rc = grow_pinned(ctx, total);
  if (rc) return rc;
  // make sure an earlier launch is no longer reading the pinned staging area
  BC_HIP(hipStreamSynchronize(ctx->stream));
  double* hth = ctx->proj_pinned;
  double* hsa = ctx->proj_pinned + th_n;
  memset(hth, 0, (th_n + sa_n) * sizeof(double));
  if (siginv) {
    // Theta' = (Siginv . Theta^T)^T  so that the contraction yields x^T Siginv theta (gaussian.py:12),
    // tSt = (th * (th.dot(Siginv))).sum(axis=1)                                       (gaussian.py:11)
    for (int q = 0; q < s; ++q) {
      const double* th = theta + (size_t)q * d;
      double tst = 0.;
      for (int aa = 0; aa < d; ++aa) {
        double m1 = 0., m2 = 0.;
        for (int bb = 0; bb < d; ++bb) {
          m1 += siginv[(size_t)aa * d + bb] * th[bb];   // (Siginv . th^T)[aa]
          m2 += th[bb] * siginv[(size_t)bb * d + aa];   // (th . Siginv)[aa]
        }
        hth[(size_t)q * dk + aa] = m1;
        tst += th[aa] * m2;
      }
      hsa[q] = tst;
    }
    memcpy(ctx->proj_pinned + th_n + sa_n, siginv, sg_n * sizeof(double));
  } else {
    for (int q = 0; q < s; ++q) memcpy(hth + (size_t)q * dk, theta + (size_t)q * d, (size_t)d * sizeof(double));
  }
  size_t off = head_n;
  for (int i = 0; i < n_extra; ++i) {
    memcpy(ctx->proj_pinned + off, extra_src[i], extra_n[i] * sizeof(double));
    extra_dev[i] = ctx->proj_theta.p + off;
    off += (extra_n[i] + 1) & ~(size_t)1;
  }
  BC_HIP(hipMemcpyAsync(ctx->proj_theta.p, ctx->proj_pinned, total * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  bc_proj_plan_bind(pl, model, s, d, dk, NTsel, NRsel, raw, ctx->proj_theta.p, siginv ? ctx->proj_theta.p + th_n + sa_n : nullptr);      // (th_n = NRsel * dk)
  return BC_OK;
}

// The resident kernel serves large shards whose Theta fits one CU's LDS next to the per-wave scratch: at least 8 tiles
// per wave slot of the grid (tile_part then has room for the per-wave partial rows, and the grid is full), S <= 112.
// BC_K1_STAGED=1 forces the staged kernel (A/B measurements).
static bool bc_model_has_np_exp_rt(int model) { return model == BC_MODEL_LINREG_BETA || model == BC_MODEL_GAUSS_BETA || model == BC_MODEL_GAUSS_BETA_GRAD; }

static int project_r_grid(const bc_ctx* ctx, const ProjPlan& pl, const bc_phi* phi, int mode) {
  const char* env = getenv("BC_K1_STAGED");          // read per call: tests toggle it inside one process
  if ((env && atoi(env) > 0) || mode == PROJ_RAW) return 0;
  if (pl.ntsel != 4 && pl.ntsel != 6 && pl.ntsel != 7) return 0;
  // S in 101..112 with an exp in the epilogue: those three instantiations need 4-6 VGPRs more than the 256 a wave of a
  // 512-thread block may hold (they would spill): the staged kernel serves them
  // (the two regression beta-gradients have no resident instantiation there either: launch_project_r_nt)
  if (pl.ntsel == 7 && (bc_model_has_np_exp_rt(pl.model) || bc_proj_model_store_only(pl.model))) return 0;
  if (pl.model == BC_MODEL_LOGISTIC_BETA && !(env && atoi(env) < 0)) return 0;      // measured slower there (0.80 vs 0.74 ms at N = 1M, D = 128): four
                                                                                       // transcendental bodies per element; BC_K1_STAGED=-1 forces the resident kernel
  const int nr = pl.ntsel * 16 + (pl.ntsel == 6 ? 4 : 0);
  if (project_r_lds_bytes(nr, pl.a.dk, BC_K1_TAB_DOUBLES + 264) > (size_t)ctx->max_lds) return 0;
  const long long grid = ctx->n_cu;
  if (phi->ntiles < grid * 8) return 0;
  return (int)grid;
}

// One launch of a staged projection over `data`'s rows.  mode PROJ_FULL: the whole of Phi (s == s_total <= 256),
// centred, with norms and column partials.  PROJ_RAW: samples [s_off, s_off + s) of s_total, un-centred.
// PROJ_COLSUM: `phi` is a stats-only Phi: column partials only.  rowaux: the scratch that receives x^T Siginv x.
int bc_proj_plan_launch(bc_ctx* ctx, const ProjPlan& pl, const bc_data* data, bc_phi* phi, int mode, int32_t s_total,
                       int32_t s_off, bc_scratch* rowaux) {
  ProjArgs a = pl.a;
  a.rowaux = nullptr;
  if (pl.siginv_dev && data->n_rows > 0) {
    int rc = bc_scratch_grow(ctx, rowaux, (size_t)data->n_rows);
    if (rc) return rc;
    rc = launch_quadform(ctx, data, 0, data->n_rows, pl.d, pl.siginv_dev, rowaux->p);
    if (rc) return rc;
    a.rowaux = rowaux->p;
  }
  a.z = data_rows_at(data, 0);
  a.tiles = phi->tiles;
  a.norms = phi->norms;
  a.tile_part = phi->tile_part;
  a.n_rows = data->n_rows;
  a.dz = data->dz;
  a.s_total = s_total;
  a.s_off = s_off;
  if (phi->ntiles <= 0) {
    if (phi->norms) BC_HIP(hipMemsetAsync(phi->norms, 0, BC_TILE * sizeof(double), ctx->stream));
    return BC_OK;
  }
  int rc = bc_timer_begin(ctx, 1);
  if (rc) return rc;
  const int rgrid = project_r_grid(ctx, pl, phi, mode);
  phi->part_rows = phi->ntiles;                 // rows of tile_part this launch fills (one per tile, or one per wave)
  if (rgrid > 0) {
    a.ngroups = (data->n_rows + 31) / 32;
    phi->part_rows = (int64_t)rgrid * 8;
    rc = k1_launch(ctx, data, a, mode == PROJ_COLSUM ? BC_K1_RESIDENT_COLSUM : BC_K1_RESIDENT_FULL, rgrid, pl.model, pl.ntsel);
  } else {
    rc = k1_launch(ctx, data, a, mode == PROJ_RAW ? BC_K1_STAGED_RAW : mode == PROJ_COLSUM ? BC_K1_STAGED_COLSUM : BC_K1_STAGED_FULL,
                   phi->ntiles, pl.model, pl.ntsel);
  }
  if (!rc) rc = bc_timer_end(ctx, 1);
  return rc;
}

int bc_proj_project_check(bc_ctx* ctx, const bc_data* data, int model, const double* theta, int32_t s,
                         const double* params, int32_t n_params, const char* who) {
  if (!ctx || !data || !theta || s <= 0 || (n_params > 0 && !params)) { bc_set_error("%s: bad argument", who); return BC_INVALID_ARGUMENT; }
  if (data->ctx != ctx) { bc_set_error("%s: data belongs to another context", who); return BC_INVALID_ARGUMENT; }
  if (model < 0 || model > BC_MODEL_LOGISTIC_BETA_GRAD) { bc_set_error("%s: unknown model %d", who, model); return BC_INVALID_ARGUMENT; }
  return BC_OK;
}

// raw == false: the whole of Phi (s == s_total <= 256).  raw == true: samples [s_off, s_off + s) of s_total, un-centred.
static int project_impl(bc_ctx* ctx, const bc_data* data, int model, const double* theta, int32_t s,
                        const double* params, int32_t n_params, int64_t row_offset, bc_phi** inout,
                        int32_t s_total, int32_t s_off, bool raw) {
  int rc = bc_proj_project_check(ctx, data, model, theta, s, params, n_params, "bc_project");
  if (rc) return rc;
  if (!inout) { bc_set_error("bc_project: bad argument"); return BC_INVALID_ARGUMENT; }
  BC_HIP(hipSetDevice(ctx->device));
  ProjPlan pl;
  rc = bc_proj_plan_stage(ctx, model, theta, s, params, n_params, data->dz, raw, &pl);
  if (rc) return rc;
  // output handle: reuse buffers when the shape matches
  bc_phi* phi = *inout;
  if (phi && (phi->ctx != ctx || phi->s != s_total || !phi->tiles || bc_phi_set_rows(phi, data->n_rows) != 0)) {
    bc_set_error("bc_project: *inout has a different S or too little row capacity; pass NULL to allocate");
    return BC_INVALID_ARGUMENT;
  }
  bool fresh = false;
  if (!phi) {
    rc = bc_phi_alloc(ctx, data->n_rows, s_total, row_offset, &phi);
    if (rc) return rc;
    fresh = true;
  }
  phi->row_offset = row_offset;
  phi->stats_valid = false;
  rc = bc_proj_plan_launch(ctx, pl, data, phi, raw ? PROJ_RAW : PROJ_FULL, s_total, s_off, &ctx->proj_rowaux);
  if (!rc && !raw) rc = bc_phi_finish_stats(phi);
  if (rc) { if (fresh) bc_phi_destroy(phi); return rc; }
  *inout = phi;
  return BC_OK;
}

// S > 256: passes of <= 256 samples write un-centred values, then one centring pass over Phi.
static int bc_project_wide(bc_ctx* ctx, const bc_data* data, int model, const double* theta, int32_t s,
                           const double* params, int32_t n_params, int64_t row_offset, bc_phi** inout) {
  const int d = data->dz - (bc_proj_model_has_y(model) ? 1 : 0);
  bc_phi* phi = *inout;
  const bool fresh = phi == nullptr;
  for (int s_off = 0; s_off < s; s_off += 256) {
    const int cs = (s - s_off) < 256 ? (s - s_off) : 256;
    int rc = project_impl(ctx, data, model, theta + (size_t)s_off * d, cs, params, n_params, row_offset, &phi, s, s_off, true);
    if (rc) { if (fresh && phi) bc_phi_destroy(phi); return rc; }
  }
  if (phi->ntiles > 0) {
    hipLaunchKernelGGL(k_center_tiles, dim3((unsigned)phi->ntiles), dim3(256), 0, ctx->stream, phi->tiles, phi->norms,
                       phi->tile_part, (long long)phi->n_rows, s);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { if (fresh) bc_phi_destroy(phi); return bc_hip_fail(e, "k_center_tiles", __FILE__, __LINE__); }
  }
  int rc = bc_phi_finish_stats(phi);
  if (rc) { if (fresh) bc_phi_destroy(phi); return rc; }
  *inout = phi;
  return BC_OK;
}

extern "C" int bc_project(bc_ctx* ctx, const bc_data* data, int model, const double* theta, int32_t s,
                          const double* params, int32_t n_params, int64_t row_offset, bc_phi** inout) {
  int rc = bc_proj_project_check(ctx, data, model, theta, s, params, n_params, "bc_project");
  if (rc) return rc;
  if (!inout) { bc_set_error("bc_project: bad argument"); return BC_INVALID_ARGUMENT; }
  if (s > 256) return bc_project_wide(ctx, data, model, theta, s, params, n_params, row_offset, inout);
  return project_impl(ctx, data, model, theta, s, params, n_params, row_offset, inout, s, 0, false);
}

// ---- constant rows with the CALLER's bits (hosts whose NumPy does not evaluate np.exp with the SVML routine bc_np_exp.h
// restates: the reference's own bits for a constant row's value are then NumPy's on THAT host).
// A data row with all-zero features projects to S equal values that depend on its y alone (model_neurlinr.py:102-110 with
// x = 0); the host layer finds those rows (bc_data_zero_feature_keys), evaluates the reference's expression for their y's
// with its own NumPy and hands (y, value) pairs over; K1's constant-row branch then takes the value from here.
template <typename ZT>
__global__ __launch_bounds__(256) void k_zero_feature_keys(const ZT* __restrict__ z, long long n_rows, int dz, int d,
                                                          double* __restrict__ out, unsigned long long* __restrict__ count,
                                                          long long cap) {
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rows) return;
  const ZT* row = z + (size_t)r * dz;
  for (int k = 0; k < d; ++k)
    if (row[k] != (ZT)0) return;                   // (almost every row leaves at k = 0)
  const unsigned long long slot = atomicAdd(count, 1ull);
  if ((long long)slot < cap) out[slot] = (double)row[d];
}

extern "C" int bc_data_zero_feature_keys(const bc_data* data, int32_t d, int64_t cap, double* out_keys, int64_t* out_n) {
  if (!data || !out_n || d <= 0 || d >= data->dz || cap < 0 || (cap > 0 && !out_keys)) {
    bc_set_error("bc_data_zero_feature_keys: bad argument");
    return BC_INVALID_ARGUMENT;
  }
  bc_ctx* ctx = data->ctx;
  *out_n = 0;
  if (data->n_rows == 0) return BC_OK;
  BC_HIP(hipSetDevice(ctx->device));
  int rc = bc_scratch_grow(ctx, &ctx->proj_rowaux2, (size_t)cap + 2);
  if (rc) return rc;
  double* buf = ctx->proj_rowaux2.p;
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(buf + cap);
  BC_HIP(hipMemsetAsync(cnt, 0, sizeof(unsigned long long), ctx->stream));
  const dim3 zgrid((unsigned)((data->n_rows + 255) / 256));
  if (data->elem == 4)
    hipLaunchKernelGGL(k_zero_feature_keys<float>, zgrid, dim3(256), 0, ctx->stream, bc_rows<float>(data), (long long)data->n_rows, data->dz, d, buf, cnt, (long long)cap);
  else
    hipLaunchKernelGGL(k_zero_feature_keys<double>, zgrid, dim3(256), 0, ctx->stream, bc_rows<double>(data), (long long)data->n_rows, data->dz, d, buf, cnt, (long long)cap);
  BC_HIP(hipGetLastError());
  unsigned long long n = 0;
  BC_HIP(hipMemcpyAsync(&n, cnt, sizeof(n), hipMemcpyDeviceToHost, ctx->stream));
  BC_HIP(hipStreamSynchronize(ctx->stream));
  *out_n = (int64_t)n;                          // may exceed cap: the caller then knows the list is truncated
  const int64_t take = (int64_t)n < cap ? (int64_t)n : cap;
  if (take > 0) {
    BC_HIP(hipMemcpyAsync(out_keys, buf, (size_t)take * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    BC_HIP(hipStreamSynchronize(ctx->stream));
  }
  return BC_OK;
}

extern "C" int bc_ctx_set_constant_row_values(bc_ctx* ctx, int model, const double* params, int32_t n_params, const double* keys,
                                              const double* values, int64_t n) {
  if (!ctx || n < 0 || (n > 0 && (!keys || !values || !params)) || n_params < 0 || n_params > 4) {
    bc_set_error("bc_ctx_set_constant_row_values: bad argument");
    return BC_INVALID_ARGUMENT;
  }
  if (n == 0) { ctx->n_const_rows = 0; ctx->const_model = -1; return BC_OK; }
  if (model != BC_MODEL_LINREG_BETA) {
    bc_set_error("bc_ctx_set_constant_row_values: only the linear-regression beta-likelihood takes host-evaluated constants");
    return BC_INVALID_ARGUMENT;
  }
  for (int64_t i = 1; i < n; ++i)
    if (!(keys[i - 1] < keys[i])) { bc_set_error("bc_ctx_set_constant_row_values: keys must be strictly increasing"); return BC_INVALID_ARGUMENT; }
  BC_HIP(hipSetDevice(ctx->device));
  BC_HIP(hipStreamSynchronize(ctx->stream));    // no launch in flight may still read the old table
  int rc = bc_scratch_grow(ctx, &ctx->const_rows, (size_t)(2 * n));
  if (rc) return rc;
  BC_HIP(hipMemcpyAsync(ctx->const_rows.p, keys, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  BC_HIP(hipMemcpyAsync(ctx->const_rows.p + n, values, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  BC_HIP(hipStreamSynchronize(ctx->stream));    // the host arrays are only borrowed for the call
  ctx->n_const_rows = n;
  ctx->const_model = model;
  ctx->const_n_params = n_params;
  memcpy(ctx->const_params, params, (size_t)n_params * sizeof(double));
  return BC_OK;
}

// ---------------------------------------------------------------------------------------------
// Host rows -> Phi, pipelined (hilbert.py:11-17 and bcores.py:44 hand the projector HOST arrays): the rows are uploaded in
// chunks (bc_upload.hip) and K1 runs on chunk c behind the event that marks its arrival while chunks c+1.. are still on
// the wire.  Rows are independent, so Phi and the norms are the resident path's bit for bit; the column sums too, because
// the chunks keep the partial sums' association: the staged kernel writes one partial row per 128-row tile (chunks are
// tile-aligned), the Theta-resident kernel's per-wave partials are CONTINUED from chunk to chunk (ProjArgs::part_init;
// chunks start at multiples of 8 * n_cu groups = 65 536 rows, so every wave adds the same groups in the same order as in
// one launch over all rows).  Which of the two kernels runs is decided once, from the total row count, exactly as
// bc_project decides it.  *out_data receives the resident rows (the caller keeps or destroys them).
static int launch_chunk(bc_ctx* ctx, const ProjPlan& pl, const bc_data* data, bc_phi* phi, int64_t row0, int64_t rows, int rgrid,
                        bool first, bc_scratch* rowaux) {
  ProjArgs a = pl.a;
  a.rowaux = nullptr;
  if (pl.siginv_dev) {
    int rc = launch_quadform(ctx, data, row0, rows, pl.d, pl.siginv_dev, rowaux->p + row0);
    if (rc) return rc;
    a.rowaux = rowaux->p + row0;
  }
  const int64_t tile0 = row0 / BC_TILE, ntiles = (rows + BC_TILE - 1) / BC_TILE;
  a.z = data_rows_at(data, row0);
  a.tiles = phi->tiles + (size_t)tile0 * phi->s * BC_TILE;
  a.norms = phi->norms + row0;
  a.n_rows = rows;
  a.dz = data->dz;
  a.s_total = phi->s;
  a.s_off = 0;
  // timer class 1 (K1), one span per chunk launch: recorded on ctx->stream behind the wait for the chunk's arrival, so the
  // span is the kernel, not the transfer it waited for
  int rc = bc_timer_begin(ctx, 1);
  if (rc) return rc;
  if (rgrid > 0) {
    a.tile_part = phi->tile_part;                 // one row per wave, shared by all chunks
    a.part_init = first ? 0 : 1;
    a.ngroups = (rows + 31) / 32;
    rc = k1_launch(ctx, data, a, BC_K1_RESIDENT_FULL, rgrid, pl.model, pl.ntsel);
  } else {
    a.tile_part = phi->tile_part + (size_t)tile0 * phi->s;
    rc = k1_launch(ctx, data, a, BC_K1_STAGED_FULL, ntiles, pl.model, pl.ntsel);
  }
  if (!rc) rc = bc_timer_end(ctx, 1);
  return rc;
}

// elem: bytes per element of z_host and of the resident copy it becomes (8 or 4); `who`: the entry point's name
static int project_from_host(bc_ctx* ctx, const void* z_host, int elem, const char* who, int64_t n_rows, int32_t dz, int model,
                             const double* theta, int32_t s, const double* params, int32_t n_params, int64_t row_offset,
                             bc_data** out_data, bc_phi** inout) {
  if (!ctx || !z_host || n_rows <= 0 || dz <= 0 || !theta || s <= 0 || !out_data || !inout || (n_params > 0 && !params)) {
    bc_set_error("%s: bad argument", who);
    return BC_INVALID_ARGUMENT;
  }
  if (model < 0 || model > BC_MODEL_LOGISTIC_BETA_GRAD) { bc_set_error("%s: unknown model %d", who, model); return BC_INVALID_ARGUMENT; }
  BC_HIP(hipSetDevice(ctx->device));
  bc_data* data = new bc_data();
  data->ctx = ctx;
  data->n_rows = n_rows;
  data->dz = dz;
  data->cap_rows = n_rows;
  data->elem = elem;
  const size_t row_bytes = (size_t)dz * elem;
  {
    hipError_t e = hipMalloc((void**)&data->z, (size_t)n_rows * row_bytes);
    if (e != hipSuccess) { delete data; return bc_hip_fail(e, "hipMalloc(data)", __FILE__, __LINE__); }
  }
  auto drop_data = [&]() { (void)hipStreamSynchronize(ctx->stream); (void)hipFree(data->z); delete data; };
  int rc;
  if (s > 256) {
    // the wide path makes several passes over all rows: plain (still multi-threaded) upload, then bc_project
    rc = bc_upload_rows(ctx, z_host, data->z, n_rows, row_bytes, bc_upload_default_chunk_rows(n_rows, row_bytes), nullptr);
    if (!rc) rc = bc_project_wide(ctx, data, model, theta, s, params, n_params, row_offset, inout);
    if (rc) { drop_data(); return rc; }
    *out_data = data;
    return BC_OK;
  }
  ProjPlan pl;
  rc = bc_proj_plan_stage(ctx, model, theta, s, params, n_params, dz, false, &pl);
  if (rc) { drop_data(); return rc; }
  bc_phi* phi = *inout;
  if (phi && (phi->ctx != ctx || phi->s != s || !phi->tiles || bc_phi_set_rows(phi, n_rows) != 0)) {
    bc_set_error("%s: *inout has a different S or too little row capacity; pass NULL to allocate", who);
    drop_data();
    return BC_INVALID_ARGUMENT;
  }
  bool fresh = false;
  if (!phi) {
    rc = bc_phi_alloc(ctx, n_rows, s, row_offset, &phi);
    if (rc) { drop_data(); return rc; }
    fresh = true;
  }
  phi->row_offset = row_offset;
  phi->stats_valid = false;
  if (pl.siginv_dev) {
    rc = bc_scratch_grow(ctx, &ctx->proj_rowaux, (size_t)n_rows);
    if (rc) { if (fresh) bc_phi_destroy(phi); drop_data(); return rc; }
  }
  const int rgrid = project_r_grid(ctx, pl, phi, PROJ_FULL);
  phi->part_rows = rgrid > 0 ? (int64_t)rgrid * 8 : phi->ntiles;
  // chunk = a multiple of (8 * rgrid) 32-row groups for the resident kernel, of 128-row tiles for the staged one; ~128 MiB.
  // The alignment is a number of ROWS whatever the element size (the waves' column sums keep their association), the size is bytes
  const int64_t unit = bc_lay_chunk_unit(rgrid);
  const char* env = getenv("BC_PIPE_CHUNK_ROWS");      // tests: force several chunks on small inputs
  const int64_t chunk_rows = bc_lay_chunk_rows_bytes((long long)row_bytes, unit, env ? atoll(env) : 0);
  bool first = true;
  bc_chunk_hook hook = [&](int64_t, int64_t row0, int64_t rows, hipEvent_t landed) -> int {
    if (landed) BC_HIP(hipStreamWaitEvent(ctx->stream, landed, 0));
    const int r = launch_chunk(ctx, pl, data, phi, row0, rows, rgrid, first, &ctx->proj_rowaux);
    first = false;
    return r;
  };
  rc = bc_upload_rows(ctx, z_host, data->z, n_rows, row_bytes, chunk_rows, &hook);
  if (!rc) rc = bc_phi_finish_stats(phi);
  if (rc) { if (fresh) { (void)hipStreamSynchronize(ctx->stream); bc_phi_destroy(phi); } drop_data(); return rc; }
  *inout = phi;
  *out_data = data;
  return BC_OK;
}

extern "C" int bc_project_from_host(bc_ctx* ctx, const double* z_host, int64_t n_rows, int32_t dz, int model, const double* theta,
                                    int32_t s, const double* params, int32_t n_params, int64_t row_offset, bc_data** out_data,
                                    bc_phi** inout) {
  return project_from_host(ctx, z_host, 8, "bc_project_from_host", n_rows, dz, model, theta, s, params, n_params, row_offset, out_data, inout);
}

extern "C" int bc_project_from_host_f32(bc_ctx* ctx, const float* z_host, int64_t n_rows, int32_t dz, int model, const double* theta,
                                        int32_t s, const double* params, int32_t n_params, int64_t row_offset, bc_data** out_data,
                                        bc_phi** inout) {
  return project_from_host(ctx, z_host, 4, "bc_project_from_host_f32", n_rows, dz, model, theta, s, params, n_params, row_offset, out_data, inout);
}

// ---------------------------------------------------------------------------------------------
// Store-free projection: the S column sums of the N x S projection and nothing else (why, and the fused gradient of the
// greedy-VI weight optimisation that is built on it: bc_vigrad.hip).

// the context's stats-only Phi, sized for n_rows x s
int bc_proj_colsum_phi_for(bc_ctx* ctx, int64_t n_rows, int32_t s, bc_phi** out) {
  bc_phi* p = ctx->colsum_phi;
  if (p && (p->s != s || bc_phi_set_rows(p, n_rows) != 0)) {
    BC_HIP(hipStreamSynchronize(ctx->stream));
    bc_phi_destroy(p);
    ctx->colsum_phi = p = nullptr;
  }
  if (!p) {
    int rc = bc_phi_alloc(ctx, n_rows, s, 0, &p, 0, true);
    if (rc) return rc;
    ctx->colsum_phi = p;
  }
  p->stats_valid = false;
  *out = p;
  return BC_OK;
}

extern "C" int bc_project_colsum(bc_ctx* ctx, const bc_data* data, int model, const double* theta, int32_t s,
                                 const double* params, int32_t n_params, bc_comm* comm, double* out_s) {
  int rc = bc_proj_project_check(ctx, data, model, theta, s, params, n_params, "bc_project_colsum");
  if (rc) return rc;
  if (!out_s) { bc_set_error("bc_project_colsum: bad argument"); return BC_INVALID_ARGUMENT; }
  if (bc_proj_model_store_only(model)) {
    bc_set_error("bc_project_colsum: model %d (a beta-gradient) has no store-free form: project and take bc_phi_colsum", model);
    return BC_INVALID_ARGUMENT;
  }
  if (comm && bc_comm_ctx(comm) != ctx) { bc_set_error("bc_project_colsum: the communicator belongs to another context"); return BC_INVALID_ARGUMENT; }
  if (s > 256) { bc_set_error("bc_project_colsum: at most 256 samples (S = %d): project and take bc_phi_colsum", s); return BC_INVALID_ARGUMENT; }
  BC_HIP(hipSetDevice(ctx->device));
  ProjPlan pl;
  rc = bc_proj_plan_stage(ctx, model, theta, s, params, n_params, data->dz, false, &pl);
  if (rc) return rc;
  bc_phi* phi = nullptr;
  rc = bc_proj_colsum_phi_for(ctx, data->n_rows, s, &phi);
  if (!rc) rc = bc_proj_plan_launch(ctx, pl, data, phi, PROJ_COLSUM, s, 0, &ctx->proj_rowaux);
  if (!rc) rc = bc_phi_reduce_colsum(phi);
  if (rc) return rc;
  const double* res = phi->colsum;
  if (comm) {
    rc = bc_comm_sum_dev(comm, phi->colsum, s, &res);
    if (rc) return rc;
  }
  BC_HIP(hipMemcpyAsync(ctx->pinned, res, (size_t)s * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  BC_HIP(hipStreamSynchronize(ctx->stream));
  memcpy(out_s, ctx->pinned, (size_t)s * sizeof(double));
  return BC_OK;
}
