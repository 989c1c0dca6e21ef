// The batched BatchPSVI run (include/beta_cores_psvi_many.h, begun with a kind: include/beta_cores_psvi_curve.h): the pseudo-coresets of many sizes stepped in lock-step, the host
// waiting once per chunk of steps.  Per step, on the context's stream, in order:
//
//   k_take_rows (bc_take.hip)   the step's sub-sample of the resident rows, once for the whole batch
//   k_pm_rowaux  grid tiles     Gaussian kind: x^T Siginv x of the gathered rows and of every problem's points (bc_pm_rowaux_tile)
//   k_pm_fit     grid P         logistic kind: bc_pm_fit (the mode search of bc_vi_laplace_dev.h from the problem's previous
//                               mode, one full Newton step, the factor) on (points_p, w_p), then the draw Theta_p
//   k_pm_post    grid P         Gaussian kind: bc_vi_sampler's closed-form weighted posterior of (points_p, w_p), the draw
//                               Theta_p, Theta'_p = (Siginv Theta_p^T)^T and theta^T Siginv theta
//   k_pm_ll      grid P x tiles bc_pm_ll_tile / bc_pm_gauss_tile on the fp64 matrix cores: the row tiles of the gathered rows give the target's
//                               partial sums, the tiles of the problem's own points its corevecs
//   k_pm_resid   grid P         target (partials in tile order), resid, g_w
//   k_pm_pgrad   grid sum m_p   bc_psvi_dev.h's point-gradient, one block per point
//   k_pm_adam    grid P         one partial_nn_opt step on (w_p, points_p)
//
// The state (points, weights, moments, modes) lives in device memory for the whole run -- L2-resident at the sizes of an
// evaluation curve -- and each stage stages what it needs in LDS.  Blocks never wait for each other; a block reads nothing but
// its own problem and the shared draws, so a problem's bits do not depend on P or on its place in the batch.  flag[p] != 0: an
// earlier stage marked the problem; every later launch returns at once for it.
#include "bc_internal.h"
#include "bc_project_plan.h"
#include "bc_vi_laplace_dev.h"
#include "bc_vi_sampler_dev.h"
#include "bc_psvi_dev.h"
#include "bc_psvi_many_dev.h"
#include "bc_slab.h"
#include "bc_batch.h"
#include "../../include/beta_cores_psvi_many.h"
#include "../../include/beta_cores_psvi_curve.h"
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

static_assert(BC_VI_MAX_DIM == BC_VIL_MAXD, "include/beta_cores_psvi_many.h states the Laplace fit's limit");
static_assert(BC_VI_MAX_DIM == BC_VIS_MAXD, "include/beta_cores_psvi_many.h states the closed-form posterior's limit");
static_assert(BC_PM_VIS_DOUBLES(BC_VIS_MAXD) == BC_VIS_WS_DOUBLES(BC_VIS_MAXD) && BC_PM_VIS_DOUBLES(3) == BC_VIS_WS_DOUBLES(3) &&
              BC_PM_VIS_TRI(7) == BC_VIS_TRI(7), "bc_psvi_many_dev.h restates the layout of bc_vi_sampler's work space (C | L | rhs | t | mu | sc)");
static_assert(BC_PSVI_MANY_MAX_SAMPLES <= BC_PM_BLOCK, "bc_pm_tile_colsum and bc_pm_resid give a sample to a thread");

struct PmRun {                  // the run's device pointers (by value to every kernel)
  const long long* row_ptr;     // [P + 1]
  const int* prob_of_row;       // [R]
  int* flag;                    // [P]
  int* newton;                  // [P][2]: Newton steps of the last fit | of all fits
  double *pts, *w;              // [R][d], [R]
  double *m1w, *m1p, *m2w, *m2p;
  double *gw, *gp;
  double *prev_w, *prev_p;      // the state before the last step of a chunk
  double* mode;                 // [P][d]
  double* theta;                // [P][s][d]
  double* cv;                   // [R][s]
  double* part;                 // [P][tiles][s]
  double *target, *resid;       // [P][s]
  double* rowc;                 // [3 R]
  const double* steps;          // [P][itrs]
  const double* moments;        // [2][itrs]
  const void* sub;              // the gathered rows [n_sub][d]
  int sub_elem;
  int d, s, diag, n_sub, tiles, itrs;
  double scale;
  int kind, pg_kind;            // BC_PM_LOGISTIC / BC_PM_GAUSS: what the tile evaluates; the point-gradient's BC_PSVI_* kind
  int post_chains;              // Gaussian kind: 1: bc_vi_sampler's own per-thread chains for the three products; 0: bc_pm_post_products
  // Gaussian kind
  const double *sig0inv, *b0, *siginv;      // [d][d], [d] Sig0inv . mu0, [d][d]
  double c0;                    // the model's constant (bc_proj_model_constants)
  double* raw;                  // [P][s][d] the draws Theta_p; theta holds Theta'_p
  double* sa;                   // [P][s]
  double *ra_sub, *ra_pts;      // [n_sub], [R]
};

#define BC_PM_POST_BLOCK 512

// Gaussian kind.  blockIdx.x < tiles: a tile of the gathered rows; beyond: a tile of the R packed points of all problems.
__global__ __launch_bounds__(BC_PM_BLOCK) void k_pm_rowaux(PmRun g, int n_points) {
  extern __shared__ double pm_ra_ws[];
  const int y = blockIdx.x;
  if (y < g.tiles) bc_pm_rowaux_tile(g.sub, g.sub_elem, g.n_sub, g.d, g.siginv, y, pm_ra_ws, g.ra_sub);
  else bc_pm_rowaux_tile(g.pts, 8, n_points, g.d, g.siginv, y - g.tiles, pm_ra_ws, g.ra_pts);
}

// Gaussian kind: the closed-form posterior of (points_p, w_p), its mean and the draw.
__global__ __launch_bounds__(BC_PM_POST_BLOCK) void k_pm_post(PmRun g, const double* __restrict__ E, int step, int snap) {
  extern __shared__ double pm_post_ws[];
  const int p = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, d = g.d;
  if (*(volatile int*)(g.flag + p) != 0) return;      // (block-uniform)
  const long long r0 = g.row_ptr[p];
  const int m = (int)(g.row_ptr[p + 1] - r0);
  if (snap) {
    for (int i = tid; i < m; i += nt) g.prev_w[r0 + i] = g.w[r0 + i];
    for (int e = tid; e < m * d; e += nt) g.prev_p[(size_t)r0 * d + e] = g.pts[(size_t)r0 * d + e];
  }
  VisArgs a;
  a.kind = BC_VIS_GAUSS;
  a.d = d;
  a.m = m;
  a.dz = d;
  a.s = g.post_chains ? g.s : 0;      // (no samples: the factor, L and mu only; the products follow below)
  a.dk = d;
  a.core = g.pts + (size_t)r0 * d;
  a.w = g.w + r0;
  a.sig0inv = g.sig0inv;
  a.b0 = g.b0;
  a.siginv = g.siginv;
  a.sigsq = 1.;
  a.E = E;
  a.theta = g.theta + (size_t)p * g.s * d;
  a.saux = g.sa + (size_t)p * g.s;
  a.raw = g.raw + (size_t)p * g.s * d;
  if (bc_vi_sampler(a, pm_post_ws)) {                 // (block-uniform)
    if (tid == 0) g.flag[p] = step + 1;
    return;
  }
  const double* mu = pm_post_ws + BC_PM_VIS_MU(d);
  if (!g.post_chains) {
    PmPostArgs b;
    b.d = d;
    b.s = g.s;
    b.E = E;
    b.Li = pm_post_ws + BC_PM_VIS_LI(d);
    b.mu = mu;
    b.siginv = g.siginv;
    b.raw = a.raw;
    b.thp = a.theta;
    b.sa = a.saux;
    bc_pm_post_products(b);
  }
  for (int j = tid; j < d; j += nt) g.mode[(size_t)p * d + j] = mu[j];
}

__global__ __launch_bounds__(BC_VIL_BLOCK) void k_pm_fit(PmRun g, const double* __restrict__ E, int step, int snap) {
  extern __shared__ double pm_fit_ws[];
  const int p = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, d = g.d;
  if (*(volatile int*)(g.flag + p) != 0) return;      // (block-uniform)
  const long long r0 = g.row_ptr[p];
  const int m = (int)(g.row_ptr[p + 1] - r0);
  if (snap) {
    for (int i = tid; i < m; i += nt) g.prev_w[r0 + i] = g.w[r0 + i];
    for (int e = tid; e < m * d; e += nt) g.prev_p[(size_t)r0 * d + e] = g.pts[(size_t)r0 * d + e];
  }
  VilArgs a;
  a.d = d;
  a.m = m;
  a.dz = d;
  a.s = g.s;
  a.dk = d;
  a.diag = g.diag;
  a.core = g.pts + (size_t)r0 * d;
  a.w = g.w + r0;
  a.E = E;
  a.theta = g.theta + (size_t)p * g.s * d;
  a.mode = g.mode + (size_t)p * d;
  a.rowc = g.rowc + 3 * (size_t)r0;
  a.counts = nullptr;
  const VilWs W = bc_vil_ws(pm_fit_ws, d);
  VilFit fit;
  if (bc_pm_fit(a, W, &fit)) {                        // (block-uniform)
    if (tid == 0) g.flag[p] = step + 1;
    return;
  }
  bc_vil_draw(a, W);
  for (int j = tid; j < d; j += nt) a.mode[j] = W.mu[j];
  if (tid == 0) {
    g.newton[2 * p] = fit.steps;
    g.newton[2 * p + 1] += fit.steps;
  }
}

// blockIdx.y < tiles: a tile of the gathered rows; beyond: a tile of the problem's points (none left: nothing to do)
__global__ __launch_bounds__(BC_PM_BLOCK) void k_pm_ll(PmRun g) {
  extern __shared__ double pm_tile[];
  const int p = blockIdx.x, y = blockIdx.y;
  if (*(volatile int*)(g.flag + p) != 0) return;
  PmTileArgs a;
  a.d = g.d;
  a.s = g.s;
  a.theta = g.theta + (size_t)p * g.s * g.d;
  const bool gauss = g.kind == BC_PM_GAUSS;      // (grid-uniform)
  a.sa = gauss ? g.sa + (size_t)p * g.s : nullptr;
  a.ra = nullptr;
  a.c0 = g.c0;
  if (y < g.tiles) {
    a.rows = g.sub;
    a.elem = g.sub_elem;
    a.n = g.n_sub;
    a.ra = g.ra_sub;
    if (gauss) bc_pm_gauss_tile(a, y, pm_tile);
    else bc_pm_ll_tile(a, y, pm_tile);
    bc_pm_tile_colsum(a, y, pm_tile, g.part + ((size_t)p * g.tiles + y) * g.s);
    return;
  }
  const long long r0 = g.row_ptr[p];
  const int m = (int)(g.row_ptr[p + 1] - r0), tile = y - g.tiles;
  if (tile * BC_PM_TILE >= m) return;
  a.rows = g.pts + (size_t)r0 * g.d;
  a.elem = 8;
  a.n = m;
  if (gauss) a.ra = g.ra_pts + r0;
  if (gauss) bc_pm_gauss_tile(a, tile, pm_tile);
  else bc_pm_ll_tile(a, tile, pm_tile);
  bc_pm_tile_store(a, tile, pm_tile, g.cv + (size_t)r0 * g.s);
}

__global__ __launch_bounds__(BC_PM_BLOCK) void k_pm_resid(PmRun g, int step) {
  const int p = blockIdx.x;
  if (*(volatile int*)(g.flag + p) != 0) return;
  const long long r0 = g.row_ptr[p];
  PmResidArgs a;
  a.m = (int)(g.row_ptr[p + 1] - r0);
  a.s = g.s;
  a.tiles = g.tiles;
  a.scale = g.scale;
  a.part = g.part + (size_t)p * g.tiles * g.s;
  a.cv = g.cv + (size_t)r0 * g.s;
  a.w = g.w + r0;
  a.target = g.target + (size_t)p * g.s;
  a.resid = g.resid + (size_t)p * g.s;
  a.gw = g.gw + r0;
  if (bc_pm_resid(a) && threadIdx.x == 0) g.flag[p] = step + 1;
}

__global__ __launch_bounds__(256) void k_pm_pgrad(PmRun g) {
  extern __shared__ double pm_pg_ws[];
  const long long row = blockIdx.x;
  const int p = g.prob_of_row[row];
  if (*(volatile int*)(g.flag + p) != 0) return;
  const long long r0 = g.row_ptr[p];
  PsviArgs a;
  a.kind = g.pg_kind;
  a.m = (int)(g.row_ptr[p + 1] - r0);
  a.s = g.s;
  a.d = g.d;
  a.dz = g.d;
  a.dk = g.d;
  a.pts = g.pts + (size_t)r0 * g.d;
  a.w = g.w + r0;
  a.theta = g.theta + (size_t)p * g.s * g.d;
  a.siginv = g.siginv;      // (null but for the Gaussian kind)
  a.resid = g.resid + (size_t)p * g.s;
  a.sigsq = 1.;
  a.out = g.gp + (size_t)r0 * g.d;
  bc_psvi_point_grad(a, (int)(row - r0), pm_pg_ws);
}

__global__ __launch_bounds__(BC_PM_BLOCK) void k_pm_adam(PmRun g, int step) {
  const int p = blockIdx.x;
  if (*(volatile int*)(g.flag + p) != 0) return;
  const long long r0 = g.row_ptr[p];
  const size_t rd = (size_t)r0 * g.d;
  PmAdamArgs a;
  a.m = (int)(g.row_ptr[p + 1] - r0);
  a.d = g.d;
  a.gw = g.gw + r0;
  a.gp = g.gp + rd;
  a.w = g.w + r0;
  a.pts = g.pts + rd;
  a.m1w = g.m1w + r0;
  a.m1p = g.m1p + rd;
  a.m2w = g.m2w + r0;
  a.m2p = g.m2p + rd;
  a.step = g.steps[(size_t)p * g.itrs + step];
  a.c1 = g.moments[step];
  a.c2 = g.moments[g.itrs + step];
  if (bc_pm_adam(a) && threadIdx.x == 0) g.flag[p] = step + 1;
}

// ------------------------------------------------------------------ host side
struct PmLayout {               // one walk over the slab: the uploaded head, then the device-only state
  size_t pts, w, mode, steps, moments, row_ptr, prob, head;
  size_t m1w, m1p, m2w, m2p, gw, gp, prev_w, prev_p, theta, cv, part, target, resid, rowc, newton, flag, total;
  size_t raw, sa, ra_sub, ra_pts;      // Gaussian kind: behind everything else (the logistic layout is a prefix of it)
};

static PmLayout pm_layout(size_t R, size_t P, size_t d, size_t s, size_t tiles, size_t itrs, int kind = BC_PM_LOGISTIC, size_t n_sub = 0) {
  bc_slab sl;
  PmLayout l;
  l.pts = sl.take(R * d);
  l.w = sl.take(R);
  l.mode = sl.take(P * d);
  l.steps = sl.take(P * itrs);
  l.moments = sl.take(2 * itrs);
  l.row_ptr = sl.take(P + 1);            // (int64)
  l.prob = sl.take((R + 1) / 2);         // (ints)
  l.head = sl.total;
  l.m1w = sl.take(R);
  l.m1p = sl.take(R * d);
  l.m2w = sl.take(R);
  l.m2p = sl.take(R * d);
  l.gw = sl.take(R);
  l.gp = sl.take(R * d);
  l.prev_w = sl.take(R);
  l.prev_p = sl.take(R * d);
  l.theta = sl.take(P * s * d);
  l.cv = sl.take(R * s);
  l.part = sl.take(P * tiles * s);
  l.target = sl.take(P * s);
  l.resid = sl.take(P * s);
  l.rowc = sl.take(3 * R);
  l.newton = sl.take(P);                 // (2 P ints)
  l.flag = sl.take((P + 1) / 2);         // (P ints)
  l.raw = sl.take(kind == BC_PM_GAUSS ? P * s * d : 0);
  l.sa = sl.take(kind == BC_PM_GAUSS ? P * s : 0);
  l.ra_sub = sl.take(kind == BC_PM_GAUSS ? n_sub : 0);
  l.ra_pts = sl.take(kind == BC_PM_GAUSS ? R : 0);
  l.total = sl.total;
  return l;
}

static const bc_run_kind PSVI_MANY_RUN = {"bc_psvi_many", "steps"};
struct bc_psvi_many : bc_run {    // (the run in progress: active, chunk_pending, failed, done of total steps, the clock)
  bc_scratch dev;                 // the slab of pm_layout
  bc_pinned pin;                  // the mirror of the uploaded head; later the landing area of _end
  bc_stage stage;                 // a chunk's draws: normals [k][S][D], then indices [k][n_sub]
  bc_scratch sub;                 // the step's gathered rows
  bc_scratch par;                 // Gaussian kind: Sig0inv | b0 | Siginv (constant over the run; not part of the work space)
  bool lds_set = false, laid_out = false;
  const bc_data* data = nullptr;
  PmRun run;
  PmLayout lay;
  size_t R = 0, P = 0;
  int max_m = 0;
  std::vector<int64_t> row_ptr;
  std::vector<int> flag;          // the marks as the last _chunk_end saw them
};

bool bc_psvi_many_active(const bc_ctx* ctx) { return ctx->psvi_many && ctx->psvi_many->active; }

void bc_psvi_many_free(bc_ctx* ctx) {
  bc_psvi_many* v = ctx->psvi_many;
  if (!v) return;
  bc_scratch_free(&v->dev);
  bc_pinned_free(&v->pin);
  bc_stage_free(&v->stage);
  bc_scratch_free(&v->sub);
  bc_scratch_free(&v->par);
  v->clock.free();
  delete v;
  ctx->psvi_many = nullptr;
}

extern "C" int64_t bc_psvi_curve_work_doubles(int64_t total_points, int32_t n_problems, int32_t d, int32_t s, int64_t n_sub,
                                                  int32_t opt_itrs, int sampler_kind) {
  if (sampler_kind != BC_VI_SAMPLER_LOGISTIC && sampler_kind != BC_VI_SAMPLER_GAUSS) return -1;
  if (total_points < 1 || n_problems < 1 || n_problems > BC_PSVI_MANY_MAX_PROBLEMS || d < 1 || d > BC_VI_MAX_DIM || s < 1 ||
      s > BC_PSVI_MANY_MAX_SAMPLES || n_sub < 1 || n_sub > BC_PSVI_MANY_MAX_SUB || opt_itrs < 1 ||
      total_points > (int64_t)n_problems * BC_PSVI_MANY_MAX_POINTS)
    return -1;
  const size_t tiles = ((size_t)n_sub + BC_PM_TILE - 1) / BC_PM_TILE;
  return (int64_t)pm_layout((size_t)total_points, (size_t)n_problems, (size_t)d, (size_t)s, tiles, (size_t)opt_itrs,
                            sampler_kind == BC_VI_SAMPLER_GAUSS ? BC_PM_GAUSS : BC_PM_LOGISTIC, (size_t)n_sub).total;
}

extern "C" int64_t bc_psvi_many_work_doubles(int64_t total_points, int32_t n_problems, int32_t d, int32_t s, int64_t n_sub, int32_t opt_itrs) {
  return bc_psvi_curve_work_doubles(total_points, n_problems, d, s, n_sub, opt_itrs, BC_VI_SAMPLER_LOGISTIC);
}

extern "C" int bc_psvi_many_auto_chunk(int32_t s, int32_t d, int64_t n_sub) {
  return bc_vi_optimize_auto_chunk(s, d, n_sub);      // (the same staged draws per step: normals [S][D] and n_sub row numbers)
}

static int pm_begin(const char* who, bc_ctx* ctx, const bc_data* data, int model, int sampler_kind, int32_t diag, const double* pts,
                    const double* w0, const int64_t* row_ptr, int32_t n_problems, const double* start, int32_t s, int32_t opt_itrs,
                    const double* steps, const double* moments, int64_t n_sub, double sum_scaling, const double* model_params,
                    int32_t n_model_params, const double* sampler_params, int32_t n_sampler_params) {
  if (!ctx || !data || !pts || !w0 || !row_ptr || !steps || !moments)
    BC_REFUSE("%s: bad argument (context, data, pts, w0, row_ptr, steps and moments are required)", who);
  const bool gauss = model == BC_MODEL_GAUSS_LL && sampler_kind == BC_VI_SAMPLER_GAUSS;
  if (!gauss) {
    if (model == BC_MODEL_GAUSS_LL)
      BC_REFUSE("%s: the Gaussian location model (BC_MODEL_GAUSS_LL) goes with the Gaussian posterior sampler (BC_VI_SAMPLER_GAUSS), "
                "got kind %d", who, sampler_kind);
    if (model != BC_MODEL_LOGISTIC_LL)
      BC_REFUSE("%s: only the logistic log-likelihood (BC_MODEL_LOGISTIC_LL) is served, got model %d: the linear-regression and "
                "Gaussian-location kinds take the loop of single builds", who, model);
    if (sampler_kind != BC_VI_SAMPLER_LOGISTIC)
      BC_REFUSE("%s: only the logistic Laplace sampler (BC_VI_SAMPLER_LOGISTIC, Newton search) is served, got kind %d", who, sampler_kind);
    if (diag != 0 && diag != 1) BC_REFUSE("%s: diag must be 0 or 1, got %d", who, diag);
    if (n_model_params != 0 || n_sampler_params != 0)
      BC_REFUSE("%s: the logistic kind takes no model or sampler parameters (start and diag are arguments), got %d and %d", who,
                n_model_params, n_sampler_params);
  } else {
    if (diag != 0) BC_REFUSE("%s: the Gaussian kind draws with the full covariance only: diag must be 0, got %d", who, diag);
    if (start) BC_REFUSE("%s: the Gaussian kind's posterior is a closed form: start must be NULL", who);
    if (!model_params || !sampler_params || n_model_params < 2 || n_sampler_params < 3)
      BC_REFUSE("%s: the Gaussian kind needs model_params {logdetSig, Siginv} and sampler_params mu0 | Sig0inv | Siginv", who);
  }
  if (n_sub == 0) BC_REFUSE("%s: n_sub = 0 (all rows every step) is not served: every problem has its own Theta", who);
  if (s < 1 || s > BC_PSVI_MANY_MAX_SAMPLES) BC_REFUSE("%s: S = %d is outside 1..%d", who, s, BC_PSVI_MANY_MAX_SAMPLES);
  if (n_sub < 1 || n_sub > BC_PSVI_MANY_MAX_SUB) BC_REFUSE("%s: n_sub = %lld is outside 1..%d", who, (long long)n_sub, BC_PSVI_MANY_MAX_SUB);
  if (opt_itrs < 1) BC_REFUSE("%s: opt_itrs must be at least 1, got %d", who, opt_itrs);
  if (n_problems < 1 || n_problems > BC_PSVI_MANY_MAX_PROBLEMS)
    BC_REFUSE("%s: the number of problems %d is outside 1..%d", who, n_problems, BC_PSVI_MANY_MAX_PROBLEMS);
  int64_t max_m = 0;
  int rc = bc_batch_walk(who, row_ptr, n_problems, BC_PSVI_MANY_MAX_POINTS, "points", &max_m);
  if (rc) return rc;
  if (!(sum_scaling - sum_scaling == 0.)) BC_REFUSE("%s: sum_scaling is not finite", who);
  // (what follows reads the data handle; everything above is decided from the arguments alone)
  if (data->ctx != ctx) BC_REFUSE("%s: data belongs to another context", who);
  const int d = data->dz;
  if (d < 1 || d > BC_VI_MAX_DIM) BC_REFUSE("%s: D = %d is outside 1..%d", who, d, BC_VI_MAX_DIM);
  const size_t P = (size_t)n_problems, R = (size_t)row_ptr[P], tiles = ((size_t)n_sub + BC_PM_TILE - 1) / BC_PM_TILE;
  const size_t dd = (size_t)d * d;
  double c_model[8] = {0.};
  if (gauss) {
    if ((size_t)n_model_params != 1 + dd || (size_t)n_sampler_params != (size_t)d + 2 * dd)
      BC_REFUSE("%s: D = %d takes %zu model parameters {logdetSig, Siginv} and %zu sampler parameters mu0 | Sig0inv | Siginv, got %d and %d",
                who, d, 1 + dd, (size_t)d + 2 * dd, n_model_params, n_sampler_params);
    if (memcmp(model_params + 1, sampler_params + d + dd, dd * sizeof(double)) != 0)
      BC_REFUSE("%s: the sampler's Siginv is not the model's (the doubles must be the same): the draw's Theta' and the tile's "
                "row terms take one matrix", who);
    const double* unused = nullptr;
    if (bc_proj_model_constants(model, model_params, n_model_params, d, c_model, &unused) != BC_OK)
      BC_REFUSE("%s: bad model parameters", who);
  }
  const PmLayout l = pm_layout(R, P, (size_t)d, (size_t)s, tiles, (size_t)opt_itrs, gauss ? BC_PM_GAUSS : BC_PM_LOGISTIC, (size_t)n_sub);
  if (l.total > (size_t)BC_PSVI_MANY_MAX_WORK_DOUBLES)
    BC_REFUSE("%s: the run needs %zu doubles of device work space, at most %lld are served (fewer or smaller problems per run)", who,
              l.total, (long long)BC_PSVI_MANY_MAX_WORK_DOUBLES);
  const size_t lds_fit = (size_t)(gauss ? BC_VIS_WS_DOUBLES(d) : BC_VIL_WS_DOUBLES(d)) * sizeof(double);
  if (lds_fit > (size_t)ctx->max_lds) BC_REFUSE("%s: D = %d needs %zu bytes of LDS, the device offers %d", who, d, lds_fit, ctx->max_lds);
  rc = bc_ctx_refuse_busy(ctx, who, BC_HOLD_ALL, BC_HOLD_PSVI_MANY);
  if (rc) return rc;
  // ---- nothing has been enqueued, allocated or written up to here
  bc_psvi_many* v = ctx->psvi_many;
  if (!v) v = ctx->psvi_many = new bc_psvi_many();
  BC_HIP(hipSetDevice(ctx->device));
  if (!v->lds_set) {
    BC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_pm_fit), hipFuncAttributeMaxDynamicSharedMemorySize, ctx->max_lds));
    BC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_pm_post), hipFuncAttributeMaxDynamicSharedMemorySize, ctx->max_lds));
    v->lds_set = true;
  }
  rc = v->clock.create();
  if (rc) return rc;
  v->laid_out = false;      // (the slab may move below)
  rc = bc_scratch_grow(ctx, &v->dev, l.total);
  const size_t down = bc_even(R) + bc_even(R * d) + P * d;      // what _end brings down: w | pts | modes
  const size_t n_par = gauss ? bc_even(2 * dd + (size_t)d) : 0, up = l.head + n_par;      // (the parameters ride behind the head's mirror)
  if (!rc) rc = bc_pinned_grow(ctx, &v->pin, up > down ? up : down);
  if (!rc && gauss) rc = bc_scratch_grow(ctx, &v->par, n_par);
  if (!rc) rc = bc_scratch_grow(ctx, &v->sub, ((size_t)n_sub * d * data->elem + 7) / 8);
  if (rc) return rc;
  BC_HIP(hipStreamSynchronize(ctx->stream));      // nothing enqueued earlier still reads the slab or the pinned area
  double* h = v->pin.p;
  double* dev = v->dev.p;
  memset(h, 0, l.head * sizeof(double));
  memcpy(h + l.pts, pts, R * d * sizeof(double));
  memcpy(h + l.w, w0, R * sizeof(double));
  if (start) memcpy(h + l.mode, start, P * d * sizeof(double));
  memcpy(h + l.steps, steps, P * (size_t)opt_itrs * sizeof(double));
  memcpy(h + l.moments, moments, 2 * (size_t)opt_itrs * sizeof(double));
  long long* hptr = reinterpret_cast<long long*>(h + l.row_ptr);
  int* hprob = reinterpret_cast<int*>(h + l.prob);
  for (size_t p = 0; p <= P; ++p) hptr[p] = (long long)row_ptr[p];
  for (size_t p = 0; p < P; ++p)
    for (int64_t r = row_ptr[p]; r < row_ptr[p + 1]; ++r) hprob[r] = (int)p;
  BC_HIP(hipMemcpyAsync(dev, h, l.head * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  BC_HIP(hipMemsetAsync(dev + l.head, 0, (l.total - l.head) * sizeof(double), ctx->stream));
  PmRun& g = v->run;
  g.kind = gauss ? BC_PM_GAUSS : BC_PM_LOGISTIC;
  g.pg_kind = bc_psvi_kind(model);
  // BC_PSVI_POST=chains: the posterior stage's three products by bc_vi_sampler's own chains instead of the matrix cores (the form
  // profiles/psvi_many_gauss_notes.md measures the kept one against; read at every begin)
  const char* post_env = getenv("BC_PSVI_POST");
  g.post_chains = post_env && strcmp(post_env, "chains") == 0 ? 1 : 0;
  g.sig0inv = g.b0 = g.siginv = nullptr;
  g.c0 = c_model[0];
  g.raw = g.sa = g.ra_sub = g.ra_pts = nullptr;
  if (gauss) {
    double* hp = h + l.head;      // Sig0inv | b0 | Siginv
    memcpy(hp, sampler_params + d, dd * sizeof(double));
    bc_vi_prior_rhs(sampler_params + d, sampler_params, d, hp + dd);
    memcpy(hp + dd + d, sampler_params + d + dd, dd * sizeof(double));
    BC_HIP(hipMemcpyAsync(v->par.p, hp, (2 * dd + (size_t)d) * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    g.sig0inv = v->par.p;
    g.b0 = v->par.p + dd;
    g.siginv = v->par.p + dd + d;
    g.raw = dev + l.raw;
    g.sa = dev + l.sa;
    g.ra_sub = dev + l.ra_sub;
    g.ra_pts = dev + l.ra_pts;
  }
  g.row_ptr = reinterpret_cast<const long long*>(dev + l.row_ptr);
  g.prob_of_row = reinterpret_cast<const int*>(dev + l.prob);
  g.flag = reinterpret_cast<int*>(dev + l.flag);
  g.newton = reinterpret_cast<int*>(dev + l.newton);
  g.pts = dev + l.pts;
  g.w = dev + l.w;
  g.m1w = dev + l.m1w;
  g.m1p = dev + l.m1p;
  g.m2w = dev + l.m2w;
  g.m2p = dev + l.m2p;
  g.gw = dev + l.gw;
  g.gp = dev + l.gp;
  g.prev_w = dev + l.prev_w;
  g.prev_p = dev + l.prev_p;
  g.mode = dev + l.mode;
  g.theta = dev + l.theta;
  g.cv = dev + l.cv;
  g.part = dev + l.part;
  g.target = dev + l.target;
  g.resid = dev + l.resid;
  g.rowc = dev + l.rowc;
  g.steps = dev + l.steps;
  g.moments = dev + l.moments;
  g.sub = v->sub.p;
  g.sub_elem = data->elem;
  g.d = d;
  g.s = s;
  g.diag = diag;
  g.n_sub = (int)n_sub;
  g.tiles = (int)tiles;
  g.itrs = opt_itrs;
  g.scale = sum_scaling;
  v->lay = l;
  v->R = R;
  v->P = P;
  v->max_m = (int)max_m;
  v->data = data;
  v->row_ptr.assign(row_ptr, row_ptr + P + 1);
  v->flag.assign(P, 0);
  v->laid_out = true;
  bc_run_opened(v, opt_itrs);
  return BC_OK;
}

extern "C" int bc_psvi_many_begin(bc_ctx* ctx, const bc_data* data, int model, int sampler_kind, int32_t diag, const double* pts,
                                  const double* w0, const int64_t* row_ptr, int32_t n_problems, const double* start, int32_t s,
                                  int32_t opt_itrs, const double* steps, const double* moments, int64_t n_sub, double sum_scaling) {
  if (model == BC_MODEL_GAUSS_LL)      // (this entry has no parameters to give that kind)
    BC_REFUSE("bc_psvi_many_begin: only the logistic log-likelihood (BC_MODEL_LOGISTIC_LL) is served, got model %d: the "
              "Gaussian-location kind takes bc_psvi_curve_begin", model);
  return pm_begin("bc_psvi_many_begin", ctx, data, model, sampler_kind, diag, pts, w0, row_ptr, n_problems, start, s, opt_itrs, steps,
                  moments, n_sub, sum_scaling, nullptr, 0, nullptr, 0);
}

extern "C" int bc_psvi_curve_begin(bc_ctx* ctx, const bc_data* data, int model, int sampler_kind, int32_t diag, const double* pts,
                                       const double* w0, const int64_t* row_ptr, int32_t n_problems, const double* start, int32_t s,
                                       int32_t opt_itrs, const double* steps, const double* moments, int64_t n_sub, double sum_scaling,
                                       const double* model_params, int32_t n_model_params, const double* sampler_params,
                                       int32_t n_sampler_params) {
  return pm_begin("bc_psvi_curve_begin", ctx, data, model, sampler_kind, diag, pts, w0, row_ptr, n_problems, start, s, opt_itrs,
                  steps, moments, n_sub, sum_scaling, model_params, n_model_params, sampler_params, n_sampler_params);
}

extern "C" int bc_psvi_many_chunk_begin(bc_ctx* ctx, const double* normals, const int64_t* sub_idx, int32_t k) {
  bc_psvi_many* v = ctx ? ctx->psvi_many : nullptr;
  int rc = bc_run_admit(v, PSVI_MANY_RUN, normals && sub_idx, k);
  if (rc) return rc;
  const PmRun& g = v->run;
  const size_t n_sub = (size_t)g.n_sub;
  const double* stage_dev = nullptr;
  const long long* didx = nullptr;
  rc = bc_stage_step_chunk(ctx, &v->stage, "bc_psvi_many_chunk_begin", normals, (size_t)k * (size_t)g.s * (size_t)g.d, sub_idx, (size_t)k,
                           n_sub, v->done, v->data->n_rows, &stage_dev, &didx);
  if (rc == BC_INVALID_ARGUMENT) v->failed = true;      // (an index out of range spoils this run: only _end is left)
  if (rc) return rc;
  rc = v->clock.start(ctx->stream);
  if (rc) return rc;
  v->chunk_pending = true;      // from here on something is enqueued: _chunk_end must wait even if a launch below fails
  const unsigned P = (unsigned)v->P;
  const bool gauss = g.kind == BC_PM_GAUSS;
  const size_t lds_fit = (size_t)(gauss ? BC_VIS_WS_DOUBLES(g.d) : BC_VIL_WS_DOUBLES(g.d)) * sizeof(double), lds_tile = BC_PM_TILE_DOUBLES(g.s) * sizeof(double);
  const size_t lds_pg = BC_PSVI_WS_DOUBLES(g.d, g.s) * sizeof(double);
  const unsigned pt_tiles = (unsigned)((v->max_m + BC_PM_TILE - 1) / BC_PM_TILE);
  const unsigned ra_tiles = (unsigned)g.tiles + (unsigned)((v->R + BC_PM_TILE - 1) / BC_PM_TILE);
  const size_t lds_ra = BC_PM_ROWAUX_DOUBLES(g.d) * sizeof(double);
  for (int t = 0; t < k; ++t) {
    const int i = (int)v->done + t;
    rc = bc_take_rows_dev(ctx, v->data, didx + (size_t)t * n_sub, (int64_t)n_sub, v->sub.p);
    if (rc) { v->failed = true; return rc; }
    const double* E = stage_dev + (size_t)t * g.s * g.d;
    if (gauss) {
      hipLaunchKernelGGL(k_pm_rowaux, dim3(ra_tiles), dim3(BC_PM_BLOCK), lds_ra, ctx->stream, g, (int)v->R);
      hipLaunchKernelGGL(k_pm_post, dim3(P), dim3(BC_PM_POST_BLOCK), lds_fit, ctx->stream, g, E, i, t == k - 1 ? 1 : 0);
    } else {
      hipLaunchKernelGGL(k_pm_fit, dim3(P), dim3(BC_VIL_BLOCK), lds_fit, ctx->stream, g, E, i, t == k - 1 ? 1 : 0);
    }
    hipLaunchKernelGGL(k_pm_ll, dim3(P, (unsigned)g.tiles + pt_tiles), dim3(BC_PM_BLOCK), lds_tile, ctx->stream, g);
    hipLaunchKernelGGL(k_pm_resid, dim3(P), dim3(BC_PM_BLOCK), 0, ctx->stream, g, i);
    hipLaunchKernelGGL(k_pm_pgrad, dim3((unsigned)v->R), dim3(256), lds_pg, ctx->stream, g);
    hipLaunchKernelGGL(k_pm_adam, dim3(P), dim3(BC_PM_BLOCK), 0, ctx->stream, g, i);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) { v->failed = true; return bc_hip_fail(le, "the step kernels of bc_psvi_many", __FILE__, __LINE__); }
  }
  rc = v->clock.stop(ctx->stream);
  if (rc) return rc;
  v->done += k;
  return BC_OK;
}

extern "C" int bc_psvi_many_chunk_end(bc_ctx* ctx, int32_t* out_marked) {
  bc_psvi_many* v = ctx ? ctx->psvi_many : nullptr;
  int rc = bc_run_pending(v, "bc_psvi_many_chunk_end");
  if (!rc) rc = bc_run_wait_chunk(ctx, v);
  if (rc) return rc;
  BC_HIP(hipMemcpy(v->flag.data(), v->run.flag, v->P * sizeof(int), hipMemcpyDeviceToHost));
  if (out_marked) {
    int32_t n = 0;
    for (int f : v->flag) n += f != 0;
    *out_marked = n;
  }
  return BC_OK;
}

extern "C" int bc_psvi_many_end(bc_ctx* ctx, double* out_w, double* out_pts, double* out_modes, int32_t* out_status) {
  bc_psvi_many* v = ctx ? ctx->psvi_many : nullptr;
  bool pending = false;
  int rc = bc_run_end(ctx, v, PSVI_MANY_RUN, &pending);
  if (rc) return rc;
  v->data = nullptr;
  if (!out_w && !out_pts && !out_modes && !out_status) return BC_OK;
  if (!out_w || !out_pts || !out_modes || !out_status) BC_REFUSE("bc_psvi_many_end: the four outputs are given together or not at all");
  rc = bc_run_complete(v, PSVI_MANY_RUN, pending, "no results");
  if (rc) return rc;
  const size_t R = v->R, P = v->P, d = (size_t)v->run.d;
  double* down = v->pin.p;      // w | pts | modes, as _begin sized it
  double *dw = down, *dp = down + bc_even(R), *dm = dp + bc_even(R * d);
  BC_HIP(hipMemcpyAsync(dw, v->run.w, R * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  BC_HIP(hipMemcpyAsync(dp, v->run.pts, R * d * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  BC_HIP(hipMemcpyAsync(dm, v->run.mode, P * d * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  BC_HIP(hipStreamSynchronize(ctx->stream));
  return bc_batch_unmarked_runs(v->flag.data(), P, out_status, [&](size_t p, size_t q) {
    const size_t r0 = (size_t)v->row_ptr[p], m = (size_t)v->row_ptr[q] - r0;
    memcpy(out_w + r0, dw + r0, m * sizeof(double));
    memcpy(out_pts + r0 * d, dp + r0 * d, m * d * sizeof(double));
    memcpy(out_modes + p * d, dm + p * d, (q - p) * d * sizeof(double));
    return BC_OK;
  });
}

extern "C" int bc_psvi_many_device_ms(bc_ctx* ctx, double* out_ms) {
  return bc_device_ms("bc_psvi_many_device_ms", ctx, ctx && ctx->psvi_many ? &ctx->psvi_many->clock : nullptr, out_ms);
}

extern "C" int bc_psvi_many_last_step(bc_ctx* ctx, int64_t total_points, int32_t n_problems, int32_t d, int32_t s, double* out_w_before,
                                      double* out_pts_before, double* out_mode, double* out_theta, double* out_target, double* out_resid,
                                      double* out_gw, double* out_gp, double* out_w, double* out_pts, double* out_mom1_w,
                                      double* out_mom1_p, double* out_mom2_w, double* out_mom2_p, int32_t* out_newton, int32_t* out_flag) {
  const char* who = "bc_psvi_many_last_step";
  if (!ctx) BC_REFUSE("%s: bad argument", who);
  bc_psvi_many* v = ctx->psvi_many;
  if (!v || !v->laid_out) BC_REFUSE("%s: no run has been begun on this context", who);
  if (v->chunk_pending) BC_REFUSE("%s: a chunk is pending (call bc_psvi_many_chunk_end first)", who);
  const PmRun& g = v->run;
  if ((size_t)total_points != v->R || (size_t)n_problems != v->P || d != g.d || s != g.s)
    BC_REFUSE("%s: the last run had %zu points in %zu problems, D = %d, S = %d, not %lld in %d, D = %d, S = %d", who, v->R, v->P, g.d, g.s,
              (long long)total_points, n_problems, d, s);
  BC_HIP(hipSetDevice(ctx->device));
  BC_HIP(hipStreamSynchronize(ctx->stream));
  const size_t R = v->R, P = v->P, D = (size_t)d, S = (size_t)s;
  const struct { double* out; const double* src; size_t n; } pieces[] = {
      {out_w_before, g.prev_w, R}, {out_pts_before, g.prev_p, R * D}, {out_mode, g.mode, P * D}, {out_theta, g.kind == BC_PM_GAUSS ? g.raw : g.theta, P * S * D},
      {out_target, g.target, P * S}, {out_resid, g.resid, P * S}, {out_gw, g.gw, R}, {out_gp, g.gp, R * D}, {out_w, g.w, R},
      {out_pts, g.pts, R * D}, {out_mom1_w, g.m1w, R}, {out_mom1_p, g.m1p, R * D}, {out_mom2_w, g.m2w, R}, {out_mom2_p, g.m2p, R * D}};
  for (const auto& pc : pieces)
    if (pc.out) BC_HIP(hipMemcpy(pc.out, pc.src, pc.n * sizeof(double), hipMemcpyDeviceToHost));
  if (out_newton) BC_HIP(hipMemcpy(out_newton, g.newton, 2 * P * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (out_flag) BC_HIP(hipMemcpy(out_flag, g.flag, P * sizeof(int32_t), hipMemcpyDeviceToHost));
  return BC_OK;
}
