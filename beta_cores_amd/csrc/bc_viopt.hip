// The weight optimisation of the greedy variational coresets as runs of steps enqueued on the device
// (include/beta_cores_viopt.h): k_vi_sampler (the posterior draw: bc_vi_sampler_dev.h), k_vi_laplace (the logistic Laplace
// sampler: bc_vi_laplace_dev.h), k_vi_adam (util/opt.py's nn_opt), and the entry points that chain them with one gradient's
// projections and algebra (bc_vi_plan_step, bc_vigrad.hip) and the row gather of bc_take.hip.
//
// Nothing here waits for the device except bc_vi_optimize_chunk_end (once per chunk) and the buffer (re)allocations of a run's
// first chunk.  The weights, both ADAM moments and the abort mark live in device memory for the whole run.
#include "bc_internal.h"
#include "bc_vi_sampler_dev.h"
#include "bc_vi_laplace_dev.h"
#include "bc_slab.h"
#include "../../include/beta_cores_viopt.h"
#include "../../include/beta_cores_vilaplace.h"
#include <cmath>
#include <cstring>
#include <vector>

#define BC_VIS_BLOCK 512

// One block.  `flag` != 0: an earlier step of this run met a bad pivot; this launch (and every one behind it) does nothing.
__global__ __launch_bounds__(BC_VIS_BLOCK) void k_vi_sampler(VisArgs a, int* __restrict__ flag, int step) {
  extern __shared__ double vis_ws[];
  if (*(volatile int*)flag != 0) return;      // (block-uniform)
  if (bc_vi_sampler(a, vis_ws) && threadIdx.x == 0) *flag = step + 1;
}

// The logistic kind's draw in the place of k_vi_sampler: one block, the Newton solve of the <= M weighted coreset rows included.
// The mode it ends at stays in a.mode, the next step's start point.
__global__ __launch_bounds__(BC_VIL_BLOCK) void k_vi_laplace(VilArgs a, int* __restrict__ flag, int step) {
  extern __shared__ double vil_ws[];
  if (*(volatile int*)flag != 0) return;      // (block-uniform)
  if (bc_vi_laplace(a, vil_ws) && threadIdx.x == 0) *flag = step + 1;
}

// step[0][i] = step_sched(i), step[1][i] = 1 - b1^(i+1), step[2][i] = 1 - b2^(i+1).  trace: [itrs][m] or null.
__global__ __launch_bounds__(256) void k_vi_adam(const int* __restrict__ flag, const double* __restrict__ g, double* __restrict__ w,
                                                 double* __restrict__ mom1, double* __restrict__ mom2, int m, const double* __restrict__ step,
                                                 int itrs, int i, double b1, double omb1, double b2, double omb2, double eps,
                                                 double* __restrict__ trace) {
  if (*(volatile const int*)flag != 0) return;
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  double x = w[j], m1 = mom1[j], m2 = mom2[j];
  bc_vi_adam_elem(g[j], &x, &m1, &m2, b1, omb1, b2, omb2, eps, step[i], step[itrs + i], step[2 * itrs + i]);
  w[j] = x;
  mom1[j] = m1;
  mom2[j] = m2;
  if (trace) trace[(size_t)i * m + j] = x;
}

static const bc_run_kind VIOPT_RUN = {"bc_vi_optimize", "steps"};
struct bc_viopt : bc_run {        // (the run in progress: active, chunk_pending, failed, done of total steps, the clock)
  bc_scratch dev;                 // one slab: what _begin uploads, then the run's device-only state
  bc_pinned pin;                  // pinned mirror of the uploaded head; later the landing area of w | trace | flag
  bc_stage stage;                 // a chunk's draws: normals [k][S][D], then indices [k][n_sub] (an index takes one double)
  bc_scratch sub;                 // the step's sub-sample of the data rows (their bytes rounded up to whole doubles)
  bc_vi_plan* plan = nullptr;
  bool lds_set = false;
  bool laid_out = false;          // va / nrsel describe the slab as the last _begin left it (bc_vi_optimize_last_draw)
  int nrsel = 0;                  // rows of the zero-padded Theta block K1 reads
  const bc_data* data = nullptr;
  bc_data core_view, sub_view;
  VisArgs va;
  VilArgs la;                     // (logistic kind; va then only names the Theta block for bc_vi_optimize_last_draw)
  int kind = 0;                   // BC_VI_SAMPLER_* of the run
  int64_t m = 0, n_sub = 0;
  int32_t s = 0;
  int d = 0, dz = 0;
  double scale = 1.;
  double *d_w = nullptr, *d_mom1 = nullptr, *d_mom2 = nullptr, *d_grad = nullptr, *d_resid = nullptr, *d_step = nullptr, *d_trace = nullptr;
  int* d_flag = nullptr;
};

bool bc_viopt_active(const bc_ctx* ctx) { return ctx->viopt && ctx->viopt->active; }

void bc_viopt_free(bc_ctx* ctx) {
  bc_viopt* v = ctx->viopt;
  if (!v) return;
  bc_scratch_free(&v->dev);
  bc_pinned_free(&v->pin);
  bc_stage_free(&v->stage);
  bc_scratch_free(&v->sub);
  v->clock.free();
  bc_vi_plan_destroy(v->plan);
  delete v;
  ctx->viopt = nullptr;
}

extern "C" int bc_vi_optimize_auto_chunk(int32_t s, int32_t d, int64_t n_sub) {
  if (s <= 0 || d <= 0 || n_sub < 0) return 1;
  const double per_step = 8. * ((double)s * (double)d + (double)n_sub);
  const double k = floor((double)BC_VI_STAGE_BYTES / per_step);
  return k < 1. ? 1 : k > 1048576. ? 1048576 : (int)k;
}

extern "C" int bc_vi_optimize_begin(bc_ctx* ctx, const bc_data* data, const double* core_rows, int64_t m, int model, const double* params,
                                    int32_t n_params, int sampler_kind, const double* sampler_params, int32_t s, const double* w0,
                                    int32_t opt_itrs, const double* step, int64_t n_sub, double sum_scaling, int want_trace) {
  if (!ctx || !data || !core_rows || !w0 || !step || !sampler_params || (n_params > 0 && !params) || n_params < 0)
    BC_REFUSE("bc_vi_optimize_begin: bad argument");
  if (data->ctx != ctx) BC_REFUSE("bc_vi_optimize_begin: data belongs to another context");
  if (m <= 0 || opt_itrs <= 0 || n_sub < 0 || s <= 0 || s > 256)
    BC_REFUSE("bc_vi_optimize_begin: needs m > 0 coreset rows, opt_itrs > 0, n_sub >= 0 and 1 <= S <= 256 (m = %lld, opt_itrs = %d, n_sub = %lld, S = %d)",
              (long long)m, opt_itrs, (long long)n_sub, s);
  if (sampler_kind != BC_VI_SAMPLER_LINREG && sampler_kind != BC_VI_SAMPLER_GAUSS && sampler_kind != BC_VI_SAMPLER_LOGISTIC)
    BC_REFUSE("bc_vi_optimize_begin: unknown sampler kind %d", sampler_kind);
  const bool gauss = sampler_kind == BC_VI_SAMPLER_GAUSS, logistic = sampler_kind == BC_VI_SAMPLER_LOGISTIC;
  const bool model_ok = gauss      ? (model == BC_MODEL_GAUSS_LL || model == BC_MODEL_GAUSS_BETA)
                        : logistic ? (model == BC_MODEL_LOGISTIC_LL || model == BC_MODEL_LOGISTIC_BETA)
                                   : (model == BC_MODEL_LINREG_LL || model == BC_MODEL_LINREG_BETA);
  if (!model_ok) BC_REFUSE("bc_vi_optimize_begin: model %d does not go with sampler kind %d", model, sampler_kind);
  const int dz = data->dz;
  int d = 0, dk = 0, nrsel = 0, ntsel = 0;
  if (bc_vi_plan_layout(model, s, dz, &d, &dk, &nrsel, &ntsel) != BC_OK || d > BC_VI_MAX_DIM)
    BC_REFUSE("bc_vi_optimize_begin: D = %d is outside 1..%d", d, BC_VI_MAX_DIM);
  if ((size_t)m * (size_t)(dz + 1) > 60000)
    BC_REFUSE("bc_vi_optimize_begin: coreset of %lld rows x %d exceeds the staging area", (long long)m, dz);
  if (logistic && !(sampler_params[d] == 0. || sampler_params[d] == 1.))
    BC_REFUSE("bc_vi_optimize_begin: the diag flag of the logistic sampler must be 0.0 or 1.0");
  const size_t lds = (size_t)(logistic ? BC_VIL_WS_DOUBLES(d) : BC_VIS_WS_DOUBLES(d)) * sizeof(double);
  if (lds > (size_t)ctx->max_lds)
    BC_REFUSE("bc_vi_optimize_begin: D = %d needs %zu bytes of LDS, the device offers %d", d, lds, ctx->max_lds);
  int rc = bc_ctx_refuse_busy(ctx, "bc_vi_optimize_begin", BC_HOLD_ALL, BC_HOLD_VIOPT);
  if (rc) return rc;
  bc_viopt* v = ctx->viopt;
  if (!v) v = ctx->viopt = new bc_viopt();
  BC_HIP(hipSetDevice(ctx->device));
  if (!v->lds_set) {
    BC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_vi_sampler), hipFuncAttributeMaxDynamicSharedMemorySize, ctx->max_lds));
    BC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_vi_laplace), hipFuncAttributeMaxDynamicSharedMemorySize, ctx->max_lds));
    v->lds_set = true;
  }
  rc = v->clock.create();
  if (rc) return rc;
  v->laid_out = false;      // (the slab may move below)
  // ---- the slab: [uploaded head] core | w | step | Sig0inv | b0 | Siginv   [device-only] mom1 | mom2 | grad | resid | Theta, saux |
  //      raw | trace | flag
  //      logistic kind: Sig0inv and b0 are the start point [d + 1] (then the run's mode) and nothing; behind the trace: the row
  //      scratch of k_vi_laplace [3 m] | its counts (4 ints), then the flag
  const size_t dd = logistic ? (size_t)d + 1 : (size_t)d * d;
  //      (a piece that the run's kind does not have takes nothing: the piece behind it starts at the same offset)
  const size_t n_trace = want_trace ? (size_t)opt_itrs * m : 0;
  bc_slab sl;
  const size_t o_core = sl.take((size_t)m * dz), o_w = sl.take(m), o_step = sl.take(3 * (size_t)opt_itrs), o_s0 = sl.take(dd);
  const size_t o_b0 = sl.take(logistic ? 0 : d), o_sg = sl.take(gauss ? dd : 0), head = sl.total;
  const size_t o_m1 = sl.take(m), o_m2 = sl.take(m), o_g = sl.take(m), o_r = sl.take(s);
  const size_t o_th = sl.take((size_t)nrsel * dk + nrsel), o_raw = sl.take((size_t)s * d), o_tr = sl.take(n_trace);
  const size_t o_rowc = sl.take(logistic ? BC_VIL_ROW_DOUBLES(m) : 0), o_cnt = sl.take(logistic ? 2 : 0), o_flag = sl.take(2);
  const size_t total = sl.total;
  rc = bc_scratch_grow(ctx, &v->dev, total);
  bc_slab dn;      // what _end brings down: w | trace, and the flag's two doubles
  dn.take(m);
  dn.take(n_trace);
  dn.take(2);
  if (!rc) rc = bc_pinned_grow(ctx, &v->pin, head > dn.total ? head : dn.total);
  if (rc) return rc;
  BC_HIP(hipStreamSynchronize(ctx->stream));      // nothing enqueued earlier still reads the slab or the pinned area
  double* h = v->pin.p;
  double* dev = v->dev.p;
  memset(h, 0, head * sizeof(double));
  memcpy(h + o_core, core_rows, (size_t)m * dz * sizeof(double));
  memcpy(h + o_w, w0, (size_t)m * sizeof(double));
  memcpy(h + o_step, step, 3 * (size_t)opt_itrs * sizeof(double));
  double sigsq = 1.;
  if (logistic) {
    memcpy(h + o_s0, sampler_params, (size_t)d * sizeof(double));      // the start point; [d] (the last decrement) starts at 0
  } else {
    const double* th0 = sampler_params;
    const double* sig0inv = sampler_params + d;
    memcpy(h + o_s0, sig0inv, dd * sizeof(double));
    bc_vi_prior_rhs(sig0inv, th0, d, h + o_b0);
    if (gauss) memcpy(h + o_sg, sampler_params + d + dd, dd * sizeof(double));
    else sigsq = sampler_params[d + dd];
  }
  BC_HIP(hipMemcpyAsync(dev, h, head * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  BC_HIP(hipMemsetAsync(dev + head, 0, (total - head) * sizeof(double), ctx->stream));
  bc_vi_plan_destroy(v->plan);
  v->plan = nullptr;
  rc = bc_vi_plan_create(ctx, model, params, n_params, dz, s, dev + o_th, gauss ? dev + o_sg : nullptr, &v->plan);
  if (rc) return rc;
  rc = bc_scratch_grow(ctx, &v->sub, ((size_t)n_sub * dz * data->elem + 7) / 8);
  if (rc) return rc;
  v->data = data;
  v->core_view = bc_data();
  v->core_view.ctx = ctx;
  v->core_view.n_rows = m;
  v->core_view.dz = dz;
  v->core_view.z = dev + o_core;
  v->core_view.owned = false;
  v->sub_view = bc_data();
  v->sub_view.ctx = ctx;
  v->sub_view.n_rows = n_sub;
  v->sub_view.dz = dz;
  v->sub_view.z = v->sub.p;
  v->sub_view.owned = false;
  v->sub_view.elem = data->elem;
  VisArgs& a = v->va;
  a.kind = gauss ? BC_VIS_GAUSS : BC_VIS_LINREG;
  a.d = d;
  a.m = (int)m;
  a.dz = dz;
  a.s = s;
  a.dk = dk;
  a.core = dev + o_core;
  a.w = dev + o_w;
  a.sig0inv = dev + o_s0;
  a.b0 = dev + o_b0;
  a.siginv = gauss ? dev + o_sg : nullptr;
  a.sigsq = sigsq;
  a.E = nullptr;
  a.theta = dev + o_th;
  a.saux = dev + o_th + (size_t)nrsel * dk;
  a.raw = dev + o_raw;
  VilArgs& l = v->la;
  l.d = d;
  l.m = (int)m;
  l.dz = dz;
  l.s = s;
  l.dk = dk;
  l.diag = logistic && sampler_params[d] != 0.;
  l.core = a.core;
  l.w = a.w;
  l.E = nullptr;
  l.theta = a.theta;
  l.mode = dev + o_s0;
  l.rowc = dev + o_rowc;
  l.counts = reinterpret_cast<int*>(dev + o_cnt);
  v->kind = sampler_kind;
  v->m = m;
  v->n_sub = n_sub;
  v->s = s;
  v->d = d;
  v->dz = dz;
  v->nrsel = nrsel;
  v->laid_out = true;
  v->scale = sum_scaling;
  v->d_w = dev + o_w;
  v->d_step = dev + o_step;
  v->d_mom1 = dev + o_m1;
  v->d_mom2 = dev + o_m2;
  v->d_grad = dev + o_g;
  v->d_resid = dev + o_r;
  v->d_trace = want_trace ? dev + o_tr : nullptr;
  v->d_flag = reinterpret_cast<int*>(dev + o_flag);
  bc_run_opened(v, opt_itrs);
  return BC_OK;
}

extern "C" int bc_vi_optimize_chunk_begin(bc_ctx* ctx, const double* normals, const int64_t* sub_idx, int32_t k) {
  bc_viopt* v = ctx ? ctx->viopt : nullptr;
  int rc = bc_run_admit(v, VIOPT_RUN, normals != nullptr, k);
  if (rc) return rc;
  const int64_t n_sub = v->n_sub;
  if ((n_sub > 0) != (sub_idx != nullptr)) BC_REFUSE("bc_vi_optimize_chunk_begin: sub_idx must be given exactly when n_sub > 0");
  const double* stage_dev = nullptr;
  const long long* didx = nullptr;
  // (nothing of this chunk is enqueued by a refusal; an index out of range does not fail the run: the next chunk may be given)
  rc = bc_stage_step_chunk(ctx, &v->stage, "bc_vi_optimize_chunk_begin", normals, (size_t)k * (size_t)v->s * (size_t)v->d, sub_idx, (size_t)k,
                           (size_t)n_sub, v->done, v->data->n_rows, &stage_dev, &didx);
  if (rc) return rc;
  rc = v->clock.start(ctx->stream);
  if (rc) return rc;
  v->chunk_pending = true;      // from here on something is enqueued: _chunk_end must wait even if a launch below fails
  const double b1 = 0.9, b2 = 0.999, eps = 1e-8;
  const bool logistic = v->kind == BC_VI_SAMPLER_LOGISTIC;
  const size_t lds = (size_t)(logistic ? BC_VIL_WS_DOUBLES(v->d) : BC_VIS_WS_DOUBLES(v->d)) * sizeof(double);
  const int m = (int)v->m;
  for (int t = 0; t < k; ++t) {
    const int i = (int)v->done + t;
    if (logistic) {
      VilArgs a = v->la;
      a.E = stage_dev + (size_t)t * v->s * v->d;
      hipLaunchKernelGGL(k_vi_laplace, dim3(1), dim3(BC_VIL_BLOCK), lds, ctx->stream, a, v->d_flag, i);
    } else {
      VisArgs a = v->va;
      a.E = stage_dev + (size_t)t * v->s * v->d;
      hipLaunchKernelGGL(k_vi_sampler, dim3(1), dim3(BC_VIS_BLOCK), lds, ctx->stream, a, v->d_flag, i);
    }
    BC_HIP(hipGetLastError());
    const bc_data* rows = v->data;
    if (n_sub > 0) {
      rc = bc_take_rows_dev(ctx, v->data, didx + (size_t)t * n_sub, n_sub, v->sub.p);
      if (rc) return rc;
      rows = &v->sub_view;
    }
    rc = bc_vi_plan_step(ctx, v->plan, &v->core_view, rows, v->d_w, v->scale, v->d_resid, v->d_grad);
    if (rc) return rc;
    hipLaunchKernelGGL(k_vi_adam, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, ctx->stream, v->d_flag, v->d_grad, v->d_w, v->d_mom1,
                       v->d_mom2, m, v->d_step, (int)v->total, i, b1, 1. - b1, b2, 1. - b2, eps, v->d_trace);
    BC_HIP(hipGetLastError());
  }
  rc = v->clock.stop(ctx->stream);
  if (rc) return rc;
  v->done += k;
  return BC_OK;
}

extern "C" int bc_vi_optimize_chunk_end(bc_ctx* ctx) {
  bc_viopt* v = ctx ? ctx->viopt : nullptr;
  int rc = bc_run_pending(v, "bc_vi_optimize_chunk_end");
  if (rc) return rc;
  BC_HIP(hipSetDevice(ctx->device));
  int* hflag = reinterpret_cast<int*>(v->pin.p + v->pin.cap - 2);
  BC_HIP(hipMemcpyAsync(hflag, v->d_flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));      // (rides in front of the wait)
  rc = bc_run_wait_chunk(ctx, v);
  if (rc) return rc;
  if (*hflag != 0) {
    v->failed = true;
    if (v->kind == BC_VI_SAMPLER_LOGISTIC)
      bc_set_error("bc_vi_optimize: step %d: the Laplace fit of the weighted coreset met a weight, a value of the log-joint, a gradient "
                   "or a pivot of the Hessian's Cholesky factorisation that is not finite (a pivot must also be positive)", *hflag - 1);
    else
      bc_set_error("bc_vi_optimize: step %d: the posterior precision matrix of the weighted coreset is not positive definite "
                   "(a pivot of its Cholesky factorisation is not finite and positive)", *hflag - 1);
    return BC_NUMERICAL_PRECISION;
  }
  return BC_OK;
}

extern "C" int bc_vi_optimize_end(bc_ctx* ctx, double* out_w, double* out_trace) {
  bc_viopt* v = ctx ? ctx->viopt : nullptr;
  bool pending = false;
  int rc = bc_run_end(ctx, v, VIOPT_RUN, &pending);
  if (rc) return rc;
  v->data = nullptr;
  if (!out_w) return BC_OK;
  rc = bc_run_complete(v, VIOPT_RUN, pending, "no weights");
  if (rc) return rc;
  if (out_trace && !v->d_trace) BC_REFUSE("bc_vi_optimize_end: the run was begun without a trace");
  const size_t m = (size_t)v->m;
  double* down = v->pin.p;      // w | trace, as _begin sized it
  BC_HIP(hipMemcpyAsync(down, v->d_w, m * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (out_trace) BC_HIP(hipMemcpyAsync(down + bc_even(m), v->d_trace, (size_t)v->total * m * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  BC_HIP(hipStreamSynchronize(ctx->stream));
  memcpy(out_w, down, m * sizeof(double));
  if (out_trace) memcpy(out_trace, down + bc_even(m), (size_t)v->total * m * sizeof(double));
  return BC_OK;
}

extern "C" int bc_vi_optimize_last_draw(bc_ctx* ctx, int32_t s, int32_t d, double* out_theta, double* out_saux, double* out_raw,
                                        double* out_pad_max) {
  if (!ctx || !out_theta || !out_pad_max) BC_REFUSE("bc_vi_optimize_last_draw: bad argument");
  bc_viopt* v = ctx->viopt;
  if (!v || !v->laid_out) BC_REFUSE("bc_vi_optimize_last_draw: no run has been begun on this context");
  if (v->chunk_pending) BC_REFUSE("bc_vi_optimize_last_draw: a chunk is pending (call bc_vi_optimize_chunk_end first)");
  if (s != v->s || d != v->d)
    BC_REFUSE("bc_vi_optimize_last_draw: the last run had S = %d, D = %d, not S = %d, D = %d", v->s, v->d, s, d);
  BC_HIP(hipSetDevice(ctx->device));
  const size_t dk = (size_t)v->va.dk, nr = (size_t)v->nrsel, n_th = nr * dk + nr, n_raw = (size_t)s * d;
  std::vector<double> h(n_th + n_raw);      // Theta [nrsel][dk] | saux [nrsel] (contiguous in the slab), then raw [s][d]
  BC_HIP(hipStreamSynchronize(ctx->stream));
  BC_HIP(hipMemcpy(h.data(), v->va.theta, n_th * sizeof(double), hipMemcpyDeviceToHost));
  BC_HIP(hipMemcpy(h.data() + n_th, v->va.raw, n_raw * sizeof(double), hipMemcpyDeviceToHost));
  double pad = 0.;
  bool pad_nan = false;
  for (size_t q = 0; q < nr; ++q) {
    for (size_t c = 0; c < dk; ++c) {
      const double x = h[q * dk + c];
      if (q < (size_t)s && c < (size_t)d) { out_theta[q * d + c] = x; continue; }
      if (x != x) pad_nan = true;
      else if (fabs(x) > pad) pad = fabs(x);
    }
    const double x = h[nr * dk + q];
    if (q < (size_t)s) { if (out_saux) out_saux[q] = x; continue; }
    if (x != x) pad_nan = true;
    else if (fabs(x) > pad) pad = fabs(x);
  }
  if (out_raw) memcpy(out_raw, h.data() + n_th, n_raw * sizeof(double));
  *out_pad_max = pad_nan ? NAN : pad;
  return BC_OK;
}

extern "C" int bc_vi_laplace_last_mode(bc_ctx* ctx, int32_t d, double* out_mu, int32_t* out_counts) {
  if (!ctx || !out_mu || !out_counts) BC_REFUSE("bc_vi_laplace_last_mode: bad argument");
  bc_viopt* v = ctx->viopt;
  if (!v || !v->laid_out) BC_REFUSE("bc_vi_laplace_last_mode: no run has been begun on this context");
  if (v->chunk_pending) BC_REFUSE("bc_vi_laplace_last_mode: a chunk is pending (call the run's chunk_end first)");
  if (v->kind != BC_VI_SAMPLER_LOGISTIC) BC_REFUSE("bc_vi_laplace_last_mode: the last run had sampler kind %d, not the logistic one", v->kind);
  if (d != v->d) BC_REFUSE("bc_vi_laplace_last_mode: the last run had D = %d, not D = %d", v->d, d);
  BC_HIP(hipSetDevice(ctx->device));
  int cnt[4] = {0, 0, 0, 0};
  BC_HIP(hipStreamSynchronize(ctx->stream));
  BC_HIP(hipMemcpy(out_mu, v->la.mode, (size_t)d * sizeof(double), hipMemcpyDeviceToHost));
  BC_HIP(hipMemcpy(cnt, v->la.counts, sizeof(cnt), hipMemcpyDeviceToHost));
  out_counts[0] = cnt[0];
  out_counts[1] = cnt[1];
  out_counts[2] = cnt[2];
  return BC_OK;
}

extern "C" int bc_vi_optimize_device_ms(bc_ctx* ctx, double* out_ms) {
  return bc_device_ms("bc_vi_optimize_device_ms", ctx, ctx && ctx->viopt ? &ctx->viopt->clock : nullptr, out_ms);
}

extern "C" int bc_vi_optimize(bc_ctx* ctx, const bc_data* data, const double* core_rows, int64_t m, int model, const double* params,
                              int32_t n_params, int sampler_kind, const double* sampler_params, int32_t s, const double* w0,
                              int32_t opt_itrs, const double* step, const double* normals, const int64_t* sub_idx, int64_t n_sub,
                              double sum_scaling, int32_t chunk_steps, double* out_w, double* out_trace) {
  if (!out_w || !normals || chunk_steps < 0) BC_REFUSE("bc_vi_optimize: bad argument");
  if (!ctx || !data || n_sub < 0 || (n_sub > 0) != (sub_idx != nullptr)) BC_REFUSE("bc_vi_optimize: bad argument");
  // every index is checked before anything is enqueued (the chunks check theirs again, which costs nothing next to a step)
  for (size_t j = 0; j < (size_t)(opt_itrs > 0 ? opt_itrs : 0) * (size_t)n_sub; ++j)
    if (sub_idx[j] < 0 || sub_idx[j] >= data->n_rows)
      BC_REFUSE("bc_vi_optimize: index %lld (step %lld, position %lld) out of range [0,%lld)", (long long)sub_idx[j],
                (long long)(j / (size_t)n_sub), (long long)(j % (size_t)n_sub), (long long)data->n_rows);
  int rc = bc_vi_optimize_begin(ctx, data, core_rows, m, model, params, n_params, sampler_kind, sampler_params, s, w0, opt_itrs, step,
                                n_sub, sum_scaling, out_trace != nullptr);
  if (rc) return rc;
  const int d = ctx->viopt->d;
  const int chunk = chunk_steps > 0 ? chunk_steps : bc_vi_optimize_auto_chunk(s, d, n_sub);
  for (int32_t i0 = 0; i0 < opt_itrs && !rc; i0 += chunk) {
    const int32_t k = opt_itrs - i0 < chunk ? opt_itrs - i0 : chunk;
    rc = bc_vi_optimize_chunk_begin(ctx, normals + (size_t)i0 * s * d, sub_idx ? sub_idx + (size_t)i0 * n_sub : nullptr, k);
    if (ctx->viopt->chunk_pending) {
      const int rc2 = bc_vi_optimize_chunk_end(ctx);
      if (!rc) rc = rc2;
    }
  }
  if (rc) return bc_close_failed_run(rc, [&] { return bc_vi_optimize_end(ctx, nullptr, nullptr); });
  return bc_vi_optimize_end(ctx, out_w, out_trace);
}
