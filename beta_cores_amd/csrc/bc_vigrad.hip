// ---------------------------------------------------------------------------------------------
// Store-free projection and the fused gradient of the greedy-VI weight optimisation.
//
// bcores.py:141-146 / sparsevi.py:129-134: every one of the opt_itrs ADAM steps of every build step evaluates
//     vecs = project_f(data, beta) ; resid = sum_scaling * vecs.sum(axis=0) - w.dot(corevecs) ; grad = -corevecs.dot(resid) / S
// i.e. of the N x S projection only its S column sums are used.  The materialising path writes 8*N*S bytes to read S
// numbers back; here K1 keeps its per-tile column partials and stores nothing else (k_project<..., STORE = false>).
//
// This file: the M x S algebra kernels, the three kinds of gradient (bc_vi_gradient, bc_vi_beta_gradient, bc_psvi_gradient) with
// what they keep on a context between calls (struct bc_vigrad), and bc_viopt.hip's way into the same projections.  The
// projection itself -- plans, launches, the K1 instantiations -- is bc_project.hip, reached through bc_project_plan.h.
#include "bc_project_plan.h"
#include "../../include/beta_cores_betagrad.h"
#include "../../include/beta_cores_psvi.h"
#include <cstdio>
#include <cstring>
#include <string>

// what the gradient keeps on a context between calls (ctx->vigrad, created on first use)
struct bc_vigrad {
  bc_phi* core_phi = nullptr;    // bc_vi_gradient: the projection of the <= M coreset rows
  bc_phi* core_gphi = nullptr;   // bc_vi_beta_gradient: their beta-gradient's projection
  bc_scratch buf;                // bc_vi_gradient: grad | resid
  hipEvent_t ev[BC_VI_PHASES + 1] = {};
  double phase_ms[BC_VI_PHASES] = {};
  int64_t calls_timed = 0;
  int64_t pending_m = 0;         // bc_vi_gradient_begin enqueued a gradient of this many rows (bc_vi_gradient_end fetches it)
  int32_t pending_s = 0;
  bool pending_timed = false;
  int pending_kind = 0;          // BC_VI_KIND_*: what the pending gradient left in `pinned`
  int32_t pending_dz = 0;        // (BC_VI_KIND_PSVI: the width of the rows of grad_p)
  double* pinned = nullptr;      // pinned landing area of the pending gradient
  hipStream_t side = nullptr;    // bc_vi_gradient: the coreset rows' K1 runs here, beside the data rows' launch on ctx->stream
  hipEvent_t ev_staged = nullptr, ev_core = nullptr;
};

static bc_vigrad* vigrad_of(bc_ctx* ctx) {
  if (!ctx->vigrad) ctx->vigrad = new bc_vigrad();
  return ctx->vigrad;
}

bool bc_vigrad_pending(const bc_ctx* ctx, int* kind) {
  if (!ctx->vigrad || ctx->vigrad->pending_m <= 0) return false;
  if (kind) *kind = ctx->vigrad->pending_kind;
  return true;
}

// The side stream is joined FIRST: a coreset rows' launch on it reads the two Phis freed here (and the context's proj_theta and
// proj_rowaux, which is why bc_ctx_destroy calls this before it frees those).
void bc_vigrad_free(bc_ctx* ctx) {
  bc_vigrad* g = ctx->vigrad;
  if (!g) return;
  if (g->side) { (void)hipStreamSynchronize(g->side); (void)hipStreamDestroy(g->side); }
  for (auto& ev : g->ev)
    if (ev) (void)hipEventDestroy(ev);
  if (g->core_phi) bc_phi_destroy(g->core_phi);
  if (g->core_gphi) bc_phi_destroy(g->core_gphi);
  bc_scratch_free(&g->buf);
  if (g->pinned) (void)hipHostFree(g->pinned);
  if (g->ev_staged) (void)hipEventDestroy(g->ev_staged);
  if (g->ev_core) (void)hipEventDestroy(g->ev_core);
  delete g;
  ctx->vigrad = nullptr;
}

const char* bc_vi_kind_name(int kind) {
  return kind == BC_VI_KIND_BETA ? "bc_vi_beta_gradient" : kind == BC_VI_KIND_PSVI ? "bc_psvi_gradient" : "bc_vi_gradient";
}

// resid[k] = scale * colsum[k] - sum_i w[i] * C[i, k]   (bcores.py:145: sum_scaling*vecs.sum(axis=0) - w.dot(corevecs))
// grad[i]  = -(sum_k C[i, k] * resid[k]) / S            (bcores.py:146: -corevecs.dot(resid)/corevecs.shape[1])
// C = the projected coreset rows in the tiled layout (row i, sample k at bc_tile_off(i, k, S)): neighbouring threads
// read neighbouring rows, so both passes are coalesced.  One block; m is the coreset size (tens to a few thousand).
__global__ __launch_bounds__(256) void k_vi_gradient(const double* __restrict__ colsum, const double* __restrict__ core,
                                                    const double* __restrict__ w, int m, int s, double scale,
                                                    double* __restrict__ resid_out, double* __restrict__ grad_out) {
  extern __shared__ double rs[];      // [s]
  for (int k = threadIdx.x; k < s; k += blockDim.x) {
    double acc = 0.;
    int i = 0;
    for (; i + 8 <= m; i += 8) {           // same fma chain, eight loads in flight (one block, pure latency)
      double c[8], ww[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) { c[u] = core[bc_tile_off(i + u, k, s)]; ww[u] = w[i + u]; }
#pragma unroll
      for (int u = 0; u < 8; ++u) acc = fma(ww[u], c[u], acc);
    }
    for (; i < m; ++i) acc = fma(w[i], core[bc_tile_off(i, k, s)], acc);
    const double r = scale * colsum[k] - acc;
    rs[k] = r;
    resid_out[k] = r;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < m; i += blockDim.x) {
    double acc = 0.;
    int k = 0;
    for (; k + 8 <= s; k += 8) {
      double c[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) c[u] = core[bc_tile_off(i, k + u, s)];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc = fma(c[u], rs[k + u], acc);
    }
    for (; k < s; ++k) acc = fma(core[bc_tile_off(i, k, s)], rs[k], acc);
    grad_out[i] = -acc / (double)s;
  }
}

// learn_beta (bcores.py:134-137): beta_dots[i] = sum_k G[i, k] * resid[k] for G = the projected beta-gradient of the coreset
// rows (tiled like C above) and the residual k_vi_gradient has just written.  A kernel of its own behind k_vi_gradient, so that
// the latter -- and with it the bits of grad and resid -- is the same code with and without the beta part.
__global__ __launch_bounds__(256) void k_vi_beta_dots(const double* __restrict__ bgrad, const double* __restrict__ resid, int m, int s,
                                                     double* __restrict__ dots_out) {
  extern __shared__ double rs[];      // [s]
  for (int k = threadIdx.x; k < s; k += blockDim.x) rs[k] = resid[k];
  __syncthreads();
  for (int i = threadIdx.x; i < m; i += blockDim.x) {
    double acc = 0.;
    int k = 0;
    for (; k + 8 <= s; k += 8) {
      double c[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) c[u] = bgrad[bc_tile_off(i, k + u, s)];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc = fma(c[u], rs[k + u], acc);
    }
    for (; k < s; ++k) acc = fma(bgrad[bc_tile_off(i, k, s)], rs[k], acc);
    dots_out[i] = acc;
  }
}

extern "C" int bc_model_beta_grad(int beta_model) {
  switch (beta_model) {
    case BC_MODEL_LINREG_BETA: return BC_MODEL_LINREG_BETA_GRAD;
    case BC_MODEL_LOGISTIC_BETA: return BC_MODEL_LOGISTIC_BETA_GRAD;
    case BC_MODEL_GAUSS_BETA: return BC_MODEL_GAUSS_BETA_GRAD;
    default: return -1;
  }
}

// the Phi of the <= M coreset rows the gradient keeps in the context (*slot: core_phi, or core_gphi for the beta-gradient)
static int core_phi_for(bc_ctx* ctx, bc_phi** slot, int64_t m, int32_t s, bc_phi** out) {
  bc_phi* cphi = *slot;
  if (cphi && (cphi->s != s || bc_phi_set_rows(cphi, m) != 0)) {
    BC_HIP(hipStreamSynchronize(ctx->stream));
    bc_phi_destroy(cphi);
    *slot = cphi = nullptr;
  }
  if (!cphi) {
    int64_t cap = 256;
    while (cap < m) cap *= 2;
    int rc = bc_phi_alloc(ctx, m, s, 0, &cphi, cap);
    if (rc) return rc;
    *slot = cphi;
  }
  cphi->stats_valid = false;
  *out = cphi;
  return BC_OK;
}

// the three kinds of gradient.  BC_VI_KIND_PLAIN: bc_vi_gradient.  BC_VI_KIND_BETA (bc_vi_beta_gradient): the coreset rows are
// projected a second time, with grad_model, and the algebra also leaves beta_dots behind grad and resid.  BC_VI_KIND_PSVI
// (bc_psvi_gradient): k_psvi_point_grad runs behind the algebra and leaves the M x dz point-gradient behind grad and resid.
static int vi_gradient_begin(bc_ctx* ctx, const bc_data* data, const double* core_rows, int64_t m, int model, int grad_model,
                             const double* theta, int32_t s, const double* params, int32_t n_params, const double* w,
                             double sum_scaling, bc_comm* comm, int kind = -1) {
  if (kind < 0) kind = grad_model >= 0 ? BC_VI_KIND_BETA : BC_VI_KIND_PLAIN;
  const bool with_beta = kind == BC_VI_KIND_BETA, psvi = kind == BC_VI_KIND_PSVI;
  int rc = bc_proj_project_check(ctx, data, model, theta, s, params, n_params, bc_vi_kind_name(kind));
  if (rc) return rc;
  if (psvi && bc_psvi_kind(model) < 0) {
    bc_set_error("bc_psvi_gradient: model %d has no x-gradient in the reference", model);
    return BC_INVALID_ARGUMENT;
  }
  if (bc_proj_model_store_only(model)) {
    bc_set_error("bc_vi_gradient: model %d (a beta-gradient) has no store-free form for the data rows", model);
    return BC_INVALID_ARGUMENT;
  }
  const char* who = psvi ? "bc_psvi_gradient" : "bc_vi_gradient";
  if (m <= 0 || !core_rows || !w) { bc_set_error("%s: needs a non-empty coreset (m = %lld)", who, (long long)m); return BC_INVALID_ARGUMENT; }
  if (s > 256) { bc_set_error("%s: at most 256 samples (S = %d)", who, s); return BC_INVALID_ARGUMENT; }
  if (comm && bc_comm_ctx(comm) != ctx) { bc_set_error("bc_vi_gradient: the communicator belongs to another context"); return BC_INVALID_ARGUMENT; }
  const int dz = data->dz;
  if (psvi && dz > bc_psvi_max_dz()) {
    bc_set_error("bc_psvi_gradient: rows of %d doubles do not fit the point-gradient's work space (at most %d)", dz, bc_psvi_max_dz());
    return BC_INVALID_ARGUMENT;
  }
  // grad | resid [| beta_dots] [| grad_p]
  const size_t n_core = (size_t)m * dz, n_down = (with_beta ? 2 : 1) * (size_t)m + (size_t)s + (psvi ? n_core : 0);
  rc = bc_ctx_refuse_busy(ctx, (std::string(who) + "_begin").c_str(), BC_HOLD_GRADIENT | BC_HOLD_HMC | BC_HOLD_HMC_SMALL | BC_HOLD_PSVI_MANY, BC_HOLD_GRADIENT);
  if (rc) return rc;
  if (n_down > ctx->pinned_doubles) {
    bc_set_error("%s: coreset of %lld rows x %d exceeds the staging area", who, (long long)m, dz);
    return BC_INVALID_ARGUMENT;
  }
  BC_HIP(hipSetDevice(ctx->device));
  bc_vigrad* vg = vigrad_of(ctx);
  const bool timed = ctx->timing != 0;
  if (timed)
    for (auto& ev : vg->ev)
      if (!ev) BC_HIP(hipEventCreate(&ev));
  auto mark = [&](int i) -> int {
    if (timed) BC_HIP(hipEventRecord(vg->ev[i], ctx->stream));
    return BC_OK;
  };
  // --- stage Theta, the coreset rows and w: one pinned area, one transfer (plan_stage synchronises with the stream first)
  ProjPlan pl;
  rc = mark(0);
  if (rc) return rc;
  const double* esrc[2] = {core_rows, w};
  const size_t en[2] = {n_core, (size_t)m};
  double* edev[2] = {nullptr, nullptr};
  rc = bc_proj_plan_stage(ctx, model, theta, s, params, n_params, dz, false, &pl, 2, esrc, en, edev);
  if (rc) return rc;
  bc_data core_view;                     // the coreset rows where the transfer put them (borrowed)
  core_view.ctx = ctx;
  core_view.n_rows = m;
  core_view.dz = dz;
  core_view.z = edev[0];
  core_view.owned = false;
  bc_data* cd = &core_view;
  const double* d_w = edev[1];
  rc = bc_scratch_grow(ctx, &vg->buf, n_down);
  if (rc) return rc;
  double* d_grad = vg->buf.p;
  double* d_resid = d_grad + m;
  double* d_bdots = d_resid + s;           // (with_beta)
  double* d_gradp = d_resid + s;           // (psvi) [m][dz]
  // the beta-gradient's plan: the value model's staged Theta, saux and Siginv (nothing is uploaded twice), its own constants
  ProjPlan gpl = pl;
  if (with_beta) {
    const double* unused = nullptr;
    if (bc_proj_model_constants(grad_model, params, n_params, pl.d, gpl.a.c, &unused) != BC_OK) {
      bc_set_error("bc_vi_beta_gradient: model %d expects a different number of parameters than %d (d = %d)", grad_model, n_params, pl.d);
      return BC_INVALID_ARGUMENT;
    }
    gpl.a.model = gpl.model = grad_model;
    gpl.a.ck = gpl.a.cv = nullptr;         // host-evaluated constants belong to the value model
    gpl.a.nck = 0;
  }
  rc = mark(1);
  if (rc) return rc;
  // --- the <= M coreset rows (materialised: the M x S algebra below reads them), then the data rows (store-free)
  bc_phi *cphi = nullptr, *gphi = nullptr;
  rc = core_phi_for(ctx, &vg->core_phi, m, s, &cphi);
  if (!rc && with_beta) rc = core_phi_for(ctx, &vg->core_gphi, m, s, &gphi);
  if (rc) return rc;
  // The coreset rows' launch (one tile or a few: ~20 us of dependent latency, no work to speak of) runs on a side stream
  // BESIDE the data rows' launch instead of in front of it; the algebra kernel waits for both (0.441 -> 0.427 ms per native
  // call at N = 1M, D = 64).  The instrumented pass (timing on) keeps everything on one stream, so that its five phases stay a
  // partition of the call.
  const bool beside = !timed;
  if (beside && !vg->side) {
    BC_HIP(hipStreamCreateWithFlags(&vg->side, hipStreamNonBlocking));
    BC_HIP(hipEventCreateWithFlags(&vg->ev_staged, hipEventDisableTiming));
    BC_HIP(hipEventCreateWithFlags(&vg->ev_core, hipEventDisableTiming));
  }
  {
    bc_proj_scope untimed(ctx, nullptr);      // the coreset rows' launch is not a K1 sample of the kernel timer
    if (beside) {
      BC_HIP(hipEventRecord(vg->ev_staged, ctx->stream));             // Theta, the coreset rows and w have landed
      BC_HIP(hipStreamWaitEvent(vg->side, vg->ev_staged, 0));
      {
        bc_proj_scope on_side(ctx, vg->side);
        rc = bc_proj_plan_launch(ctx, pl, cd, cphi, PROJ_FULL, s, 0, &ctx->proj_rowaux);
        if (!rc && with_beta) rc = bc_proj_plan_launch(ctx, gpl, cd, gphi, PROJ_FULL, s, 0, &ctx->proj_rowaux);      // behind it, same stream
      }
      if (!rc) {
        const hipError_t e = hipEventRecord(vg->ev_core, vg->side);
        if (e != hipSuccess) rc = bc_hip_fail(e, "hipEventRecord(vi_ev_core)", __FILE__, __LINE__);
      }
    } else {
      rc = bc_proj_plan_launch(ctx, pl, cd, cphi, PROJ_FULL, s, 0, &ctx->proj_rowaux);
      if (!rc && with_beta) rc = bc_proj_plan_launch(ctx, gpl, cd, gphi, PROJ_FULL, s, 0, &ctx->proj_rowaux);
    }
  }
  // Everything after the side launch runs inside `rest`: on ANY failure in it the side stream is joined before the error
  // leaves this function -- the next call's plan_stage / bc_scratch_grow synchronise ctx->stream only and would otherwise
  // overwrite proj_theta / free core_phi under a coreset-row kernel that is still reading them.
  auto rest = [&]() -> int {
    int rc = mark(2);
    bc_phi* phi = nullptr;
    if (!rc) rc = bc_proj_colsum_phi_for(ctx, data->n_rows, s, &phi);
    // (x^T Siginv x of the data rows, Gaussian models, goes to a scratch of its own: the coreset rows' is still in use)
    if (!rc) rc = bc_proj_plan_launch(ctx, pl, data, phi, PROJ_COLSUM, s, 0, &ctx->proj_rowaux2);
    if (!rc) rc = mark(3);
    if (!rc) rc = bc_phi_reduce_colsum(phi);
    if (rc) return rc;
    const double* colsum = phi->colsum;
    if (comm) {
      rc = bc_comm_sum_dev(comm, phi->colsum, s, &colsum);
      if (rc) return rc;
    }
    rc = mark(4);
    if (rc) return rc;
    if (beside) BC_HIP(hipStreamWaitEvent(ctx->stream, vg->ev_core, 0));
    hipLaunchKernelGGL(k_vi_gradient, dim3(1), dim3(256), (size_t)s * sizeof(double), ctx->stream, colsum, cphi->tiles, d_w,
                       (int)m, s, sum_scaling, d_resid, d_grad);
    BC_HIP(hipGetLastError());
    if (with_beta) {
      hipLaunchKernelGGL(k_vi_beta_dots, dim3(1), dim3(256), (size_t)s * sizeof(double), ctx->stream, gphi->tiles, d_resid, (int)m, s, d_bdots);
      BC_HIP(hipGetLastError());
    }
    if (psvi) {      // the points, their weights, Theta (Gaussian: Theta') and Siginv are where plan_stage has put them
      rc = bc_psvi_point_grad_launch(ctx, model, edev[0], d_w, m, dz, pl.d, s, pl.a.theta, pl.a.dk, pl.siginv_dev,
                                     model == BC_MODEL_LINREG_LL ? params[0] : 0., d_resid, d_gradp);
      if (rc) return rc;
    }
    // the result lands in a pinned area of its own: whatever the host does between _begin and _end (it may well call into this
    // library, whose other entry points stage through ctx->pinned) cannot overwrite it
    if (!vg->pinned) BC_HIP(hipHostMalloc((void**)&vg->pinned, ctx->pinned_doubles * sizeof(double), hipHostMallocDefault));
    BC_HIP(hipMemcpyAsync(vg->pinned, d_grad, n_down * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    return mark(5);
  };
  if (!rc) rc = rest();
  if (rc) {
    if (beside) (void)hipStreamSynchronize(vg->side);
    return rc;
  }
  vg->pending_m = m;
  vg->pending_s = s;
  vg->pending_timed = timed;
  vg->pending_kind = kind;
  vg->pending_dz = dz;
  return BC_OK;
}

extern "C" int bc_vi_gradient_begin(bc_ctx* ctx, const bc_data* data, const double* core_rows, int64_t m, int model,
                                    const double* theta, int32_t s, const double* params, int32_t n_params, const double* w,
                                    double sum_scaling, bc_comm* comm) {
  return vi_gradient_begin(ctx, data, core_rows, m, model, -1, theta, s, params, n_params, w, sum_scaling, comm);
}

extern "C" int bc_vi_beta_gradient_begin(bc_ctx* ctx, const bc_data* data, const double* core_rows, int64_t m, int beta_model,
                                         const double* theta, int32_t s, const double* params, int32_t n_params, const double* w,
                                         double sum_scaling, bc_comm* comm) {
  const int grad_model = bc_model_beta_grad(beta_model);
  if (grad_model < 0) {
    bc_set_error("bc_vi_beta_gradient: model %d is not a beta-likelihood with a beta-gradient", beta_model);
    return BC_INVALID_ARGUMENT;
  }
  return vi_gradient_begin(ctx, data, core_rows, m, beta_model, grad_model, theta, s, params, n_params, w, sum_scaling, comm);
}

// second half: wait for the enqueued gradient and hand it out (whatever the host did meanwhile -- e.g. drawing the next
// sample matrix's normals -- ran beside the GPU)
// out_extra: beta_dots [m] (BC_VI_KIND_BETA) or grad_p [m][dz] (BC_VI_KIND_PSVI)
static int vi_gradient_end(bc_ctx* ctx, double* out_grad, double* out_extra, double* out_resid, int kind) {
  char who[40];
  snprintf(who, sizeof(who), "%s_end", bc_vi_kind_name(kind));
  if (!ctx || !out_grad || (kind != BC_VI_KIND_PLAIN && !out_extra)) { bc_set_error("%s: bad argument", who); return BC_INVALID_ARGUMENT; }
  bc_vigrad* vg = ctx->vigrad;          // (null: no gradient was ever begun on this context)
  if (!vg || vg->pending_m <= 0) { bc_set_error("%s: no gradient is pending on this context", who); return BC_INVALID_ARGUMENT; }
  if (vg->pending_kind != kind) {       // the pending gradient stays pending
    bc_set_error("%s: the pending gradient was begun by %s_begin", who, bc_vi_kind_name(vg->pending_kind));
    return BC_INVALID_ARGUMENT;
  }
  const int64_t m = vg->pending_m;
  const int32_t s = vg->pending_s;
  const bool timed = vg->pending_timed;
  vg->pending_m = 0;
  BC_HIP(hipSetDevice(ctx->device));
  BC_HIP(hipStreamSynchronize(ctx->stream));
  memcpy(out_grad, vg->pinned, (size_t)m * sizeof(double));
  if (out_resid) memcpy(out_resid, vg->pinned + m, (size_t)s * sizeof(double));
  if (kind == BC_VI_KIND_BETA) memcpy(out_extra, vg->pinned + m + s, (size_t)m * sizeof(double));
  if (kind == BC_VI_KIND_PSVI) memcpy(out_extra, vg->pinned + m + s, (size_t)m * vg->pending_dz * sizeof(double));
  if (timed) {
    for (int i = 0; i < BC_VI_PHASES; ++i) {
      float ms = 0.f;
      BC_HIP(hipEventElapsedTime(&ms, vg->ev[i], vg->ev[i + 1]));
      vg->phase_ms[i] += ms;
    }
    vg->calls_timed++;
  }
  return BC_OK;
}

extern "C" int bc_vi_gradient_end(bc_ctx* ctx, double* out_grad, double* out_resid) {
  return vi_gradient_end(ctx, out_grad, nullptr, out_resid, BC_VI_KIND_PLAIN);
}

extern "C" int bc_vi_beta_gradient_end(bc_ctx* ctx, double* out_grad, double* out_beta_dots, double* out_resid) {
  return vi_gradient_end(ctx, out_grad, out_beta_dots, out_resid, BC_VI_KIND_BETA);
}

// ---- include/beta_cores_psvi.h: BatchPSVICoreset's whole gradient.  The same staging, the same projections and the same
// k_vi_gradient launch as bc_vi_gradient (grad_w and resid carry its bits), k_psvi_point_grad behind it, one download.
extern "C" int bc_psvi_gradient_begin(bc_ctx* ctx, const bc_data* data, const double* points, int64_t m, int model,
                                      const double* theta, int32_t s, const double* params, int32_t n_params, const double* w,
                                      double sum_scaling) {
  return vi_gradient_begin(ctx, data, points, m, model, -1, theta, s, params, n_params, w, sum_scaling, nullptr, BC_VI_KIND_PSVI);
}

extern "C" int bc_psvi_gradient_end(bc_ctx* ctx, double* out_grad_w, double* out_grad_p, double* out_resid) {
  return vi_gradient_end(ctx, out_grad_w, out_grad_p, out_resid, BC_VI_KIND_PSVI);
}

extern "C" int bc_psvi_gradient(bc_ctx* ctx, const bc_data* data, const double* points, int64_t m, int model,
                                const double* theta, int32_t s, const double* params, int32_t n_params, const double* w,
                                double sum_scaling, double* out_grad_w, double* out_grad_p, double* out_resid) {
  if (!out_grad_w || !out_grad_p) { bc_set_error("bc_psvi_gradient: bad argument"); return BC_INVALID_ARGUMENT; }
  int rc = bc_psvi_gradient_begin(ctx, data, points, m, model, theta, s, params, n_params, w, sum_scaling);
  if (rc) return rc;
  return bc_psvi_gradient_end(ctx, out_grad_w, out_grad_p, out_resid);
}

extern "C" int bc_vi_beta_gradient(bc_ctx* ctx, const bc_data* data, const double* core_rows, int64_t m, int beta_model,
                                   const double* theta, int32_t s, const double* params, int32_t n_params, const double* w,
                                   double sum_scaling, bc_comm* comm, double* out_grad, double* out_beta_dots, double* out_resid) {
  if (!out_grad || !out_beta_dots) { bc_set_error("bc_vi_beta_gradient: bad argument"); return BC_INVALID_ARGUMENT; }
  int rc = bc_vi_beta_gradient_begin(ctx, data, core_rows, m, beta_model, theta, s, params, n_params, w, sum_scaling, comm);
  if (rc) return rc;
  return bc_vi_beta_gradient_end(ctx, out_grad, out_beta_dots, out_resid);
}

extern "C" int bc_vi_gradient(bc_ctx* ctx, const bc_data* data, const double* core_rows, int64_t m, int model,
                              const double* theta, int32_t s, const double* params, int32_t n_params, const double* w,
                              double sum_scaling, bc_comm* comm, double* out_grad, double* out_resid) {
  if (!out_grad) { bc_set_error("bc_vi_gradient: bad argument"); return BC_INVALID_ARGUMENT; }
  int rc = bc_vi_gradient_begin(ctx, data, core_rows, m, model, theta, s, params, n_params, w, sum_scaling, comm);
  if (rc) return rc;
  return bc_vi_gradient_end(ctx, out_grad, out_resid);
}

extern "C" int bc_ctx_phase_times(bc_ctx* ctx, double* out_ms, int32_t n, int64_t* calls, int reset) {
  if (!ctx || (n > 0 && !out_ms)) { bc_set_error("bc_ctx_phase_times: bad argument"); return BC_INVALID_ARGUMENT; }
  bc_vigrad* vg = ctx->vigrad;          // (null: no gradient yet, zeros and no calls)
  for (int i = 0; i < n; ++i) out_ms[i] = vg && i < BC_VI_PHASES ? vg->phase_ms[i] : 0.;
  if (calls) *calls = vg ? vg->calls_timed : 0;
  if (reset && vg) {
    for (auto& v : vg->phase_ms) v = 0.;
    vg->calls_timed = 0;
  }
  return BC_OK;
}

// ------------------------------------------------------------------ bc_viopt.hip's way into the projection
// The steps 2 and 4-6 of one gradient (include/beta_cores_viopt.h) for a Theta that is ALREADY on the device -- k_vi_sampler
// has written it there in the zero-padded layout the plan describes -- enqueued on ctx->stream without any host wait.
struct bc_vi_plan {
  ProjPlan pl;
};

int bc_vi_plan_layout(int model, int32_t s, int dz, int* d, int* dk, int* nrsel, int* ntsel) {
  *d = dz - (bc_proj_model_has_y(model) ? 1 : 0);
  if (*d <= 0 || s <= 0 || s > 256) return BC_INVALID_ARGUMENT;
  bc_proj_theta_layout(s, *d, false, ntsel, nrsel, dk);
  return BC_OK;
}

// theta_dev: [nrsel][dk] | saux [nrsel], zero outside the s x d block the sampler writes.  siginv_dev: the Gaussian models' Siginv.
int bc_vi_plan_create(bc_ctx* ctx, int model, const double* params, int32_t n_params, int dz, int32_t s, const double* theta_dev,
                      const double* siginv_dev, bc_vi_plan** out) {
  if (model < 0 || model > BC_MODEL_LOGISTIC_BETA_GRAD || bc_proj_model_store_only(model)) {
    bc_set_error("bc_vi_optimize: model %d has no store-free projection", model);
    return BC_INVALID_ARGUMENT;
  }
  int d, dk, nrsel, ntsel;
  if (bc_vi_plan_layout(model, s, dz, &d, &dk, &nrsel, &ntsel) != BC_OK) { bc_set_error("bc_vi_optimize: bad shape (S = %d, dz = %d)", s, dz); return BC_INVALID_ARGUMENT; }
  bc_vi_plan* p = new bc_vi_plan();
  memset(&p->pl.a, 0, sizeof(p->pl.a));
  const double* siginv = nullptr;
  if (bc_proj_plan_constants(ctx, model, params, n_params, d, &p->pl.a, &siginv) != BC_OK) { delete p; return BC_INVALID_ARGUMENT; }
  if ((siginv != nullptr) != (siginv_dev != nullptr)) { bc_set_error("bc_vi_optimize: internal: Siginv"); delete p; return BC_INVALID_ARGUMENT; }
  bc_proj_plan_bind(&p->pl, model, s, d, dk, ntsel, nrsel, false, theta_dev, siginv_dev);
  *out = p;
  return BC_OK;
}

void bc_vi_plan_destroy(bc_vi_plan* p) { delete p; }

// resid = scale * colsum(K1(rows)) - w . K1(core), grad = -K1(core) . resid / S: everything on ctx->stream, nothing waited for
int bc_vi_plan_step(bc_ctx* ctx, const bc_vi_plan* p, const bc_data* core, const bc_data* rows, const double* w_dev, double scale,
                    double* resid_dev, double* grad_dev) {
  const ProjPlan& pl = p->pl;
  const int32_t s = pl.s;
  bc_phi *cphi = nullptr, *phi = nullptr;
  int rc = core_phi_for(ctx, &vigrad_of(ctx)->core_phi, core->n_rows, s, &cphi);
  if (!rc) rc = bc_proj_colsum_phi_for(ctx, rows->n_rows, s, &phi);
  {
    bc_proj_scope untimed(ctx, nullptr);      // (no K1 samples of the kernel timer from inside the loop)
    if (!rc) rc = bc_proj_plan_launch(ctx, pl, core, cphi, PROJ_FULL, s, 0, &ctx->proj_rowaux);
    if (!rc) rc = bc_proj_plan_launch(ctx, pl, rows, phi, PROJ_COLSUM, s, 0, &ctx->proj_rowaux2);
  }
  if (!rc) rc = bc_phi_reduce_colsum(phi);
  if (rc) return rc;
  hipLaunchKernelGGL(k_vi_gradient, dim3(1), dim3(256), (size_t)s * sizeof(double), ctx->stream, phi->colsum, cphi->tiles, w_dev,
                     (int)core->n_rows, s, scale, resid_dev, grad_dev);
  BC_HIP(hipGetLastError());
  return BC_OK;
}
