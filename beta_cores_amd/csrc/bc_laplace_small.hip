// The Laplace fit of many small logistic posteriors at once (include/beta_cores_laplace_small.h): k_laplace_many, one thread
// block per problem, and its one synchronous entry point.
//
// k_laplace_many.  Block p fills a VilArgs for its own problem -- its rows and weights inside the packed batch, its start, its
// normals, its slices of the outputs, its own 3 n_p doubles of row scratch -- and runs the four stages of bc_vi_laplace_dev.h
// (the device function k_vi_laplace runs for ONE problem inside the weight optimisation loop: damped Newton with H and the
// gradient as one Gram product on v_mfma_f64_16x16x4_f64, a right-looking Cholesky in LDS, C^-1, the draw on the matrix cores).
// Between and behind the stages it stores what that function computes but does not keep: diag H(mu) from the packed triangle
// before it is factorised, f(mu), C and C^-1 as dense lower triangles, the iteration counts.  Grid = P blocks of BC_VIL_BLOCK
// threads, dynamic LDS = BC_VIL_WS_DOUBLES(D) doubles (134 KiB at D = 128: one block per CU; more at small D).  The rows stay in
// device memory and are read through L2, so a problem's row count is not bounded by the LDS.
//
// Blocks never wait for each other: no flags between blocks, no cooperative launch; blocks beyond the resident capacity queue.
// Every loop of the header has a fixed bound and every sum a fixed order, and a block reads nothing but its own problem, so a
// problem's bits do not depend on P, on its place in the batch or on the other problems.  A problem the stages refuse (a weight,
// start, value, decrement or pivot that is not finite; a pivot must also be positive) sets its flag and returns before it has
// stored anything: k_hmc_small's rule.
#include "bc_internal.h"
#include "bc_vi_laplace_dev.h"
#include "bc_slab.h"
#include "bc_batch.h"
#include "../../include/beta_cores_laplace_small.h"
#include <cstring>
#include <vector>

static_assert(BC_LAPLACE_SMALL_MAX_DIM == BC_VIL_MAXD, "include/beta_cores_laplace_small.h states the device function's limit");

struct LmArgs {
  const double* rows;           // packed rows [sum n][d]
  const double* w;              // [sum n]
  const long long* row_ptr;     // [P + 1]
  const double* start;          // [P][d]
  const double* e;              // the normals: [s][d] per problem
  long long e_stride;           // per problem (0: shared)
  double* rowc;                 // [3 sum n]: problem p's BC_VIL_ROW_DOUBLES(n_p) begin at 3 row_ptr[p]
  int* flag;                    // [P]: 1 = the problem was refused (zeroed by the call)
  double* theta;                // out [P][s][d]
  double* mu;                   // out [P][d]
  double* hdiag;                // out [P][d]
  double* value;                // out [P]
  double* chol;                 // out [P][d][d], or null (the diagonal form, or factors not wanted)
  double* inv;                  // out [P][d][d], or null
  int* counts;                  // out [P][3]: Newton steps | halvings of the last line search | halvings of all line searches
  int d, s, diag;
};

__global__ __launch_bounds__(BC_VIL_BLOCK) void k_laplace_many(LmArgs g) {
  extern __shared__ double lm_ws[];
  const int p = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, d = g.d;
  const long long r0 = g.row_ptr[p];
  VilArgs a;
  a.d = d;
  a.m = (int)(g.row_ptr[p + 1] - r0);
  a.dz = d;
  a.s = g.s;
  a.dk = d;
  a.diag = g.diag;
  a.core = g.rows + (size_t)r0 * d;
  a.w = g.w + r0;
  a.E = g.e + (size_t)p * g.e_stride;
  a.theta = g.theta + (size_t)p * g.s * d;
  a.mode = const_cast<double*>(g.start) + (size_t)p * d;      // (the stages only read the start point from it)
  a.rowc = g.rowc + 3 * (size_t)r0;
  a.counts = nullptr;                                          // (written by bc_vi_laplace() only)
  const VilWs W = bc_vil_ws(lm_ws, d);
  VilFit fit;
  int bad = bc_vil_mode(a, W, &fit);
  if (!bad) {
    bc_vil_hessian(a, W);
    // diag H(mu), kept in `stp` (free since the mode search ended) until the problem is known to be good: the factorisation
    // overwrites the triangle.  Element j is written and later read by the same thread.
    for (int j = tid; j < d; j += nt) W.stp[j] = W.A[bc_vil_tri(j, j)];
    BC_VIL_SYNC();
    bad = bc_vil_factor(a, W);
  }
  if (bad) {                                                   // (block-uniform)
    if (tid == 0) g.flag[p] = 1;
    return;
  }
  bc_vil_draw(a, W);
  const size_t od = (size_t)p * d;
  for (int j = tid; j < d; j += nt) {
    g.mu[od + j] = W.mu[j];
    g.hdiag[od + j] = W.stp[j];
  }
  if (g.chol) {
    double* oc = g.chol + od * d;
    double* oi = g.inv + od * d;
    for (int e = tid; e < d * d; e += nt) {
      const int i = e / d, j = e - i * d;
      oc[e] = j <= i ? W.A[bc_vil_tri(i, j)] : 0.;
      oi[e] = j <= i ? W.Li[bc_vil_tri(i, j)] : 0.;
    }
  }
  if (tid == 0) {
    g.value[p] = fit.f;
    g.counts[3 * (size_t)p] = fit.steps;
    g.counts[3 * (size_t)p + 1] = fit.halvings;
    g.counts[3 * (size_t)p + 2] = fit.halvings_all;
  }
}

// ------------------------------------------------------------------ host side
struct bc_lap_small {
  bc_stage in;                    // rows | w | start | normals | row_ptr (int64) | flags (ints, zero): one transfer
  bc_scratch work;                // the row scratch of all problems
  bc_scratch out;                 // theta | mu | hdiag | value | chol | inv | counts (ints)
  bc_scratch score;               // ll [P s] | correct [P s] (ints)
  bc_run_clock clock;
};

void bc_laplace_small_free(bc_ctx* ctx) {
  bc_lap_small* h = ctx->laplace_small;
  if (!h) return;
  bc_stage_free(&h->in);
  bc_scratch_free(&h->work);
  bc_scratch_free(&h->out);
  bc_scratch_free(&h->score);
  h->clock.free();
  delete h;
  ctx->laplace_small = nullptr;
}

extern "C" int bc_laplace_small(bc_ctx* ctx, const double* rows, const double* w, const int64_t* row_ptr, int32_t n_problems, int32_t d,
                                const double* start, int32_t diag, const double* normals, int64_t problem_stride, int32_t s,
                                const bc_data* zt, const bc_data* yt, double* out_mu, double* out_hdiag, double* out_value,
                                int32_t* out_counts, int32_t* out_status, double* out_chol, double* out_inv, double* out_theta,
                                int32_t* out_correct, double* out_ll) {
  const char* who = "bc_laplace_small";
  if (!ctx || !rows || !w || !row_ptr || !out_mu || !out_hdiag || !out_value || !out_counts || !out_status)
    BC_REFUSE("%s: bad argument (context, rows, weights, row_ptr, out_mu, out_hdiag, out_value, out_counts and out_status are required)", who);
  if (n_problems < 1) BC_REFUSE("%s: needs at least one problem, got %d", who, n_problems);
  if (d < 1 || d > BC_LAPLACE_SMALL_MAX_DIM) BC_REFUSE("%s: rows must have 1 .. %d columns, got %d", who, BC_LAPLACE_SMALL_MAX_DIM, d);
  if (s < 0 || s > BC_LAPLACE_SMALL_MAX_DRAWS) BC_REFUSE("%s: 0 .. %d draws per problem are served, got %d", who, BC_LAPLACE_SMALL_MAX_DRAWS, s);
  if (diag != 0 && diag != 1) BC_REFUSE("%s: diag must be 0 or 1, got %d", who, diag);
  if ((normals == nullptr) != (s == 0)) BC_REFUSE("%s: normals are given exactly when s >= 1 (s = %d)", who, s);
  const size_t sd = (size_t)s * d;
  if (problem_stride != 0 && (problem_stride < 0 || (size_t)problem_stride < sd))
    BC_REFUSE("%s: problem_stride must be 0 or at least s D = %zu, got %lld", who, sd, (long long)problem_stride);
  if ((out_chol == nullptr) != (out_inv == nullptr)) BC_REFUSE("%s: out_chol and out_inv are given together or not at all", who);
  if (diag && out_chol) BC_REFUSE("%s: the diagonal form has no factors (out_chol and out_inv must be NULL with diag)", who);
  if ((zt == nullptr) != (yt == nullptr)) BC_REFUSE("%s: the held-out rows and labels are given together or not at all", who);
  if ((out_correct == nullptr) != (out_ll == nullptr) || (out_ll != nullptr) != (zt != nullptr))
    BC_REFUSE("%s: out_correct and out_ll are given exactly when the held-out rows and labels are", who);
  int64_t max_n = 0;
  int rc = bc_batch_walk(who, row_ptr, n_problems, (int64_t)1 << 24, "rows", &max_n);
  if (rc) return rc;
  const size_t P = (size_t)n_problems, n_all = (size_t)row_ptr[P], t = P * (size_t)s;
  if (zt) {
    if (s < 1) BC_REFUSE("%s: scoring needs at least one draw per problem (s = 0)", who);
    rc = bc_score_check(ctx, zt, yt, (int64_t)t, d, who);
    if (rc) return rc;
  }
  const size_t lds = (size_t)BC_VIL_WS_DOUBLES(d) * sizeof(double);
  if (lds > (size_t)ctx->max_lds) BC_REFUSE("%s: D = %d needs %zu bytes of LDS, a block has %d", who, d, lds, ctx->max_lds);
  rc = bc_ctx_refuse_busy(ctx, who, BC_HOLD_ALL);
  if (rc) return rc;
  // ---- nothing has been enqueued, allocated or written up to here
  BC_HIP(hipSetDevice(ctx->device));
  if (!ctx->laplace_small) ctx->laplace_small = new bc_lap_small();
  bc_lap_small* h = ctx->laplace_small;
  const bool shared = problem_stride == 0, factors = out_chol != nullptr;
  bc_slab in, out;
  const size_t i_rows = in.take(n_all * d), i_w = in.take(n_all), i_start = in.take(P * d), i_e = in.take(shared ? sd : P * sd);
  const size_t i_ptr = in.take(P + 1), i_flag = in.take((P + 1) / 2);      // (P + 1 int64; P ints)
  const size_t o_theta = out.take(t * d), o_mu = out.take(P * d), o_hd = out.take(P * d), o_val = out.take(P);
  const size_t o_chol = out.take(factors ? P * d * d : 0), o_inv = out.take(factors ? P * d * d : 0), o_cnt = out.take((3 * P + 1) / 2);
  rc = h->clock.create();
  if (!rc) rc = bc_stage_reserve(ctx, &h->in, in.total);
  if (!rc) rc = bc_scratch_grow(ctx, &h->work, 3 * n_all);
  if (!rc) rc = bc_scratch_grow(ctx, &h->out, out.total);
  if (!rc && zt) rc = bc_scratch_grow(ctx, &h->score, bc_even(t) + (t + 1) / 2);
  if (rc) return rc;
  BC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_laplace_many), hipFuncAttributeMaxDynamicSharedMemorySize, ctx->max_lds));
  BC_HIP(hipStreamSynchronize(ctx->stream));      // (the staging area: the last call's transfer has left it)
  double* pin = h->in.pin.p;
  memcpy(pin + i_rows, rows, n_all * d * sizeof(double));
  memcpy(pin + i_w, w, n_all * sizeof(double));
  if (start) memcpy(pin + i_start, start, P * d * sizeof(double));
  else memset(pin + i_start, 0, P * d * sizeof(double));
  if (shared) { if (sd) memcpy(pin + i_e, normals, sd * sizeof(double)); }
  else
    for (size_t p = 0; p < P; ++p) memcpy(pin + i_e + p * sd, normals + p * (size_t)problem_stride, sd * sizeof(double));
  memcpy(pin + i_ptr, row_ptr, (P + 1) * sizeof(int64_t));
  memset(pin + i_flag, 0, bc_even((P + 1) / 2) * sizeof(double));
  double* dev = h->in.dev.p;
  BC_HIP(hipMemcpyAsync(dev, pin, in.total * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  LmArgs a;
  memset(&a, 0, sizeof(a));
  a.rows = dev + i_rows;
  a.w = dev + i_w;
  a.row_ptr = reinterpret_cast<const long long*>(dev + i_ptr);
  a.start = dev + i_start;
  a.e = dev + i_e;
  a.e_stride = shared ? 0 : (long long)sd;
  a.rowc = h->work.p;
  a.flag = reinterpret_cast<int*>(dev + i_flag);
  double* o = h->out.p;
  a.theta = o + o_theta;
  a.mu = o + o_mu;
  a.hdiag = o + o_hd;
  a.value = o + o_val;
  a.chol = factors ? o + o_chol : nullptr;
  a.inv = factors ? o + o_inv : nullptr;
  a.counts = reinterpret_cast<int*>(o + o_cnt);
  a.d = d;
  a.s = s;
  a.diag = diag;
  h->clock.ms = 0.;
  rc = h->clock.start(ctx->stream);
  if (!rc) {
    hipLaunchKernelGGL(k_laplace_many, dim3((unsigned)P), dim3(BC_VIL_BLOCK), lds, ctx->stream, a);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) rc = bc_hip_fail(le, "k_laplace_many", __FILE__, __LINE__);
  }
  int* cor_dev = zt ? reinterpret_cast<int*>(h->score.p + bc_even(t)) : nullptr;
  // (the stream orders the scorer behind the fit; a marked problem's slice holds no draws: its scores are never copied)
  if (!rc && zt) rc = bc_score_launch(ctx, zt, yt, a.theta, (int64_t)t, cor_dev, h->score.p);
  if (!rc) rc = h->clock.stop(ctx->stream);
  BC_HIP(hipStreamSynchronize(ctx->stream));      // (after a failure too: nothing enqueued may outlive the call)
  if (rc) return rc;
  h->clock.collect();
  std::vector<int> flag(P);
  BC_HIP(hipMemcpy(flag.data(), a.flag, P * sizeof(int), hipMemcpyDeviceToHost));
  const size_t dd = (size_t)d * d;
  return bc_batch_unmarked_runs(flag.data(), P, out_status, [&](size_t p, size_t q) {
    const size_t k = q - p;
    BC_HIP(hipMemcpy(out_mu + p * d, a.mu + p * d, k * d * sizeof(double), hipMemcpyDeviceToHost));
    BC_HIP(hipMemcpy(out_hdiag + p * d, a.hdiag + p * d, k * d * sizeof(double), hipMemcpyDeviceToHost));
    BC_HIP(hipMemcpy(out_value + p, a.value + p, k * sizeof(double), hipMemcpyDeviceToHost));
    BC_HIP(hipMemcpy(out_counts + 3 * p, a.counts + 3 * p, 3 * k * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (factors) {
      BC_HIP(hipMemcpy(out_chol + p * dd, a.chol + p * dd, k * dd * sizeof(double), hipMemcpyDeviceToHost));
      BC_HIP(hipMemcpy(out_inv + p * dd, a.inv + p * dd, k * dd * sizeof(double), hipMemcpyDeviceToHost));
    }
    if (out_theta && sd) BC_HIP(hipMemcpy(out_theta + p * sd, a.theta + p * sd, k * sd * sizeof(double), hipMemcpyDeviceToHost));
    if (out_ll) {
      BC_HIP(hipMemcpy(out_ll + p * s, h->score.p + p * s, k * s * sizeof(double), hipMemcpyDeviceToHost));
      BC_HIP(hipMemcpy(out_correct + p * s, cor_dev + p * s, k * s * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    return BC_OK;
  });
}

extern "C" int bc_laplace_small_device_ms(bc_ctx* ctx, double* out_ms) {
  return bc_device_ms("bc_laplace_small_device_ms", ctx, ctx && ctx->laplace_small ? &ctx->laplace_small->clock : nullptr, out_ms);
}
