// The solver's side of the diagnostic seam into the sweep's pre-filter (include/beta_cores_prefdiag.h): the three
// bc_snnls_prefdiag_* entry points and the one-wave kernel that quantises an uploaded vector with the step kernels' functions.
// TEST AIDS: the product calls nothing in this unit, and bc_snnls.hip knows nothing of it.  The pre-filter's side is the last
// block of bc_pref.h, defined in bc_prefilter.hip.
#include "bc_snnls_state.h"
#include "bc_i8_quant.h"
#include "bc_i4_quant.h"
#include "../../include/beta_cores_prefdiag.h"
#include <cmath>
#include <cstring>

extern "C" int bc_snnls_prefdiag_info(const bc_snnls* h, int64_t* out) {
  if (!h || !out) { bc_set_error("bc_snnls_prefdiag_info: bad argument"); return BC_INVALID_ARGUMENT; }
  for (int i = 0; i < BC_PREFDIAG_INFO_N; ++i) out[i] = 0;
  if (h->pref) bc_pref_diag_info(h->pref, h->d.qv != nullptr, out);
  return BC_OK;
}

extern "C" int bc_snnls_prefdiag_copy(const bc_snnls* h, const char* which, void* out, int64_t cap_bytes, int64_t* bytes) {
  if (!h || !which) { bc_set_error("bc_snnls_prefdiag_copy: bad argument"); return BC_INVALID_ARGUMENT; }
  if (bytes) *bytes = 0;
  if (!h->pref) { bc_set_error("bc_snnls_prefdiag_copy: this solver has no pre-filter"); return BC_INVALID_ARGUMENT; }
  const void* dev = nullptr;
  size_t n = 0;
  const double one = 1.0;
  const void* host = nullptr;
  const int s = h->d.s;
  if (strcmp(which, "v") == 0) { dev = h->d.v; n = (size_t)(h->alg == BC_ALG_GIGA ? 2 * s : s) * sizeof(double); }
  else if (strcmp(which, "v_norm") == 0) { n = sizeof(double); if (h->alg == BC_ALG_GIGA) host = &one; else dev = &h->d.st->v_norm; }
  else if (strcmp(which, "post_div") == 0) { n = sizeof(double); host = &one; }
  else if (strcmp(which, "qv") == 0 || strcmp(which, "qv4") == 0) {
    const bool four = which[2] == '4';
    dev = four ? (const void*)h->d.qv4 : (const void*)h->d.qv;
    n = (four ? (size_t)BC_I4Q_INTS(h->d.sp8) : (size_t)BC_I8Q_INTS(h->d.sp4)) * sizeof(int);
    if (!dev) { bc_set_error("bc_snnls_prefdiag_copy: this solver keeps no \"%s\" record", which); return BC_INVALID_ARGUMENT; }
  } else {
    const int rc = bc_pref_diag_buffer(h->pref, which, &dev, &n);
    if (rc == 1) { bc_set_error("bc_snnls_prefdiag_copy: unknown buffer \"%s\"", which); return BC_INVALID_ARGUMENT; }
    if (rc == 2) { bc_set_error("bc_snnls_prefdiag_copy: this solver's pre-filter has no buffer \"%s\"", which); return BC_INVALID_ARGUMENT; }
  }
  if (bytes) *bytes = (int64_t)n;
  if (!out || cap_bytes < (int64_t)n) {
    bc_set_error("bc_snnls_prefdiag_copy: \"%s\" holds %zu bytes, the caller offers %lld", which, n, (long long)cap_bytes);
    return BC_INVALID_ARGUMENT;
  }
  BC_HIP(hipStreamSynchronize(h->ctx->stream));
  if (host) memcpy(out, host, n);
  else BC_HIP(hipMemcpy(out, dev, n, hipMemcpyDeviceToHost));
  return BC_OK;
}

// one wave: both digit records of a vector that did not come out of a step kernel, with the step kernels' functions
template <int MODE>
__global__ __launch_bounds__(64) void k_prefdiag_quant(const double* __restrict__ v, int s, int sp4, int sp8, int* __restrict__ qv,
                                                       int* __restrict__ qv4, double* __restrict__ v_norm) {
  const int lane = threadIdx.x;
  double m0 = 0., m1 = 0., vn = 0.;
  for (int k = lane; k < s; k += BC_WAVE) {
    if (MODE == 0) {
      m0 = bc_i8q_absmax(m0, v[2 * k]);
      m1 = bc_i8q_absmax(m1, v[2 * k + 1]);
    } else {
      m0 = bc_i8q_absmax(m0, v[k]);
      vn = fma(v[k], v[k], vn);
    }
  }
  const double vnorm = (MODE == 0) ? 1. : sqrt(bc_wave_sum(vn));      // (as dev_prep: GIGA's are unit vectors)
  if (lane == 0) *v_norm = vnorm;
  bc_i8q_wave<MODE>(v, s, sp4, vnorm, qv, lane, m0, m1);
  if (qv4 != nullptr) bc_i4q_wave<MODE>(v, s, sp8, vnorm, qv4, lane, bc_wave_max_all(m0), bc_wave_max_all(m1));
}

extern "C" int bc_snnls_prefdiag_sweep(bc_snnls* h, int32_t mode, const double* v, double post_div, int32_t self_quantise, float* out_ul,
                                       float* out_ul8, float* out_theta0, int64_t rows_cap, int32_t blocks_cap, int32_t* form_run) {
  if (!h || !out_ul || !form_run || mode < 0 || mode > 1) { bc_set_error("bc_snnls_prefdiag_sweep: bad argument"); return BC_INVALID_ARGUMENT; }
  if (!h->pref) { bc_set_error("bc_snnls_prefdiag_sweep: this solver has no pre-filter"); return BC_INVALID_ARGUMENT; }
  int64_t info[BC_PREFDIAG_INFO_N];
  bc_pref_diag_info(h->pref, h->d.qv != nullptr, info);
  if (info[BC_PREFDIAG_PREC] != 8 || info[BC_PREFDIAG_NEXT_FORM] == 2) {
    bc_set_error("bc_snnls_prefdiag_sweep: only the one-level int8 sweep and the two-level form have a per-row output (this solver: "
                 "precision %d, form %d)", (int)info[BC_PREFDIAG_PREC], (int)info[BC_PREFDIAG_NEXT_FORM]);
    return BC_INVALID_ARGUMENT;
  }
  if (h->rs_pending) { bc_set_error("bc_snnls_prefdiag_sweep: a step is in flight"); return BC_INVALID_ARGUMENT; }
  if (!(post_div == post_div) || post_div == 0. || fabs(post_div) > 1.7976931348623157e308) {
    bc_set_error("bc_snnls_prefdiag_sweep: post_div must be finite and non-zero");
    return BC_INVALID_ARGUMENT;
  }
  if (!v && mode != mode_of(h)) {
    bc_set_error("bc_snnls_prefdiag_sweep: the solver's own vectors are those of mode %d", mode_of(h));
    return BC_INVALID_ARGUMENT;
  }
  const int s = h->d.s;
  if (v && mode == 0) {
    double n0 = 0., n1 = 0.;
    for (int k = 0; k < s; ++k) { n0 += v[2 * k] * v[2 * k]; n1 += v[2 * k + 1] * v[2 * k + 1]; }
    n0 = sqrt(n0); n1 = sqrt(n1);
    if (fabs(n0 - 1.) > 1e-9 || fabs(n1 - 1.) > 1e-9) {
      bc_set_error("bc_snnls_prefdiag_sweep: the GIGA sweep takes unit vectors (norms %.12g, %.12g)", n0, n1);
      return BC_INVALID_ARGUMENT;
    }
  }
  // the digit records this sweep reads: the solver's own, or those of the uploaded vector
  const bool own = v == nullptr;
  const bool two = info[BC_PREFDIAG_NEXT_FORM] == 3 && (own ? h->d.qv4 != nullptr : true);
  if (two && self_quantise) { bc_set_error("bc_snnls_prefdiag_sweep: the two-level form reads digit records (self_quantise)"); return BC_INVALID_ARGUMENT; }
  const int64_t rows = info[BC_PREFDIAG_PTILES] * 256;
  if (rows_cap < rows) { bc_set_error("bc_snnls_prefdiag_sweep: %lld rows of output, the caller offers %lld", (long long)rows, (long long)rows_cap); return BC_INVALID_ARGUMENT; }
  if (two && (!out_ul8 || !out_theta0 || blocks_cap < info[BC_PREFDIAG_GRID1])) {
    bc_set_error("bc_snnls_prefdiag_sweep: the two-level form needs out_ul8 and out_theta0[%d]", (int)info[BC_PREFDIAG_GRID1]);
    return BC_INVALID_ARGUMENT;
  }
  BC_HIP(hipStreamSynchronize(h->ctx->stream));
  const int grid1 = (int)info[BC_PREFDIAG_GRID1];
  const size_t o_d1 = 0, o_d2 = o_d1 + bc_up256((size_t)rows * sizeof(float2)), o_th = o_d2 + bc_up256(two ? (size_t)rows * sizeof(float2) : 0),
               o_v = o_th + bc_up256((size_t)(grid1 > 0 ? grid1 : 1) * sizeof(float)), o_vn = o_v + bc_up256(2 * (size_t)(s + BC_V_PAD) * sizeof(double)),
               o_qv = o_vn + bc_up256(sizeof(double)), o_qv4 = o_qv + bc_up256((size_t)BC_I8Q_INTS(h->d.sp4) * sizeof(int)),
               o_save = o_qv4 + bc_up256((size_t)BC_I4Q_INTS(h->d.sp8) * sizeof(int)), total = o_save + bc_up256(bc_pref_diag_save_bytes());
  char* sc = nullptr;
  BC_HIP(hipMalloc((void**)&sc, total));
  hipStream_t st = h->ctx->stream;
  int rc = BC_OK, form = 0;
  auto hip = [&](hipError_t e, const char* what) { if (e != hipSuccess && rc == BC_OK) rc = bc_hip_fail(e, what, __FILE__, __LINE__); };
  hip(hipMemsetAsync(sc + o_v, 0, total - o_v, st), "hipMemsetAsync(prefdiag)");
  const double* v_dev = h->d.v;
  const double* vn_dev = &h->d.st->v_norm;
  const int* qv = self_quantise ? nullptr : h->d.qv;
  const int* qv4 = h->d.qv4;
  if (!own && rc == BC_OK) {
    hip(hipMemcpyAsync(sc + o_v, v, (size_t)(mode == 0 ? 2 * s : s) * sizeof(double), hipMemcpyHostToDevice, st), "hipMemcpyAsync(prefdiag v)");
    v_dev = (const double*)(sc + o_v);
    vn_dev = (const double*)(sc + o_vn);
    int* q8 = (int*)(sc + o_qv);
    int* q4 = two ? (int*)(sc + o_qv4) : nullptr;
    if (rc == BC_OK) {
      if (mode == 0) hipLaunchKernelGGL(k_prefdiag_quant<0>, dim3(1), dim3(64), 0, st, v_dev, s, h->d.sp4, h->d.sp8, q8, q4, (double*)(sc + o_vn));
      else hipLaunchKernelGGL(k_prefdiag_quant<1>, dim3(1), dim3(64), 0, st, v_dev, s, h->d.sp4, h->d.sp8, q8, q4, (double*)(sc + o_vn));
      hip(hipGetLastError(), "k_prefdiag_quant");
    }
    qv = self_quantise ? nullptr : q8;
    qv4 = q4;
  }
  if (rc == BC_OK)
    rc = bc_pref_diag_sweep(h->pref, mode, v_dev, vn_dev, qv, two ? qv4 : nullptr, post_div, (float2*)(sc + o_d1), (float2*)(sc + o_d2),
                            (float*)(sc + o_th), sc + o_save, &form);
  if (rc == BC_OK && (form == 3) != two) { bc_set_error("bc_snnls_prefdiag_sweep: internal: form %d", form); rc = BC_INVALID_ARGUMENT; }
  if (rc == BC_OK) hip(hipMemcpyAsync(out_ul, sc + o_d1, (size_t)rows * sizeof(float2), hipMemcpyDeviceToHost, st), "hipMemcpyAsync(prefdiag out)");
  if (rc == BC_OK && two) {
    hip(hipMemcpyAsync(out_ul8, sc + o_d2, (size_t)rows * sizeof(float2), hipMemcpyDeviceToHost, st), "hipMemcpyAsync(prefdiag out8)");
    hip(hipMemcpyAsync(out_theta0, sc + o_th, (size_t)grid1 * sizeof(float), hipMemcpyDeviceToHost, st), "hipMemcpyAsync(prefdiag theta0)");
  }
  const hipError_t es = hipStreamSynchronize(st);
  hip(es, "hipStreamSynchronize(prefdiag)");
  (void)hipFree(sc);
  *form_run = form;
  return rc;
}
