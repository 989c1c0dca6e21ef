// k_psvi_point_grad: BatchPSVICoreset's gradient with respect to its pseudo-points (include/beta_cores_psvi.h) without the
// M x S x W tensor of x-gradients: one work-group per point, the arithmetic of bc_psvi_dev.h.  The work is a few MFlop and
// latency-bound: what counts is that the M groups spread over the CUs, that a group's dependent chain is short (a wave-level
// dot product per sample, then one S-term fma chain per coordinate with eight loads in flight) and that nothing goes back to
// the host in between -- it runs behind k_vi_gradient on the context's stream and reads Theta where K1's staging has put it.
#include "bc_internal.h"
#include "bc_psvi_dev.h"

__global__ __launch_bounds__(256) void k_psvi_point_grad(PsviArgs a) {
  extern __shared__ __attribute__((aligned(16))) double psvi_ws[];      // BC_PSVI_WS_DOUBLES(dz, s)
  bc_psvi_point_grad(a, (int)blockIdx.x, psvi_ws);
}

int bc_psvi_kind(int model) {
  return model == BC_MODEL_LINREG_LL ? BC_PSVI_LINREG : model == BC_MODEL_LOGISTIC_LL ? BC_PSVI_LOGISTIC
       : model == BC_MODEL_GAUSS_LL ? BC_PSVI_GAUSS : -1;
}

int bc_psvi_max_dz(void) { return BC_PSVI_MAX_DZ; }

// g_p [m][dz] for points, weights, Theta (pitch dk), Siginv and resid that are already on the device; enqueued only
int bc_psvi_point_grad_launch(bc_ctx* ctx, int model, const double* pts_dev, const double* w_dev, int64_t m, int dz, int d,
                              int32_t s, const double* theta_dev, int dk, const double* siginv_dev, double sigsq,
                              const double* resid_dev, double* out_dev) {
  PsviArgs a;
  a.kind = bc_psvi_kind(model);
  if (a.kind < 0 || m <= 0 || m > (1 << 20) || dz <= 0 || dz > BC_PSVI_MAX_DZ || d <= 0 || d > dz || dk < d || s <= 0 || s > 256 ||
      (a.kind == BC_PSVI_GAUSS) != (siginv_dev != nullptr)) {
    bc_set_error("bc_psvi_gradient: internal: bad launch shape (model %d, m = %lld, dz = %d, S = %d)", model, (long long)m, dz, s);
    return BC_INVALID_ARGUMENT;
  }
  a.m = (int)m; a.s = s; a.d = d; a.dz = dz; a.dk = dk;
  a.pts = pts_dev; a.w = w_dev; a.theta = theta_dev; a.siginv = siginv_dev; a.resid = resid_dev; a.sigsq = sigsq; a.out = out_dev;
  const size_t lds = BC_PSVI_WS_DOUBLES(dz, s) * sizeof(double);      // <= 64 KiB by BC_PSVI_MAX_DZ
  hipLaunchKernelGGL(k_psvi_point_grad, dim3((unsigned)m), dim3(256), lds, ctx->stream, a);
  BC_HIP(hipGetLastError());
  return BC_OK;
}
