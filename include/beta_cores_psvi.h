/*
 * beta_cores_psvi.h -- C ABI of the fused gradient of BatchPSVICoreset (bayesiancoresets/coreset/bpsvi.py:47-57) in
 * libbeta_cores: the gradient with respect to the weights AND the pseudo-points in one native call.
 *
 * An extension of include/beta_cores.h (same library, same conventions: int status, bc_last_error(), host pointers
 * borrowed for the call); kept in a header of its own so that the ABI of the existing headers stays as it is.
 * Bound in Python by beta_cores_amd/_native.py (_PSVI_SIGNATURES).
 *
 * With corevecs = the row-centred projection of the m pseudo-points, target = sum_scaling * the column sums of the
 * row-centred projection of the data rows, and G (m x S x W) the x-gradient tensor bc_project_grad_x returns (centred over
 * its last axis), the reference forms
 *   resid  = target - w . corevecs                                            (S)
 *   grad_w = -corevecs . resid / S                                            (m)
 *   grad_p = -sum_s ( w[:, None, None] * G * resid[None, :, None] ) / S       (m x W)
 * Centring over the coordinates commutes with the sum over the samples, so grad_p needs only
 *   V[i, c] = sum_s resid[s] * Gu[i, s, c]     (Gu: G before centring),     grad_p[i, c] = -(w[i] / S) (V[i, c] - mean_c V[i, :])
 * and the tensor is never formed: k_psvi_point_grad (csrc/bc_psvi.hip, the arithmetic of csrc/bc_psvi_dev.h) computes one
 * row of grad_p per work-group from the points, the Theta and the Siginv that the call has staged anyway.
 *
 * grad_w and resid come from the same kernels on the same staged data as bc_vi_gradient's (beta_cores.h): for the same inputs
 * they carry the same bits.  grad_p equals the reference's expression to rounding; every sum in it has a fixed order, so a
 * repeated call returns the same bits.  For BC_MODEL_GAUSS_LL the kernel reads Theta' = (Siginv . Theta^T)^T from K1's
 * staging in place of Theta . Siginv: the two agree for a symmetric Siginv, which is what a precision matrix is.
 */
#ifndef BETA_CORES_PSVI_H
#define BETA_CORES_PSVI_H

#include "beta_cores.h"

#ifdef __cplusplus
extern "C" {
#endif

/* First half: stage Theta, the points and w (one transfer), enqueue the projections, the m x S algebra, the point-gradient
 * kernel and ONE download into a pinned area; returns without waiting.
 *   data:   the data rows (float64 or float32, include/beta_cores_f32.h), through the store-free K1
 *   points: host, m x dz float64 (dz = the width of the data rows; W = dz for all three models)
 *   model:  BC_MODEL_LINREG_LL (params = {sigsq}, rows [x, y]), BC_MODEL_LOGISTIC_LL (no params, rows y*x) or
 *           BC_MODEL_GAUSS_LL (params = {logdetSig, Siginv[d*d]}); any other model has no x-gradient and is refused
 *   limits: 1 <= s <= 256, m >= 1, dz <= 3840, and the staging area must hold m + s + m*dz doubles
 * A shape outside the limits, a NULL argument or data of another context returns BC_INVALID_ARGUMENT before anything is
 * enqueued.  There is no communicator: BatchPSVICoreset does not run on row shards.
 * ONE gradient of any kind (this one, bc_vi_gradient's, the beta-gradient's of beta_cores_betagrad.h) can be pending per
 * context: while it is, a _begin of any kind is refused, an _end of another kind is refused and leaves it pending, and the
 * device weight optimisation of beta_cores_viopt.h cannot be begun. */
int bc_psvi_gradient_begin(bc_ctx* ctx, const bc_data* data, const double* points, int64_t m, int model,
                           const double* theta, int32_t s, const double* params, int32_t n_params, const double* w,
                           double sum_scaling);
/* Second half: wait for the download and hand it out.  out_grad_w: m, out_grad_p: m x dz, out_resid: s or NULL */
int bc_psvi_gradient_end(bc_ctx* ctx, double* out_grad_w, double* out_grad_p, double* out_resid);
/* the two in one */
int bc_psvi_gradient(bc_ctx* ctx, const bc_data* data, const double* points, int64_t m, int model,
                     const double* theta, int32_t s, const double* params, int32_t n_params, const double* w,
                     double sum_scaling, double* out_grad_w, double* out_grad_p, double* out_resid);

#ifdef __cplusplus
}
#endif
#endif /* BETA_CORES_PSVI_H */
