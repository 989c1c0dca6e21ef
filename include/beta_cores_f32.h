/*
 * beta_cores_f32.h -- C ABI of float32 data rows in libbeta_cores.
 *
 * An extension of include/beta_cores.h (same library, same conventions: int status, bc_last_error(), host pointers
 * borrowed for the call); kept in a header of its own so that the core ABI of beta_cores.h stays as it is.
 * Bound in Python by beta_cores_amd/_native.py (_F32_SIGNATURES).
 *
 * A bc_data made here stores its rows as row-major n_rows x dz IEEE float (4 bytes per element: half the bytes on the
 * host link and half the HBM of a float64 handle).  Only the STORAGE is float32: every kernel that reads the rows widens
 * them to double in registers, which is exact, and computes in double as before -- so a projection, Gram matrix or Newton
 * pass over float32 rows has the bits the float64 path gives over the same rows widened on the host.  Nothing is ever
 * rounded to float32: Phi, norms, column sums, Theta, weights, parameters and every output stay double.
 *
 * The entry points of beta_cores.h / beta_cores_laplace.h that take a `const bc_data*` dispatch on the stored type:
 *   serve float32 rows:  bc_project, bc_project_colsum, bc_vi_gradient(_begin/_end) (the data rows; the coreset rows are
 *                        host doubles), bc_data_gather_rows (output stays double), bc_data_zero_feature_keys,
 *                        bc_weighted_gram, bc_logistic_newton_pass (the rows; the weights handle must be float64)
 *   refuse them (BC_INVALID_ARGUMENT, the message names the dtype):
 *                        bc_data_upload (its source is doubles), bc_project_grad_x (serves the pseudo-points, which live
 *                        in float64 slots), a float32 weights handle of bc_logistic_newton_pass
 */
#ifndef BETA_CORES_F32_H
#define BETA_CORES_F32_H

#include "beta_cores.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rows from a host float array: uploaded as they are (4 bytes per element), like bc_data_from_host */
int bc_data_from_host_f32(bc_ctx* ctx, const float* z_rowmajor, int64_t n_rows, int32_t dz, bc_data** out);
/* borrow a device float array (e.g. a torch.float32 tensor): no copy, the caller keeps it alive, like bc_data_from_device */
int bc_data_from_device_f32(bc_ctx* ctx, const float* z_dev, int64_t n_rows, int32_t dz, bc_data** out);
/* bc_project_from_host for a host float array: the same pipelined upload + K1 per chunk (chunks are aligned in ROWS as
 * there, so Phi, norms and column sums are bc_project's over the resident float32 rows bit for bit); *out_data receives the
 * resident float32 rows */
int bc_project_from_host_f32(bc_ctx* ctx, const float* z_host, int64_t n_rows, int32_t dz, int model, const double* theta,
                             int32_t s, const double* params, int32_t n_params, int64_t row_offset, bc_data** out_data,
                             bc_phi** inout);
/* bytes per stored element of a handle -> *out_bytes: 8 (float64) or 4 (float32) */
int bc_data_elem_bytes(const bc_data* data, int32_t* out_bytes);

#ifdef __cplusplus
}
#endif
#endif /* BETA_CORES_F32_H */
