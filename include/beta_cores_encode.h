/*
 * beta_cores_encode.h -- C ABI of the device feature encoder in libbeta_cores.
 *
 * An extension of include/beta_cores.h (same library, same conventions: int status, bc_last_error(), host pointers
 * borrowed for the call); kept in a header of its own so that the ABI of the existing headers stays as it is.
 * Bound in Python by beta_cores_amd/_native.py (_ENCODE_SIGNATURES).
 *
 * The neural-linear model evaluates the linear-regression formula on [features(x), y], where features() is a small learned
 * network (Linear -> BatchNorm -> ReLU, twice).  An encoder is that network with its parameters resident on the device;
 * bc_data_encode turns resident raw rows into resident encoded rows, which bc_project, bc_project_colsum and bc_vi_gradient
 * then take like any other bc_data.
 *
 * An encoder has L <= 4 layers; layer l maps width d[l] to d[l+1], every width in 1..512:
 *     h <- act((W h + b) * s + t)
 * W is d[l+1] x d[l], row-major; b, s, t are per-output vectors (an eval-mode batch norm folds into s and t); act is ReLU or
 * the identity.  All parameters and all arithmetic are float64.  ReLU passes a NaN through.
 */
#ifndef BETA_CORES_ENCODE_H
#define BETA_CORES_ENCODE_H

#include "beta_cores.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bc_encoder bc_encoder;

/* An encoder of n_layers layers (1..4) on ctx; widths holds the n_layers + 1 widths d[0] .. d[L] (each 1..512).  Its
 * parameters are unset: every layer needs a bc_encoder_set_layer before the encoder can be used. */
int bc_encoder_create(bc_ctx* ctx, int32_t n_layers, const int32_t* widths, bc_encoder** out);

/* The parameters of one layer, from HOST arrays borrowed for the call (they have been read when it returns): W is
 * d[layer+1] x d[layer] row-major; b, s, t hold d[layer+1] values each, NULL meaning all 0 / all 1 / all 0; relu != 0
 * applies ReLU.  The copy is ordered on the context's stream: calls on the same context issued earlier use the old
 * parameters, calls issued later the new ones. */
int bc_encoder_set_layer(bc_encoder* enc, int32_t layer, const double* W, const double* b, const double* s, const double* t,
                         int32_t relu);

int bc_encoder_destroy(bc_encoder* enc);

/* out[j] = [ mlp(src[j, :d[0]]), src[j, d[0]:] ] for every row of src, on the device.
 *   src: n x (d[0] + pass_cols) rows, stored as float64 or float32 (widened exactly); pass_cols >= 0 trailing columns are
 *        carried over unchanged.
 *   out_elem_bytes: 8 stores the result as float64, 4 as float32 -- each value of the float64 result rounded once, to
 *        nearest; pass-through columns of a float32 source are copied exactly.
 *   *inout == NULL: a new owned handle of n x (d[L] + pass_cols) is allocated.  Otherwise *inout is re-used (and grown, as
 *        bc_data_upload grows): it must be an owned handle of the same context, column count and element size, and must
 *        not be src.
 *   Refused (BC_INVALID_ARGUMENT, the message names the offender): a layer never set, a source whose width is not
 *        d[0] + pass_cols, pass_cols < 0, an element size other than 4 or 8.
 *   A refused call leaves *inout and the rows it holds untouched.  n == 0 is valid and yields a handle of 0 rows.
 * A row's features depend on that row and the parameters alone: they have the same bits whichever rows accompany it and
 * whichever storage types are involved.  The call is enqueued on the context's stream and not waited for. */
int bc_data_encode(const bc_encoder* enc, const bc_data* src, int32_t pass_cols, int32_t out_elem_bytes, bc_data** inout);

#ifdef __cplusplus
}
#endif
#endif /* BETA_CORES_ENCODE_H */
