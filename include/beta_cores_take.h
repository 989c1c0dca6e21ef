/*
 * beta_cores_take.h -- C ABI of the on-device row sub-sample in libbeta_cores.
 *
 * An extension of include/beta_cores.h (same library, same conventions: int status, bc_last_error(), host pointers
 * borrowed for the call); kept in a header of its own so that the ABI of the existing headers stays as it is.
 * Bound in Python by beta_cores_amd/_native.py (_TAKE_SIGNATURES).
 *
 * A sub-sampled tangent space needs m of the n resident rows as a bc_data of their own (bc_project, bc_project_colsum and
 * bc_vi_gradient take one).  bc_data_gather_rows brings such rows to the HOST as doubles, from where they would be uploaded
 * again; the entry point below keeps them in HBM.
 */
#ifndef BETA_CORES_TAKE_H
#define BETA_CORES_TAKE_H

#include "beta_cores.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out[j, :] = src[idx[j], :] for j < m, on the device, in src's storage type (float64 or float32: words are copied, never
 * converted).
 *   idx: HOST array of LOCAL row numbers, borrowed for the call only; repeats allowed.  Every index is checked before
 *        anything is enqueued: one that is negative or >= the row count is refused (BC_INVALID_ARGUMENT, the message names
 *        the first offender).
 *   *inout == NULL: a new owned handle is allocated.  Otherwise *inout is re-used (and grown, as bc_data_upload grows): it
 *        must be an owned handle of the same context, column count and element size, and must not be src.
 *   A refused call leaves *inout and the rows it holds untouched.  m == 0 is valid and yields a handle of 0 rows.
 * The copy is enqueued on the context's stream and not waited for: as with every producer in this library, calls on the same
 * context see the rows.  Into a re-used handle that is large enough the call allocates and frees nothing. */
int bc_data_take_rows(const bc_data* src, const int64_t* idx, int64_t m, bc_data** inout);

#ifdef __cplusplus
}
#endif
#endif /* BETA_CORES_TAKE_H */
