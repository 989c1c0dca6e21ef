// A batch of small problems packed as rows | w | row_ptr (bc_hmc_small.hip, bc_laplace_small.hip, bc_psvi_many.hip): the walk
// over row_ptr before anything is touched, and what the per-problem marks become when the results are handed out.  Host only.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/beta_cores.h"

void bc_set_error(const char* fmt, ...);

// row_ptr [n_problems + 1] must begin at 0 and increase strictly, by at most `cap` per problem.  `holds`: what a problem
// holds ("rows", "points").  *largest: the largest problem (with BC_OK).
static inline int bc_batch_walk(const char* who, const int64_t* row_ptr, int32_t n_problems, int64_t cap, const char* holds, int64_t* largest) {
  if (row_ptr[0] != 0) return bc_set_error("%s: row_ptr[0] must be 0, got %lld", who, (long long)row_ptr[0]), BC_INVALID_ARGUMENT;
  *largest = 0;
  for (int32_t p = 0; p < n_problems; ++p) {
    const int64_t n = row_ptr[p + 1] - row_ptr[p];
    if (n > *largest) *largest = n;
    if (n >= 1 && n <= cap) continue;
    bc_set_error("%s: problem %d has %lld %s, 1 .. %lld are served (row_ptr must increase strictly: row_ptr[%d] = %lld, row_ptr[%d] = %lld)",
                 who, p, (long long)n, holds, (long long)cap, p, (long long)row_ptr[p], p + 1, (long long)row_ptr[p + 1]);
    return BC_INVALID_ARGUMENT;
  }
  return BC_OK;
}

// out_status[p] = BC_NUMERICAL_PRECISION for a marked problem (flag[p] != 0) and BC_OK otherwise.  The results of
// runs of consecutive unmarked problems are copied together (one run of all P when nothing is marked): copy(p, q) is called
// once per maximal run [p, q), and what it returns ends the walk if it is not BC_OK.
template <typename F>
static inline int bc_batch_unmarked_runs(const int* flag, size_t n_problems, int32_t* out_status, F&& copy) {
  for (size_t p = 0, q; p < n_problems; p = q) {
    for (q = p; q < n_problems && flag[q] != 0; ++q) out_status[q] = BC_NUMERICAL_PRECISION;      // the marked ones in front of a run
    for (p = q; q < n_problems && flag[q] == 0; ++q) out_status[q] = BC_OK;                       // the run [p, q)
    const int rc = q > p ? copy(p, q) : BC_OK;
    if (rc != BC_OK) return rc;
  }
  return BC_OK;
}
