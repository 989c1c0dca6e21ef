// The chain summary (include/beta_cores_diag.h) for the units that run it: bc_diag.hip has the kernels and the stand-alone entry,
// bc_hmc_small.hip the entries attached to its run.  Host only.
#pragma once
#include "bc_internal.h"
#include "../../include/beta_cores_diag.h"

struct bc_diag_shape {
  int64_t p = 0, n = 0;
  int32_t c = 0, d = 0;
  int64_t max_lag = 0;
};

// the host arrays of include/beta_cores_diag.h (rho and moments may be null)
struct bc_diag_out {
  double *mean, *cov, *rhat, *ess;
  int32_t *truncated, *status;
  double *rho, *moments;
};

// what an attached summary keeps between its calls (a member of the run it is attached to)
struct bc_diag_attached {
  bool on = false;           // between bc_diag_attach and bc_diag_end
  bool folded = false;       // the pending chunk has been folded in
  int64_t n_keep = 0, kept = 0, max_lag = 0;
  bc_scratch keep, work;     // the retained draws [p][j][c][i]; bc_diag_run's work space
};

// the limits of the header (the cap on the work space included); `who` names the entry point in the message
int bc_diag_check(const char* who, const bc_diag_shape& s);
// the doubles of the retained layout, and of bc_diag_run's work space (bc_diag_work_doubles = 2 x the first + the second)
size_t bc_diag_keep_doubles(const bc_diag_shape& s);
size_t bc_diag_run_doubles(const bc_diag_shape& s);
// k_diag_keep: src_dev [p][k][c][d] -> keep_dev [p][d][c][n] at iterations i0 .. i0 + k - 1 (i0 + k <= n); enqueued only
int bc_diag_keep_launch(bc_ctx* ctx, const double* src_dev, const bc_diag_shape& s, int64_t k, int64_t i0, double* keep_dev);
// the summary of keep_dev into the host arrays: enqueues the kernels, waits and copies.  marks_dev: [p] ints of problems that are
// already marked, or null.  work_dev: bc_diag_run_doubles(s) doubles.
int bc_diag_run(bc_ctx* ctx, const double* keep_dev, double* work_dev, const bc_diag_shape& s, const int* marks_dev, const bc_diag_out& out);
// the outputs an entry point requires are there
bool bc_diag_out_ok(const bc_diag_out& out);
