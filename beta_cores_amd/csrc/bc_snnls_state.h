// What the sparse-NNLS solver is: its state on the device (SnnlsState), the argument block its single-block kernels take by
// value (SnnlsDev), the handle (struct bc_snnls), and the constants the kernels and the host both use.  No kernel and no
// __device__ function in here.  Included by bc_snnls.hip (the kernels and the host side; its device functions are
// bc_snnls_dev.h) and by bc_snnls_diag.hip (the test aids of include/beta_cores_prefdiag.h); no other unit sees inside a handle.
// SnnlsDev and RescoreArgs are kernel arguments: their member order is the kernels' argument layout.
#pragma once
#include "bc_internal.h"
#include "bc_pref.h"

#define BC_FIN_THREADS 512        // threads of every single-block kernel of the solver
#define BC_PF_MAXNNZ 1024         // list entries and record doubles the one-round finish kernel (k_step_finish_pf) can hold in
#define BC_PF_MAXREC 2048         // LDS / registers: the host takes the plain kernel beyond them (finish_pf_ok)
#define BC_ST_LIST_LIMIT 100      // last_status of k_refit: the list would outgrow BC_NNLS_MAXP (the host words the error)

struct SnnlsState {
  long long nnz;        // length of the (idx, val) list, selection order; val may be 0
  long long npos;       // count(val > 0)  == SparseNNLS.size()
  long long iter;       // consumed iterations since reset (trace length)
  long long sel_f;      // last picked global index, -1 if none
  double sel_score;
  double sel_norm;
  double err_cur;       // ||A.w - b||_2 for the current w
  double xw_sq;         // ||A.w||^2 for the current w
  int skip;             // select_fail | reached_limit : makes the next sweep a no-op
  int reached_limit;
  int retried;
  int select_fail;      // the reference's _select would raise (giga.py:28-29)
  int sel_valid;
  int last_status;      // status of the last step-wise call
  int overflow;         // list capacity exceeded (host bug guard)
  int pf_overflow;      // the pre-filter's candidate lists overflowed in this step: nothing was consumed, the host
                        // re-runs the step with the exact fp64 sweep (sticky until it does; later launches are no-ops)
  double v_norm;        // ||v|| of the dot-mode sweep vector (scales the pre-filter's error bound)
};

struct SnnlsDev {
  SnnlsState* st;
  long long* idx;
  double* val;
  double* prev_val;
  double* cols;       // [cap][s]
  double* colnorm;    // [cap]
  long long cap;
  double* b;
  double* bn;
  double* xw;
  double* xw_prev;
  double* v;          // sweep vectors: GIGA [s][2], else [s]
  int* qv;            // the same, quantised for the int8 pre-filter's sweep (bc_i8_quant.h record) -- or nullptr
  int sp4;            // k-groups of that record
  int* qv4;           // two-level pre-filter: the same in 4-bit digits for its first level (bc_i4_quant.h record) -- or nullptr
  int sp8;            // k-groups of that record
  double* xf;         // picked column
  const double* cand_all;
  const double* tiles;
  const double* norms;
  long long n_rows, row_offset;
  long long* tr_f;
  int* tr_status;
  double* tr_err;
  long long tr_cap;
  double bnorm, tol, norm_sum;
  int s, world, rec_len;
  // single-rank fast path: the finish kernel reduces the sweep's per-block candidates itself
  const double* blk_val;
  const long long* blk_idx;
  int nblk;
  int fuse_winner;
  // device NNLS refit (bc_nnls_dev.h): Gram matrix of the list's cached columns [BC_NNLS_MAXP][BC_NNLS_MAXP], its right-hand
  // side cols . b, and {refits, solves, rejected, covered}: the refit counters and the number of leading list entries the Gram
  // state covers -- written by the kernels that extend it, lowered by every kernel that puts another column into a covered
  // slot (dev_gram_touch).  nullptr until a refit entry point is first used
  double* gram;
  double* gram_c;
  long long* nnls_stats;
};

struct bc_snnls {
  bc_ctx* ctx = nullptr;
  bc_phi* phi = nullptr;
  int alg = 0;
  SnnlsDev d;
  // second buffer set for set_weights (swapped in after the rebuild kernel)
  long long* idx2 = nullptr;
  double* val2 = nullptr;
  double* cols2 = nullptr;
  double* colnorm2 = nullptr;
  // The small state arrays (st, b, bn, xw, xw_prev, v, xf, the send record) live in ONE allocation and the active
  // lists (both buffer sets) in another: the single-block step kernel starts every greedy step with cold TLBs (a 1 GB
  // sweep ran in between), and its first round of loads paid one page-table walk per separately allocated array.
  void* state_slab = nullptr;
  void* list_slab = nullptr;
  bc_pref* pref = nullptr;         // reduced-precision pre-filter of the sweep (large shards), see bc_prefilter.hip
  double* cand_send = nullptr;     // this rank's candidate record (S + 4 doubles)
  bool cand_send_owned = true;     // false once the host bound its own exchange buffers
  bc_comm* comm = nullptr;         // native RCCL exchange (bc_comm.hip): the loop all-gathers by itself
  double* cand_all_owned = nullptr;
  long long nnz_upper = 0;   // host-side upper bound on the list length
  long long iter_upper = 0;
  RescoreArgs rs;                 // argument block of the rescoring stage for the step in flight (fused finish)
  bool rs_pending = false;        // step_local ran the sweep only: step_finish must run the fused rescoring + finish
  bool exact_step = false;        // the step in flight uses the exact fp64 sweep (redo after a pre-filter overflow)
  bool pref_suspended = false;    // repeated overflows: the rest of this build call sweeps in fp64
  int consec_overflow = 0;
  bool dev_refit = false;         // bc_snnls_device_refit: an OrthoPursuit handle runs the fused loop with the device NNLS refit
  void* nnls_slab = nullptr;      // gram | gram_c | nnls_stats
  bool no_pf = false;             // BC_FINISH_NOPF / BC_FINISH_NOFUSE as the environment had them at creation: no one-round
  bool no_fuse = false;           // finish kernel / no rescoring inside it (tests and A/B measurements choose the form with them)
  int finish_form = 0;            // BC_FINISH_* of the last step_finish (bc_snnls_finish_form)
};

// the sweep's mode for this solver's algorithm: 0 GIGA (two unit vectors), 1 dot (one vector)
static inline int mode_of(const bc_snnls* h) { return h->alg == BC_ALG_GIGA ? 0 : 1; }

// the solver's slabs lay their pieces out 256-byte aligned
static inline size_t bc_up256(size_t b) { return (b + 255) & ~(size_t)255; }
