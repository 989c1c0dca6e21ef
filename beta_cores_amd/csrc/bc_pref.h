// The pre-filter's internal interface: what a translation unit other than bc_prefilter.hip (the solver: bc_snnls.hip and
// bc_snnls_diag.hip, through bc_snnls_state.h) needs in order to own one and sweep with it.  No kernel in here.  Everything declared below is defined in bc_prefilter.hip, which
// includes this header itself; the control block the kernels and the host share is bc_pref_ctrl.h, and no other unit reads it.
#pragma once
#include "bc_rescore_dev.h"

#define BC_PREF_DEFAULT_PREC 8      // storage precision of the mirror where the caller names none
#define BC_PREF_SPILL_CAP 4096      // pairs the two-level form's spill list holds

struct bc_pref;
// prec: 32, 16, 8, or 4 = the int8 mirror behind a 4-bit first level (the two-level form, where the shape allows it)
int bc_pref_create(bc_phi* phi, int prec, bc_pref** out);
void bc_pref_destroy(bc_pref* p);
void bc_pref_set_cap(bc_pref* p, int cap);
int bc_pref_precision(const bc_pref* p);
int bc_pref_sp4(const bc_pref* p);
int bc_pref_sp8(const bc_pref* p);
int bc_pref_bb(const bc_pref* p);
int bc_pref_two_level(const bc_pref* p);
int bc_pref_two_level_active(const bc_pref* p);
// the owner's digit records of its sweep vector (bc_i8_quant.h, bc_i4_quant.h), kept current by its step kernels
void bc_pref_set_qv(bc_pref* p, const int* qv_dev);
void bc_pref_set_qv4(bc_pref* p, const int* qv4_dev);
int bc_pref_adapt(bc_pref* p);

// pass A alone (fills the argument block of the rescoring stage), and passes A, B, C with the record left in rec_dev
int bc_pref_launch_sweep(bc_pref* p, int mode, const double* v_dev, const double* v_norm_dev, double post_div,
                         const int* skip_flag, double* rec_dev, RescoreArgs* r_out);
int bc_pref_launch(bc_pref* p, int mode, const double* v_dev, const double* v_norm_dev, double post_div,
                   const int* skip_flag, double* rec_dev);

// the counters of the control block, read in one copy on the pre-filter's stream and one synchronisation
struct bc_pref_counters {
  long long overflows;       // rescorings that overflowed (each one a step redone with the exact sweep)
  long long sweeps;          // rescorings that ran
  long long rescored;        // rows they rescored
  long long l1_passed;       // two-level form: rows the first level passed on (the second re-bounds every one of them)
  long long l1_seq;          // two-level sweeps launched (the HOST's count: includes sweeps the device skipped)
};
int bc_pref_read_counters(const bc_pref* p, bc_pref_counters* out);

// diagnostic seam (include/beta_cores_prefdiag.h): test aids, nothing here is called by the product; the one caller is
// bc_snnls_diag.hip, which holds the entry points
void bc_pref_diag_info(const bc_pref* p, bool qv_set, int64_t* out);
int bc_pref_diag_buffer(const bc_pref* p, const char* which, const void** dev, size_t* bytes);
size_t bc_pref_diag_save_bytes(void);
int bc_pref_diag_sweep(bc_pref* p, int mode, const double* v_dev, const double* v_norm_dev, const int* qv, const int* qv4,
                       double post_div, float2* dump1, float2* dump2, float* theta0, void* save_dev, int* form_run);
