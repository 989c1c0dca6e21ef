// The projection's internal interface: what a translation unit other than bc_project.hip needs in order to project rows with
// a plan (bc_vigrad.hip).  No kernel in here: the K1 kernels, their __device__ tables and their launch tables are
// bc_project_k1.h, which only the two units that instantiate them include.  Everything declared below is defined in
// bc_project.hip.
#pragma once
#include "bc_internal.h"

struct ProjArgs {
  const void* z;          // [n_rows][dz] of the kernel's ZT (double, or float: widened in registers, see k_project_r)
  const double* theta;    // [nt*16][dk]  zero padded            (MFMA kernel)
  const double* saux;     // [nt*16] per-sample extra (gauss: theta^T Siginv theta)
  const double* rowaux;   // [n_rows] per-row extra (gauss: x^T Siginv x) or null
  double* tiles;
  double* norms;
  double* tile_part;
  long long n_rows;
  int dz, d, dk, s, model;
  int s_total, s_off;     // RAW passes (S > 256): this launch fills samples [s_off, s_off + s) of s_total, un-centred
  long long ngroups;      // k_project_r: 32-row groups of this launch
  int part_init;          // k_project_r: start the per-wave column partials from tile_part instead of 0 (a later chunk of
                          // a chunked projection, bc_project_from_host: the same sums in the same order as ONE launch)
  double c[8];            // model constants, see model_constants()
  // constant rows whose model value the HOST evaluated (bc_ctx_set_constant_row_values: hosts whose NumPy does not take the
  // SVML exp bc_np_exp.h restates): sorted keys (LINREG_BETA: the row's y), the values, how many; 0: none
  const double* ck;
  const double* cv;
  int nck;
#ifdef BC_K1_STAMPS       // diagnostic build: s_memtime of wave 0 at phase boundaries, 32 slots per tile
  unsigned long long* stamps;
#endif
};

enum { PROJ_FULL = 0, PROJ_RAW = 1, PROJ_COLSUM = 2 };

// ---- a projection in two steps: the plan (model constants, Theta zero-padded and uploaded: once per Theta) and the
// launches that use it (one per set of rows: bc_vi_gradient projects the data rows and the coreset rows with one plan)
struct ProjPlan {
  ProjArgs a;             // constants, theta, saux, d, dk, s, model filled in; the per-launch fields are set by plan_launch
  int model = 0, s = 0, d = 0, ntsel = 0;
  bool raw = false;
  const double* siginv_dev = nullptr;      // Gaussian models: Siginv [d][d] on the device
};

int bc_proj_project_check(bc_ctx* ctx, const bc_data* data, int model, const double* theta, int32_t s, const double* params,
                          int32_t n_params, const char* who);
int bc_proj_plan_stage(bc_ctx* ctx, int model, const double* theta, int32_t s, const double* params, int32_t n_params, int dz,
                       bool raw, ProjPlan* pl, int n_extra = 0, const double* const* extra_src = nullptr,
                       const size_t* extra_n = nullptr, double** extra_dev = nullptr);
int bc_proj_plan_launch(bc_ctx* ctx, const ProjPlan& pl, const bc_data* data, bc_phi* phi, int mode, int32_t s_total, int32_t s_off,
                        bc_scratch* rowaux);
int bc_proj_plan_constants(bc_ctx* ctx, int model, const double* params, int32_t n_params, int d, ProjArgs* a, const double** siginv);
void bc_proj_plan_bind(ProjPlan* pl, int model, int32_t s, int d, int dk, int NTsel, int NRsel, bool raw, const double* theta_dev,
                       const double* siginv_dev);
void bc_proj_theta_layout(int s, int d, bool raw, int* NTsel_out, int* NRsel_out, int* dk_out);
int bc_proj_model_constants(int model, const double* p, int np, int d, double* c, const double** siginv);
bool bc_proj_model_has_y(int model);
bool bc_proj_model_store_only(int model);
int bc_proj_colsum_phi_for(bc_ctx* ctx, int64_t n_rows, int32_t s, bc_phi** out);      // the context's stats-only Phi

// bc_proj_plan_launch takes the stream and the kernel timer from the context.  While one of these lives, the context's
// launches go to `launch_on` (null: where they went before) and are no samples of the kernel timer.
struct bc_proj_scope {
  bc_ctx* const ctx;
  const hipStream_t stream;
  const int timing;
  bc_proj_scope(bc_ctx* c, hipStream_t launch_on) : ctx(c), stream(c->stream), timing(c->timing) {
    if (launch_on) c->stream = launch_on;
    c->timing = 0;
  }
  ~bc_proj_scope() { ctx->stream = stream; ctx->timing = timing; }
  bc_proj_scope(const bc_proj_scope&) = delete;
};
