// Internal definitions shared by the HIP translation units of libbeta_cores.
// gfx950 (MI355X, CDNA4) only: wave = 64 lanes, fp64 throughout.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <functional>
#include <vector>
#include "../../include/beta_cores.h"
#include "bc_layout.h"
#include "bc_run.h"

#define BC_WAVE 64
#define BC_TILE BC_LAY_TILE           // rows per Phi tile: bc_layout.h's value, which the public header states to callers
static_assert(BC_TILE_ROWS == BC_LAY_TILE, "include/beta_cores.h documents the tile's rows");
#define BC_REC_HDR 4                  // candidate record header doubles: score, gidx(bits), norm, valid

void bc_set_error(const char* fmt, ...);
int bc_hip_fail(hipError_t e, const char* what, const char* file, int line);

#define BC_HIP(call)                                                        \
  do {                                                                      \
    hipError_t _e = (call);                                                 \
    if (_e != hipSuccess) return bc_hip_fail(_e, #call, __FILE__, __LINE__); \
  } while (0)
// a refusal before anything is touched: the message (printf style), then BC_INVALID_ARGUMENT
#define BC_REFUSE(...) do { bc_set_error(__VA_ARGS__); return BC_INVALID_ARGUMENT; } while (0)

struct bc_timer {
  std::vector<hipEvent_t> start, stop;
  size_t used = 0;
  double acc_ms = 0.0;     // folded-in time of already collected events
  int64_t launches = 0;    // timed launches
  int64_t seq = 0;         // all launches seen (timed or not)
  bool armed = false;      // the launch in progress is being timed
};

// grow-only device buffer owned by a context (freed in bc_ctx_destroy): scratch of calls that are made thousands of
// times on coreset-sized inputs, where a hipMalloc / hipFree pair per call would dominate
struct bc_scratch {
  double* p = nullptr;
  size_t cap = 0;                // doubles
};

// ---- what the chunked device runs share (bc_viopt.hip, bc_hmc.hip, bc_hmc_small.hip, bc_psvi_many.hip; the functions are in bc_core.hip)
// the pinned twin of bc_scratch: grow-only host memory, contents not kept when it grows
struct bc_pinned {
  double* p = nullptr;
  size_t cap = 0;                // doubles
};
// a chunk's staging pair: filled on the host in `pin`, sent to `dev` in one transfer.  A half that failed to grow is left
// with capacity 0 (and no memory), so the next bc_stage_reserve grows it again.
struct bc_stage {
  bc_scratch dev;
  bc_pinned pin;
};
// the device time of a run's chunks: two events around each chunk's launches, folded into `ms` once the chunk has been waited for
struct bc_run_clock {
  hipEvent_t ev[2] = {nullptr, nullptr};
  double ms = 0.;
  int create();                  // the events, where they do not exist yet
  int start(hipStream_t s);
  int stop(hipStream_t s);
  void collect();                // after the stream has been synchronised; an elapsed time that cannot be read is left out
  void free();
};
// a chunked run as its unit's state embeds it: the protocol's state (bc_run.h) and the clock of its chunks
struct bc_run : bc_run_state {
  bc_run_clock clock;
};
// the tail of every _begin: a fresh run of `total`, its clock at 0
inline void bc_run_opened(bc_run* r, int64_t total) { bc_run_open(r, total); r->clock.ms = 0.; }
// _chunk_end, after bc_run_pending: the chunk is no longer pending; sets the device, waits for the stream, collects the clock
int bc_run_wait_chunk(struct bc_ctx* ctx, bc_run* r);
// _end: refuses where no run is open; otherwise closes it (bc_run_close) and waits for a chunk that was abandoned
int bc_run_end(struct bc_ctx* ctx, bc_run* r, const bc_run_kind& kd, bool* was_pending);
// the body of every *_device_ms (`clock`: null where the unit has no state on the context yet)
int bc_device_ms(const char* who, const struct bc_ctx* ctx, const bc_run_clock* clock, double* out_ms);

// phases of bc_vi_gradient, timed with HIP events when the context's timing is on (bc_ctx_phase_times)
#define BC_VI_PHASES 5           // upload (Theta, coreset rows, w) | K1 of the coreset rows | K1 over the data rows (store-free) |
                                 // column-sum reduction (+ rank-order sum over ranks) | M x S algebra + download
// the three kinds of pending gradient: bc_vi_gradient (grad | resid), bc_vi_beta_gradient (grad | resid | beta_dots),
// bc_psvi_gradient (grad_w | resid | grad_p [m][dz])
#define BC_VI_KIND_PLAIN 0
#define BC_VI_KIND_BETA 1
#define BC_VI_KIND_PSVI 2
struct bc_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int timing = 0;                // 0 = off, n >= 1: every n-th launch of each kernel class is timed
  unsigned timing_mask = 0x7;    // which classes (bit = class): the step stages 3-5 only on request (bc_ctx_timing_classes)
  bc_timer timers[7];            // 0 K3 sweep | 1 K1 projection | 2 K4 Gram + reduce | 3 rescoring / local winner |
                                 // 4 candidate all-gather (RCCL) | 5 step finish | 6 logistic rows pass + reduce (K5), k_lr_score
  int n_cu = 256;
  int max_lds = 64 * 1024;       // hipDeviceAttributeMaxSharedMemoryPerBlock (160 KiB on gfx950)
  double* pinned = nullptr;      // small pinned staging area (host)
  size_t pinned_doubles = 0;
  // K1 staging (bc_project.hip): zero-padded Theta, per-sample / per-row extras, Siginv; a pinned host mirror
  bc_scratch proj_theta, proj_rowaux, proj_rowaux2;      // proj_theta: Theta | saux | Siginv | extras, one transfer
  double* proj_pinned = nullptr;
  size_t proj_pinned_cap = 0;
  bc_scratch gradx;              // bc_project_grad_x
  bc_scratch gram[5];            // K4: partial, partial_y, out, out_y, w
  bc_scratch lap[3];             // K5 (bc_laplace.hip): theta | reduced terms, per-block partials, curvature weights
  bc_phi* colsum_phi = nullptr;  // store-free K1: a Phi with the per-tile column partials but no tiles / norms
  struct bc_vigrad* vigrad = nullptr;  // the fused VI gradients (bc_vigrad.hip): cached Phis, result buffers, side stream, what is pending
  struct bc_uploader* upl = nullptr;   // pipelined host -> HBM uploads (bc_upload.hip): copy streams, pinned staging, events
  // host-evaluated constants of constant rows (bc_ctx_set_constant_row_values): sorted keys, then values, on the device
  bc_scratch const_rows;
  int64_t n_const_rows = 0;
  int const_model = -1;
  double const_params[4] = {0., 0., 0., 0.};
  int const_n_params = 0;
  // bc_data_take_rows (bc_take.hip): the indices on the device; two pinned staging areas used in turn, each with the event
  // of the last copy out of it (a call waits for the copy of the call before the previous one, not for the previous one)
  bc_scratch take_idx;
  long long* take_pinned[2] = {nullptr, nullptr};
  size_t take_pinned_cap[2] = {0, 0};      // indices
  hipEvent_t take_ev[2] = {nullptr, nullptr};
  int take_turn = 0;
  struct bc_viopt* viopt = nullptr;    // bc_vi_optimize (bc_viopt.hip): the buffers and the state of the run in progress
  struct bc_hmc* hmc = nullptr;        // bc_hmc_* (bc_hmc.hip): the buffers and the state of the HMC run in progress
  struct bc_hmc_small* hmc_small = nullptr;   // bc_hmc_small_* (bc_hmc_small.hip): the same for the batched small-problem run
  struct bc_lap_small* laplace_small = nullptr;   // bc_laplace_small (bc_laplace_small.hip): the buffers of the batched Laplace fit
  struct bc_psvi_many* psvi_many = nullptr;   // bc_psvi_many_* (bc_psvi_many.hip): the buffers and the state of the batched BatchPSVI run
  bc_scratch score;              // bc_lr_score (bc_score.hip): theta | ll | correct (ints)
  bc_scratch diag;               // bc_chain_summary (bc_diag.hip): the uploaded samples | the retained layout | the run's work space
  bc_scratch predict;            // bc_linreg_predict (bc_predict.hip): mu | factor | packed factor | noise | scale | partials | ll | sse | mean | var
};

// bc_upload.hip: rows of a host array -> dst_dev through pinned staging and several copy threads; the hook (optional) is
// called per chunk in row order with the event that marks the chunk's arrival (nullptr: it has already landed)
typedef std::function<int(int64_t chunk, int64_t row0, int64_t rows, hipEvent_t landed)> bc_chunk_hook;
// row_bytes: the size of one row (dz elements of the rows' storage type: the uploader moves bytes)
int bc_upload_rows(bc_ctx* ctx, const void* src, void* dst_dev, int64_t n_rows, size_t row_bytes, int64_t chunk_rows,
                   const bc_chunk_hook* on_chunk);
int64_t bc_upload_default_chunk_rows(int64_t n_rows, size_t row_bytes);
void bc_uploader_free(bc_ctx* ctx);
void bc_take_free(bc_ctx* ctx);      // bc_take.hip: the two pinned index staging areas and their events
void bc_vigrad_free(bc_ctx* ctx);    // bc_vigrad.hip: joins the gradient's side stream, then frees what it kept
bool bc_vigrad_pending(const bc_ctx* ctx, int* kind);   // a fused gradient is pending (*kind, optional: its BC_VI_KIND_*)
void bc_viopt_free(bc_ctx* ctx);     // bc_viopt.hip
bool bc_viopt_active(const bc_ctx* ctx);   // the context holds an open bc_vi_optimize run
void bc_hmc_free(bc_ctx* ctx);       // bc_hmc.hip
bool bc_hmc_active(const bc_ctx* ctx);     // the context holds an open bc_hmc run
void bc_hmc_small_free(bc_ctx* ctx); // bc_hmc_small.hip
bool bc_hmc_small_active(const bc_ctx* ctx);   // the context holds an open bc_hmc_small run
void bc_laplace_small_free(bc_ctx* ctx);   // bc_laplace_small.hip (the call is synchronous: it never holds the context)
void bc_psvi_many_free(bc_ctx* ctx); // bc_psvi_many.hip
bool bc_psvi_many_active(const bc_ctx* ctx);   // the context holds an open bc_psvi_many run
// bc_score.hip: the checks of the held-out pair (d_run > 0: the columns the rows must have), and k_lr_score over t thetas that are
// already on the device; enqueued only
int bc_score_check(const bc_ctx* ctx, const struct bc_data* zt, const struct bc_data* yt, int64_t t, int32_t d_run, const char* who);
int bc_score_launch(bc_ctx* ctx, const struct bc_data* zt, const struct bc_data* yt, const double* theta_dev, int64_t t, int* correct_dev,
                    double* ll_dev);
// What may hold a context, and the one place that says who is refused while it does (the table is beside the function in
// bc_core.hip).  `holders`: the BC_HOLD_* that refuse the caller `who`; `own`: the caller's own kind, if it is a holder.
#define BC_HOLD_GRADIENT 1u          // a fused gradient is pending (bc_vi_gradient_begin and its kin)
#define BC_HOLD_VIOPT 2u             // an open bc_vi_optimize run
#define BC_HOLD_HMC 4u               // an open bc_hmc run
#define BC_HOLD_HMC_SMALL 8u         // an open bc_hmc_small run
#define BC_HOLD_PSVI_MANY 16u        // an open bc_psvi_many run
#define BC_HOLD_ALL 31u
int bc_ctx_refuse_busy(const bc_ctx* ctx, const char* who, unsigned holders, unsigned own = 0);
const char* bc_vi_kind_name(int kind);     // the entry point's name of a BC_VI_KIND_* (bc_vigrad.hip)
// the tail of the one-call drivers: closes a run that failed with `end`, keeps the message of what failed, and returns rc
int bc_close_failed_run(int rc, const std::function<int()>& end);
// bc_take.hip: dst[j, :] = src[idx_dev[j], :] for indices that are already on the device and already checked; enqueued only
int bc_take_rows_dev(bc_ctx* ctx, const bc_data* src, const long long* idx_dev, int64_t m, void* dst_z);
// bc_vigrad.hip: one gradient's projections and algebra for a Theta that is already on the device (bc_viopt.hip)
struct bc_vi_plan;
int bc_vi_plan_layout(int model, int32_t s, int dz, int* d, int* dk, int* nrsel, int* ntsel);
int bc_vi_plan_create(bc_ctx* ctx, int model, const double* params, int32_t n_params, int dz, int32_t s, const double* theta_dev,
                      const double* siginv_dev, bc_vi_plan** out);
void bc_vi_plan_destroy(bc_vi_plan* p);
int bc_vi_plan_step(bc_ctx* ctx, const bc_vi_plan* p, const struct bc_data* core, const struct bc_data* rows, const double* w_dev,
                    double scale, double* resid_dev, double* grad_dev);

// bc_psvi.hip: k_psvi_point_grad behind k_vi_gradient (bc_psvi_gradient_begin); everything is already on the device
int bc_psvi_kind(int model);      // BC_PSVI_* of a model with an x-gradient, -1 otherwise
int bc_psvi_max_dz(void);
int bc_psvi_point_grad_launch(bc_ctx* ctx, int model, const double* pts_dev, const double* w_dev, int64_t m, int dz, int d,
                              int32_t s, const double* theta_dev, int dk, const double* siginv_dev, double sigsq,
                              const double* resid_dev, double* out_dev);

int bc_scratch_grow(bc_ctx* ctx, bc_scratch* s, size_t doubles);   // contents are NOT kept when it grows
int bc_pinned_grow(bc_ctx* ctx, bc_pinned* s, size_t doubles);     // the same for pinned host memory
int bc_stage_reserve(bc_ctx* ctx, bc_stage* st, size_t doubles);   // both halves hold `doubles`; contents are NOT kept
void bc_scratch_free(bc_scratch* s);
void bc_pinned_free(bc_pinned* s);
void bc_stage_free(bc_stage* st);
// A step chunk's draws into `st`, one transfer: n_e normals ([k][S][D]), then, where n_sub > 0, the int64 row numbers
// [k][n_sub] of the steps first_step .. first_step + k - 1, each checked against [0, n_rows).  An index out of range is
// BC_INVALID_ARGUMENT with nothing enqueued.  *e_dev / *idx_dev: where they lie on the device.
int bc_stage_step_chunk(bc_ctx* ctx, bc_stage* st, const char* who, const double* normals, size_t n_e, const int64_t* sub_idx, size_t k,
                        size_t n_sub, int64_t first_step, int64_t n_rows, const double** e_dev, const long long** idx_dev);

int bc_timer_begin(bc_ctx* ctx, int which);
int bc_gram_no_y(bc_ctx* ctx, const bc_data* data, const double* w_dev, double** out_dev);   // bc_gram.hip
int bc_timer_end(bc_ctx* ctx, int which);
// bc_laplace.hip: out[e] = sum over blocks of part[b][e] in block order (k_lr_reduce), enqueued on the context's stream
int bc_lr_reduce_launch(bc_ctx* ctx, const double* part_dev, long long blocks, int elems, double* out_dev);

struct bc_data {
  bc_ctx* ctx = nullptr;
  int64_t n_rows = 0;
  int32_t dz = 0;
  double* z = nullptr;           // row-major n_rows x dz; elem == 4: the allocation holds FLOATS (read it through bc_rows<float>)
  bool owned = true;
  int64_t cap_rows = 0;          // allocation size in rows (owned buffers)
  int elem = 8;                  // bytes per stored element: 8 = float64, 4 = float32 (include/beta_cores_f32.h).  float32 rows
                                 // are widened in registers by the kernels that read them; nothing else in the library is float32
};

// the rows of a handle as their storage type (the caller has dispatched on data->elem)
template <typename T>
static inline const T* bc_rows(const bc_data* d) { return reinterpret_cast<const T*>(d->z); }
// entry points that only serve float64 rows: BC_INVALID_ARGUMENT and a message that names the dtype
int bc_refuse_f32(const bc_data* d, const char* who);

struct bc_phi {
  bc_ctx* ctx = nullptr;
  int64_t n_rows = 0;
  int32_t s = 0;
  int64_t row_offset = 0;
  int64_t ntiles = 0;
  int64_t cap_tiles = 0;         // allocation size in tiles (n_rows may change below it)
  void* slab = nullptr;          // the one device allocation all pointers below point into
  double* stage = nullptr;       // row-major staging for bc_phi_to_host (lazy)
  size_t stage_cap = 0;
  double* tiles = nullptr;       // [ntiles][s][128]
  double* norms = nullptr;       // [ntiles*128]
  double* colsum = nullptr;      // [s]   (valid when stats_valid)
  double* tile_part = nullptr;   // [ntiles][s] per-tile column partial sums (scratch)
  int64_t part_rows = 0;         // rows of tile_part the last producer filled: ntiles, or one per wave (k_project_r)
  double* stats = nullptr;       // device: {norm_sum, zero_rows}
  double* part2 = nullptr;       // [stat_blocks][s] second-level column partials
  double* nstat = nullptr;       // [stat_blocks][2]
  int stat_blocks = 1;
  bool stats_valid = false;
  double norm_sum = 0.0;
  int64_t zero_rows = 0;
  // scratch for standalone argmax sweeps
  double* blk_val = nullptr;
  long long* blk_idx = nullptr;
  int sweep_blocks = 0;
  double* vbuf = nullptr;        // [2*s]
  double* rec = nullptr;         // one candidate record
  unsigned* sweep_counter = nullptr;   // arrival counter of the sweep's last-block reduction (kept at 0 between launches)
};

int bc_phi_alloc(bc_ctx* ctx, int64_t n_rows, int32_t s, int64_t row_offset, bc_phi** out, int64_t cap_rows = 0,
                 bool stats_only = false);   // stats_only: no tiles, no norms (store-free K1)
int bc_phi_set_rows(bc_phi* phi, int64_t n_rows);   // 0 if n_rows fits the capacity (state updated), 1 otherwise
int bc_phi_finish_stats(bc_phi* phi);   // tile_part -> colsum, norm stats (device), then host copy
int bc_phi_reduce_colsum(bc_phi* phi);  // tile_part -> colsum on the device only: no norm statistics, no host copy, no sync
int bc_sweep_grid(const bc_phi* phi);
// bc_sweep.hip: the exact fp64 K3 sweep with v_dev, enqueued only (rec_dev == nullptr: no record, the caller reduces
// blk_val / blk_idx itself)
int bc_launch_sweep(bc_phi* p, int mode, const double* v_dev, double post_div, const int* skip_flag, double* rec_dev);

// bc_comm.hip, for the other units (a communicator's C ABI is include/beta_cores.h): enqueued on the context's stream, no
// host synchronisation; *result_dev of the rank-order sum stays valid until the next sum through the communicator
bc_ctx* bc_comm_ctx(const bc_comm* c);
int bc_comm_all_gather_dev(bc_comm* c, const double* send_dev, double* recv_dev, size_t count);
int bc_comm_sum_dev(bc_comm* c, const double* in_dev, int64_t count, const double** result_dev);

// ------------------------------------------------------------------ device helpers
#if defined(__HIPCC__)

__device__ __forceinline__ bool bc_better(double av, long long ai, double bv, long long bi) {
  // np.argmax semantics: NaN beats everything, first occurrence wins ties.
  const bool an = av != av, bn = bv != bv;
  if (an | bn) {
    if (an & bn) return ai < bi;
    return an;
  }
  if (av > bv) return true;
  if (av < bv) return false;
  return ai < bi;
}

__device__ __forceinline__ long long bc_shfl_down_ll(long long v, int d) {
  int lo = (int)(v & 0xffffffffLL), hi = (int)(v >> 32);
  lo = __shfl_down(lo, d, BC_WAVE);
  hi = __shfl_down(hi, d, BC_WAVE);
  return ((long long)hi << 32) | (unsigned int)lo;
}

__device__ __forceinline__ void bc_wave_argmax(double& v, long long& i) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    double ov = __shfl_down(v, d, BC_WAVE);
    long long oi = bc_shfl_down_ll(i, d);
    if (bc_better(ov, oi, v, i)) { v = ov; i = oi; }
  }
}

// Wave-wide sum of a double, the total in EVERY lane (all 64 lanes must be active).  Inside a 16-lane row the
// partners come through DPP row rotations (v_mov_b32_dpp: a few cycles each) -- a rotation butterfly, so all lanes of
// a row hold bit-identical sums -- and the four row sums are combined from SGPRs (v_readlane) in a fixed order.  The
// __shfl_down tree this replaces moved each step through ds_bpermute: ~1.5k cycles per reduction, and the
// single-block step kernels do a dozen of them back to back (8 of the 20 us of a greedy step's tail).
template <int CTRL>
__device__ __forceinline__ double bc_dpp_mov(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, false);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double bc_readlane(double v, int src) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), src), hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
  return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double bc_wave_sum_all(double v) {
  v += bc_dpp_mov<0x128>(v);   // row_ror:8
  v += bc_dpp_mov<0x124>(v);   // row_ror:4
  v += bc_dpp_mov<0x122>(v);   // row_ror:2
  v += bc_dpp_mov<0x121>(v);   // row_ror:1
  return (bc_readlane(v, 0) + bc_readlane(v, 16)) + (bc_readlane(v, 32) + bc_readlane(v, 48));
}

__device__ __forceinline__ double bc_wave_sum(double v) { return bc_wave_sum_all(v); }

// wave-wide fmax of a double, the maximum in every lane (all 64 lanes active): the same rotation butterfly
__device__ __forceinline__ double bc_wave_max_all(double v) {
  v = fmax(v, bc_dpp_mov<0x128>(v));   // row_ror:8
  v = fmax(v, bc_dpp_mov<0x124>(v));   // row_ror:4
  v = fmax(v, bc_dpp_mov<0x122>(v));   // row_ror:2
  v = fmax(v, bc_dpp_mov<0x121>(v));   // row_ror:1
  return fmax(fmax(bc_readlane(v, 0), bc_readlane(v, 16)), fmax(bc_readlane(v, 32), bc_readlane(v, 48)));
}

// Wave-wide fmaxf, the maximum in every lane (all 64 lanes active): the same rotation butterfly on one register.
template <int CTRL>
__device__ __forceinline__ float bc_dpp_mov_f32(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}

__device__ __forceinline__ float bc_wave_max_f32_all(float v) {
  v = fmaxf(v, bc_dpp_mov_f32<0x128>(v));   // row_ror:8
  v = fmaxf(v, bc_dpp_mov_f32<0x124>(v));   // row_ror:4
  v = fmaxf(v, bc_dpp_mov_f32<0x122>(v));   // row_ror:2
  v = fmaxf(v, bc_dpp_mov_f32<0x121>(v));   // row_ror:1
  const int b = __builtin_bit_cast(int, v);
  const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0)), r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16));
  const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32)), r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48));
  return fmaxf(fmaxf(r0, r1), fmaxf(r2, r3));
}

// block-wide sum, result broadcast to every thread; red must hold >= 17 doubles
__device__ __forceinline__ double bc_block_sum(double v, double* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  v = bc_wave_sum(v);
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < nw; ++w) t += red[w];
    red[16] = t;
  }
  __syncthreads();
  return red[16];
}

// block-wide sum of N values at once (one barrier pair for all of them); red must hold >= 17*N doubles
template <int N>
__device__ __forceinline__ void bc_block_sum_n(double (&v)[N], double* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = bc_wave_sum(v[i]);
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) red[i * 17 + wave] = v[i];
  }
  __syncthreads();
  if (threadIdx.x < N) {
    double t = 0.0;
    for (int w = 0; w < nw; ++w) t += red[threadIdx.x * 17 + w];
    red[threadIdx.x * 17 + 16] = t;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = red[i * 17 + 16];
}

#include "bc_np_sum.h"   // bc_np_sum_const_*: NumPy's pairwise sum of n equal numbers (the mean of a constant row)

// element (row r, sample k) of a tiled Phi
__device__ __forceinline__ size_t bc_tile_off(long long r, int k, int s) {
  return (size_t)(r >> 7) * (size_t)s * BC_TILE + (size_t)k * BC_TILE + (size_t)(r & (BC_TILE - 1));
}

#endif  // __HIPCC__
