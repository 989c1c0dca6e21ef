// K5: the logistic log-likelihood of the resident rows z = y*x (model_lr.py:29, no y column) and its derivatives at one theta,
// the pieces of a full-data Laplace fit (get_laplace, util/opt.py:10-33; the Newton iteration of samplers._lr_mode_newton):
//
//   m_n = -z_n . theta
//   value = sum_n w_n ll_n        ll = -log1p(exp(m)), and -m for m >= 100               (model_lr.py:72-79)
//   grad  = sum_n w_n p_n z_n     p  = e^m / (1 + e^m), and 1 for m >= 100               (model_lr.py:98-105)
//   diag  = sum_n w_n c_n z_n^2   c  = p (1 - p), and 0 for m >= 100                     (model_lr.py:139-153)
//   H     = sum_n w_n c_n z_n z_n^T                                                      (model_lr.py:123-137)
//
// The rows pass (k_lr_rows) reads every row once (8 D bytes per row: memory-bound).  A wave owns batches of R consecutive rows,
// its lanes the columns (lane l: columns l, l + 64, ...); the dot product is a lane-partial fma chain plus the DPP butterfly of
// bc_wave_sum_all, so m is wave-uniform; the transcendental part of the R rows is one evaluation with lane l on row l % R,
// broadcast back through v_readlane.  value / grad / diag are accumulated per
// lane in row order, the four waves of a block are combined in wave order through LDS, and the per-block partials are summed
// in block order by k_lr_reduce: the association is fixed by (n_rows, grid), a call is bit-reproducible run to run.  The pass
// optionally writes the curvature weights w_n c_n to an N-vector, from which H is K4 (bc_gram.hip) in its no-y-column mode.
#include "bc_internal.h"
#include "bc_lr_terms.h"
#include "../../include/beta_cores_laplace.h"
#include <cmath>
#include <cstring>

#define BC_LR_MAX_D 1024          // 16 column slots of 64 lanes
#define BC_LR_BLOCKS_PER_CU 2     // 8 waves per CU (two per SIMD: 140-220 VGPRs), R * NC row loads in flight each
#define BC_LR_RED_PARTS 16        // k_lr_reduce: 16 runs of consecutive blocks per element, summed in run order

struct LrArgs {
  const void* z;          // [n_rows][d] of the kernel's ZT (double or float)
  const double* w;        // [n_rows] or null (all ones)
  const double* theta;    // [d]
  double* wc;             // [n_rows]: w_n c_n (the Hessian's weights), or null
  double* part;           // [blocks][1 + 2 d]: value | grad | diag
  long long n_rows;
  long long rows_per_block;   // multiple of 4 R
  int d;
};

template <int NC, int R, bool DIAG, typename ZT = double>   // R: a power of two <= 64; ZT: the rows' storage type (float: widened as read)
__global__ __launch_bounds__(256) void k_lr_rows(LrArgs a) {
  __shared__ double red[2 * NC * 64 + 1];
  const ZT* __restrict__ zrows = reinterpret_cast<const ZT*>(a.z);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int d = a.d;
  const long long start = (long long)blockIdx.x * a.rows_per_block;
  long long end = start + a.rows_per_block;
  if (end > a.n_rows) end = a.n_rows;
  double th[NC], g[NC], dg[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int col = c * 64 + lane;
    th[c] = col < d ? a.theta[col] : 0.;
    g[c] = 0.;
    dg[c] = 0.;
  }
  double val = 0.;
  // batch k of R rows goes to wave k % 4 (wave-uniform loop: every lane takes part in the butterflies)
  for (long long r0 = start + (long long)wv * R; r0 < end; r0 += 4LL * R) {
    double x[R][NC], wr[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const long long row = r0 + i;
      const bool ok = row < end;
      const ZT* zr = zrows + (size_t)(ok ? row : start) * d;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int col = c * 64 + lane;
        x[i][c] = ok && col < d ? (double)zr[col] : 0.;
      }
      wr[i] = ok ? (a.w ? a.w[row] : 1.) : 0.;     // (rows past the end: z = 0 and weight 0 -- finite terms times zero)
    }
    // m of the R rows (wave-uniform), then the transcendental part ONCE per batch: lane l evaluates row l % R, the R results
    // are read back from lanes 0 .. R-1 (an fp64 exp + log1p + divisions per row and wave cost ~1 300 cycles a row at D = 128
    // when every lane evaluated every row: 0.24 of the HBM bound)
    double mm = 0.;
#pragma unroll
    for (int i = 0; i < R; ++i) {
      double s = 0.;
#pragma unroll
      for (int c = 0; c < NC; ++c) s = fma(x[i][c], th[c], s);
      const double m = -bc_wave_sum_all(s);
      if ((lane & (R - 1)) == i) mm = m;
    }
    double lll, pl, cl;
    lr_terms(mm, lll, pl, cl);
    double wcv = 0.;
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const double ll = bc_readlane(lll, i), p = bc_readlane(pl, i), cc = bc_readlane(cl, i);
      val = fma(wr[i], ll, val);
      const double wp = wr[i] * p, wc = wr[i] * cc;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        g[c] = fma(wp, x[i][c], g[c]);
        if (DIAG) dg[c] = fma(wc * x[i][c], x[i][c], dg[c]);
      }
      if (lane == i) wcv = wc;
    }
    if (a.wc && lane < R && r0 + lane < end) a.wc[r0 + lane] = wcv;
  }
  // the four waves, in wave order: ((w0 + w1) + w2) + w3
  for (int q = 0; q < 4; ++q) {
    if (wv == q) {
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        red[c * 64 + lane] = q ? red[c * 64 + lane] + g[c] : g[c];
        if (DIAG) red[(NC + c) * 64 + lane] = q ? red[(NC + c) * 64 + lane] + dg[c] : dg[c];
      }
      if (lane == 0) red[2 * NC * 64] = q ? red[2 * NC * 64] + val : val;
    }
    __syncthreads();
  }
  double* out = a.part + (size_t)blockIdx.x * (1 + 2 * d);
  for (int e = tid; e < 1 + 2 * d; e += 256) {
    double v;
    if (e == 0) v = red[2 * NC * 64];
    else if (e <= d) v = red[e - 1];
    else v = DIAG ? red[NC * 64 + (e - 1 - d)] : 0.;
    out[e] = v;
  }
}

// out[e] = sum over blocks of part[b][e], in block order: BC_LR_RED_PARTS runs of consecutive blocks (eight loads in flight),
// the run sums added in run order.  Block = 16 elements x 16 runs.
__global__ __launch_bounds__(256) void k_lr_reduce(const double* __restrict__ part, long long blocks, int elems, double* __restrict__ out) {
  __shared__ double rs[BC_LR_RED_PARTS][16];
  const int el = threadIdx.x & 15, run = threadIdx.x >> 4;
  const int e = blockIdx.x * 16 + el;
  const long long len = (blocks + BC_LR_RED_PARTS - 1) / BC_LR_RED_PARTS;
  const long long b0 = run * len;
  long long b1 = b0 + len;
  if (b1 > blocks) b1 = blocks;
  double acc = 0.;
  if (e < elems) {
    const double* p = part + e;
    long long b = b0;
    for (; b + 8 <= b1; b += 8) {
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(b + u) * elems];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc += v[u];
    }
    for (; b < b1; ++b) acc += p[(size_t)b * elems];
  }
  rs[run][el] = acc;
  __syncthreads();
  if (run == 0 && e < elems) {
    double t = rs[0][el];
#pragma unroll
    for (int q = 1; q < BC_LR_RED_PARTS; ++q) t += rs[q][el];
    out[e] = t;
  }
}

int bc_lr_reduce_launch(bc_ctx* ctx, const double* part_dev, long long blocks, int elems, double* out_dev) {
  hipLaunchKernelGGL(k_lr_reduce, dim3((unsigned)((elems + 15) / 16)), dim3(256), 0, ctx->stream, part_dev, blocks, elems, out_dev);
  BC_HIP(hipGetLastError());
  return BC_OK;
}

template <int NC, int R>
static void launch_rows(bool diag, bool f32, dim3 grid, hipStream_t s, const LrArgs& a) {
  if (f32) {
    if (diag) hipLaunchKernelGGL((k_lr_rows<NC, R, true, float>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_lr_rows<NC, R, false, float>), grid, dim3(256), 0, s, a);
    return;
  }
  if (diag) hipLaunchKernelGGL((k_lr_rows<NC, R, true>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((k_lr_rows<NC, R, false>), grid, dim3(256), 0, s, a);
}

template <int NC, int R>
static long long rows_grid(const bc_ctx* ctx, long long n_rows, long long* rpb) {
  long long want = (long long)ctx->n_cu * BC_LR_BLOCKS_PER_CU;
  long long r = (n_rows + want - 1) / want;
  r = ((r + 4 * R - 1) / (4 * R)) * (4 * R);
  *rpb = r;
  return (n_rows + r - 1) / r;
}

extern "C" int bc_logistic_newton_pass(bc_ctx* ctx, const bc_data* data, const bc_data* w, const double* theta, double* out_value,
                                       double* out_grad, double* out_diag, double* out_hess) {
  if (!ctx || !data || !theta || !out_value || !out_grad) {
    bc_set_error("bc_logistic_newton_pass: bad argument (context, rows, theta, value and gradient are required)");
    return BC_INVALID_ARGUMENT;
  }
  if (data->ctx != ctx || (w && w->ctx != ctx)) { bc_set_error("bc_logistic_newton_pass: rows or weights belong to another context"); return BC_INVALID_ARGUMENT; }
  const int d = data->dz;
  if (d < 1 || d > BC_LR_MAX_D) { bc_set_error("bc_logistic_newton_pass: rows must have 1 .. %d columns, got %d", BC_LR_MAX_D, d); return BC_INVALID_ARGUMENT; }
  if (w && (w->dz != 1 || w->n_rows != data->n_rows)) {
    bc_set_error("bc_logistic_newton_pass: weights must be %lld x 1, got %lld x %d", (long long)data->n_rows, (long long)w->n_rows, w->dz);
    return BC_INVALID_ARGUMENT;
  }
  if (w && bc_refuse_f32(w, "bc_logistic_newton_pass (weights)")) return BC_INVALID_ARGUMENT;
  const bool f32 = data->elem == 4;
  const long long n = data->n_rows;
  const int elems = 1 + 2 * d;
  if (n == 0) {
    *out_value = 0.;
    memset(out_grad, 0, (size_t)d * sizeof(double));
    if (out_diag) memset(out_diag, 0, (size_t)d * sizeof(double));
    if (out_hess) memset(out_hess, 0, (size_t)d * d * sizeof(double));
    return BC_OK;
  }
  BC_HIP(hipSetDevice(ctx->device));
  const int nc = d <= 64 ? 1 : d <= 128 ? 2 : d <= 256 ? 4 : d <= 512 ? 8 : 16;
  long long rpb = 0, blocks = 0;
  switch (nc) {
    case 1: blocks = rows_grid<1, 8>(ctx, n, &rpb); break;
    case 2: blocks = rows_grid<2, 8>(ctx, n, &rpb); break;
    case 4: blocks = rows_grid<4, 4>(ctx, n, &rpb); break;
    case 8: blocks = rows_grid<8, 4>(ctx, n, &rpb); break;
    default: blocks = rows_grid<16, 2>(ctx, n, &rpb); break;
  }
  // scratch: theta | reduced value, grad, diag  ;  per-block partials  ;  curvature weights (Hessian only)
  int rc = bc_scratch_grow(ctx, &ctx->lap[0], (size_t)d + elems);
  if (!rc) rc = bc_scratch_grow(ctx, &ctx->lap[1], (size_t)blocks * elems);
  if (!rc && out_hess) rc = bc_scratch_grow(ctx, &ctx->lap[2], (size_t)n);
  if (rc) return rc;
  double* th_dev = ctx->lap[0].p;
  double* red_dev = th_dev + d;
  BC_HIP(hipMemcpyAsync(th_dev, theta, (size_t)d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  LrArgs a;
  a.z = data->z;
  a.w = w ? w->z : nullptr;
  a.theta = th_dev;
  a.wc = out_hess ? ctx->lap[2].p : nullptr;
  a.part = ctx->lap[1].p;
  a.n_rows = n;
  a.rows_per_block = rpb;
  a.d = d;
  rc = bc_timer_begin(ctx, 6);
  if (rc) return rc;
  const dim3 grid((unsigned)blocks);
  const bool diag = out_diag != nullptr;
  switch (nc) {
    case 1: launch_rows<1, 8>(diag, f32, grid, ctx->stream, a); break;
    case 2: launch_rows<2, 8>(diag, f32, grid, ctx->stream, a); break;
    case 4: launch_rows<4, 4>(diag, f32, grid, ctx->stream, a); break;
    case 8: launch_rows<8, 4>(diag, f32, grid, ctx->stream, a); break;
    default: launch_rows<16, 2>(diag, f32, grid, ctx->stream, a); break;
  }
  BC_HIP(hipGetLastError());
  rc = bc_lr_reduce_launch(ctx, a.part, blocks, elems, red_dev);
  if (rc) return rc;
  rc = bc_timer_end(ctx, 6);
  if (rc) return rc;
  double* hess_dev = nullptr;
  if (out_hess) {
    rc = bc_gram_no_y(ctx, data, a.wc, &hess_dev);
    if (rc) return rc;
  }
  double* host = ctx->pinned;                         // (pinned_doubles >= 1 + 2 * BC_LR_MAX_D)
  BC_HIP(hipMemcpyAsync(host, red_dev, (size_t)elems * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (out_hess) BC_HIP(hipMemcpyAsync(out_hess, hess_dev, (size_t)d * d * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  BC_HIP(hipStreamSynchronize(ctx->stream));
  *out_value = host[0];
  memcpy(out_grad, host + 1, (size_t)d * sizeof(double));
  if (out_diag) memcpy(out_diag, host + 1 + d, (size_t)d * sizeof(double));
  return BC_OK;
}
