// bc_take.hip -- bc_data_take_rows (include/beta_cores_take.h): m of the resident rows, by index, as a bc_data of their own.
//
// k_take_rows is a streaming gather: out[j, :] = src[idx[j], :], words copied as they are.  It moves rows as W-byte words
// (W = 16, 8 or 4: what the row pitch and both base addresses allow, bc_take_width.h) through one of two lane mappings:
//   * rows of at least one wave-instruction (>= 256 bytes): a wave per row, BC_TAKE_ROWS rows at a time -- the loads of all
//     of them are issued before the first store, each a contiguous wave-wide access of one source row, each store one of a
//     destination row.  The row numbers are wave-uniform (scalar loads of idx).
//   * shorter rows (the Gaussian model's 2-3 columns): consecutive lanes take consecutive words of the OUTPUT, crossing row
//     ends, BC_TAKE_ROWS words per lane in flight, so no lane idles on a 16-byte row.  A block works on tiles of 1 024
//     words; the 64-bit division that finds a tile's first row is done once per tile, the per-word ones are 32-bit.
// The grid is sized from the CU count (4 blocks of 4 waves per CU) and strides over the work.  No LDS, no atomics.
#include "bc_internal.h"
#include "bc_take_width.h"
#include "../../include/beta_cores_take.h"

#define BC_TAKE_ROWS 4             // rows (long form) / words per lane (flat form) whose loads are in flight before a store
#define BC_TAKE_BLOCK 256
#define BC_TAKE_BLOCKS_PER_CU 4    // 16 waves per CU
#define BC_TAKE_TILE (BC_TAKE_BLOCK * BC_TAKE_ROWS)      // flat form: words per block and iteration

// R whole rows j0 .. j0+R-1 by one wave: every load of a 64-word column chunk is issued before the chunk's first store
template <typename W, int R>
__device__ __forceinline__ void bc_take_group(const W* __restrict__ src, const long long* __restrict__ idx, long long j0,
                                              long long wpr, int lane, W* __restrict__ dst) {
  const W* s[R];
#pragma unroll
  for (int r = 0; r < R; ++r) s[r] = src + (size_t)idx[j0 + r] * (size_t)wpr;
  W* d = dst + (size_t)j0 * (size_t)wpr;
  for (long long c = lane; c < wpr; c += BC_WAVE) {
    W v[R];
#pragma unroll
    for (int r = 0; r < R; ++r) v[r] = s[r][c];
#pragma unroll
    for (int r = 0; r < R; ++r) d[(size_t)r * (size_t)wpr + (size_t)c] = v[r];
  }
}

// One tile of BC_TAKE_TILE consecutive OUTPUT words by one block (rows shorter than a wave-instruction): lane after lane
// takes word after word, across row ends.  FULL: the whole tile exists, so all loads are issued before the first store.
template <typename W, bool FULL>
__device__ __forceinline__ void bc_take_tile(const W* __restrict__ src, const long long* __restrict__ idx, long long t,
                                             long long total, long long wpr, W* __restrict__ dst) {
  const long long w0 = t * BC_TAKE_TILE;
  const long long row0 = w0 / wpr;                             // (block-uniform: the one 64-bit division of the tile)
  const unsigned w32 = (unsigned)wpr;                          // < 64 words per row in this form
  const unsigned rem0 = (unsigned)(w0 - row0 * wpr);
  if constexpr (FULL) {
    W v[BC_TAKE_ROWS];
#pragma unroll
    for (int u = 0; u < BC_TAKE_ROWS; ++u) {
      const unsigned loc = rem0 + (unsigned)(u * BC_TAKE_BLOCK) + threadIdx.x;
      const unsigned jr = loc / w32, col = loc - jr * w32;
      v[u] = src[(size_t)idx[row0 + jr] * (size_t)wpr + col];
    }
#pragma unroll
    for (int u = 0; u < BC_TAKE_ROWS; ++u) dst[w0 + (unsigned)(u * BC_TAKE_BLOCK) + threadIdx.x] = v[u];
  } else {
    for (unsigned off = threadIdx.x; w0 + off < total && off < BC_TAKE_TILE; off += BC_TAKE_BLOCK) {
      const unsigned loc = rem0 + off;
      const unsigned jr = loc / w32, col = loc - jr * w32;
      dst[w0 + off] = src[(size_t)idx[row0 + jr] * (size_t)wpr + col];
    }
  }
}

template <typename W, bool FLAT>
__global__ __launch_bounds__(BC_TAKE_BLOCK) void k_take_rows(const W* __restrict__ src, const long long* __restrict__ idx,
                                                             long long m, long long wpr, W* __restrict__ dst) {
  if constexpr (!FLAT) {
    const int lane = threadIdx.x & (BC_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (BC_TAKE_BLOCK / BC_WAVE) + (threadIdx.x >> 6)));
    const long long step = (long long)gridDim.x * (BC_TAKE_BLOCK / BC_WAVE) * BC_TAKE_ROWS;
    for (long long j0 = (long long)wave * BC_TAKE_ROWS; j0 < m; j0 += step) {
      if (j0 + BC_TAKE_ROWS <= m) {
        bc_take_group<W, BC_TAKE_ROWS>(src, idx, j0, wpr, lane, dst);
      } else {                                                // the last, partial group: row by row
        for (long long j = j0; j < m; ++j) bc_take_group<W, 1>(src, idx, j, wpr, lane, dst);
      }
    }
  } else {
    const long long total = m * wpr;
    const long long ntiles = (total + BC_TAKE_TILE - 1) / BC_TAKE_TILE;
    for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
      if ((t + 1) * BC_TAKE_TILE <= total) bc_take_tile<W, true>(src, idx, t, total, wpr, dst);
      else bc_take_tile<W, false>(src, idx, t, total, wpr, dst);      // the last, partial tile
    }
  }
}

template <typename W>
static hipError_t launch_take(bc_ctx* ctx, const void* src, const long long* idx, int64_t m, int64_t wpr, bool flat, void* dst) {
  // blocks that have work: tiles of words (flat), groups of BC_TAKE_ROWS rows per wave (long rows)
  const long long per_block = flat ? (long long)BC_TAKE_TILE : (long long)(BC_TAKE_BLOCK / BC_WAVE) * BC_TAKE_ROWS;
  const long long work = flat ? (long long)m * wpr : (long long)m;
  long long blocks = (work + per_block - 1) / per_block;
  const long long cap = (long long)ctx->n_cu * BC_TAKE_BLOCKS_PER_CU;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  if (flat)
    hipLaunchKernelGGL((k_take_rows<W, true>), dim3((unsigned)blocks), dim3(BC_TAKE_BLOCK), 0, ctx->stream, (const W*)src, idx,
                       (long long)m, (long long)wpr, (W*)dst);
  else
    hipLaunchKernelGGL((k_take_rows<W, false>), dim3((unsigned)blocks), dim3(BC_TAKE_BLOCK), 0, ctx->stream, (const W*)src, idx,
                       (long long)m, (long long)wpr, (W*)dst);
  return hipGetLastError();
}

void bc_take_free(bc_ctx* ctx) {
  for (int h = 0; h < 2; ++h) {
    if (ctx->take_pinned[h]) (void)hipHostFree(ctx->take_pinned[h]);
    if (ctx->take_ev[h]) (void)hipEventDestroy(ctx->take_ev[h]);
    ctx->take_pinned[h] = nullptr;
    ctx->take_pinned_cap[h] = 0;
    ctx->take_ev[h] = nullptr;
  }
}

// the launch alone: indices already on the device and already checked (take_enqueue below; bc_viopt.hip, once per step)
int bc_take_rows_dev(bc_ctx* ctx, const bc_data* src, const long long* idx_dev, int64_t m, void* dst_z) {
  const size_t pitch = (size_t)src->dz * (size_t)src->elem;
  const int w = bc_take_word_bytes((uint64_t)(uintptr_t)src->z, (uint64_t)(uintptr_t)dst_z, src->dz, src->elem);
  const bool flat = bc_take_flat(src->dz, src->elem) != 0;
  hipError_t e;
  if (w == 16) e = launch_take<uint4>(ctx, src->z, idx_dev, m, (int64_t)(pitch / 16), flat, dst_z);
  else if (w == 8) e = launch_take<uint2>(ctx, src->z, idx_dev, m, (int64_t)(pitch / 8), flat, dst_z);
  else e = launch_take<unsigned>(ctx, src->z, idx_dev, m, (int64_t)(pitch / 4), flat, dst_z);
  if (e != hipSuccess) return bc_hip_fail(e, "k_take_rows", __FILE__, __LINE__);
  return BC_OK;
}

// The indices (host, borrowed) -> one of two pinned staging areas of the context -> a device scratch buffer (all grow-only),
// then the launch into dst_z.  `idx` has been read when this returns.  The staging areas take turns, so the only host wait
// is for the index copy of the call BEFORE the previous one (an event): back-to-back takes do not block on each other.
static int take_enqueue(bc_ctx* ctx, const bc_data* src, const int64_t* idx, int64_t m, void* dst_z) {
  const int h = ctx->take_turn;
  if (!ctx->take_ev[h]) BC_HIP(hipEventCreateWithFlags(&ctx->take_ev[h], hipEventDisableTiming));
  else BC_HIP(hipEventSynchronize(ctx->take_ev[h]));
  if ((size_t)m > ctx->take_pinned_cap[h]) {
    if (ctx->take_pinned[h]) (void)hipHostFree(ctx->take_pinned[h]);
    ctx->take_pinned[h] = nullptr;
    ctx->take_pinned_cap[h] = 0;
    const size_t want = (size_t)m + (size_t)m / 2;
    BC_HIP(hipHostMalloc((void**)&ctx->take_pinned[h], want * sizeof(long long), hipHostMallocDefault));
    ctx->take_pinned_cap[h] = want;
  }
  int rc = bc_scratch_grow(ctx, &ctx->take_idx, (size_t)m);      // (8-byte units: one per index)
  if (rc) return rc;
  long long* stage = ctx->take_pinned[h];
  for (int64_t j = 0; j < m; ++j) stage[j] = (long long)idx[j];
  long long* didx = reinterpret_cast<long long*>(ctx->take_idx.p);
  BC_HIP(hipMemcpyAsync(didx, stage, (size_t)m * sizeof(long long), hipMemcpyHostToDevice, ctx->stream));
  BC_HIP(hipEventRecord(ctx->take_ev[h], ctx->stream));
  ctx->take_turn = h ^ 1;
  return bc_take_rows_dev(ctx, src, didx, m, dst_z);
}

extern "C" int bc_data_take_rows(const bc_data* src, const int64_t* idx, int64_t m, bc_data** inout) {
  if (!src || !inout || m < 0 || (m > 0 && !idx)) { bc_set_error("bc_data_take_rows: bad argument"); return BC_INVALID_ARGUMENT; }
  bc_ctx* ctx = src->ctx;
  bc_data* d = *inout;
  if (d) {
    if (d == src) { bc_set_error("bc_data_take_rows: the destination is the source"); return BC_INVALID_ARGUMENT; }
    if (!d->owned) { bc_set_error("bc_data_take_rows: the destination borrows its memory (only an owned handle can be refilled)"); return BC_INVALID_ARGUMENT; }
    if (d->ctx != ctx) { bc_set_error("bc_data_take_rows: the destination belongs to another context"); return BC_INVALID_ARGUMENT; }
    if (d->dz != src->dz) {
      bc_set_error("bc_data_take_rows: the destination holds rows of %d columns, the source %d", (int)d->dz, (int)src->dz);
      return BC_INVALID_ARGUMENT;
    }
    if (d->elem != src->elem) {
      bc_set_error("bc_data_take_rows: the destination stores float%d rows, the source float%d", d->elem * 8, src->elem * 8);
      return BC_INVALID_ARGUMENT;
    }
  }
  if ((uintptr_t)src->z & (uintptr_t)(src->elem - 1)) {
    bc_set_error("bc_data_take_rows: the source rows are not aligned to their element size");
    return BC_INVALID_ARGUMENT;
  }
  for (int64_t j = 0; j < m; ++j)
    if (idx[j] < 0 || idx[j] >= src->n_rows) {
      bc_set_error("bc_data_take_rows: index %lld (position %lld) out of range [0,%lld)", (long long)idx[j], (long long)j,
                   (long long)src->n_rows);
      return BC_INVALID_ARGUMENT;
    }
  // ---- nothing has been enqueued or changed up to here.  From here on only a HIP failure can end the call early: a handle
  // made here is then destroyed (*inout stays NULL), a re-used one is left holding 0 rows if its old rows are gone
  BC_HIP(hipSetDevice(ctx->device));
  const size_t pitch = (size_t)src->dz * (size_t)src->elem;
  const bool fresh = d == nullptr;
  if (fresh) {
    d = new bc_data();
    d->ctx = ctx;
    d->dz = src->dz;
    d->elem = src->elem;
    d->cap_rows = m > 0 ? m : 1;
    hipError_t e = hipMalloc((void**)&d->z, (size_t)d->cap_rows * pitch);
    if (e != hipSuccess) { delete d; return bc_hip_fail(e, "hipMalloc(take)", __FILE__, __LINE__); }
  } else if (m > d->cap_rows) {
    BC_HIP(hipStreamSynchronize(ctx->stream));      // an enqueued kernel may still read the old rows
    if (d->z) (void)hipFree(d->z);
    d->z = nullptr;
    d->n_rows = 0;
    const int64_t cap = d->cap_rows * 2 > m ? d->cap_rows * 2 : m;
    d->cap_rows = 0;
    BC_HIP(hipMalloc((void**)&d->z, (size_t)cap * pitch));
    d->cap_rows = cap;
  }
  if (m > 0) {
    const int rc = take_enqueue(ctx, src, idx, m, d->z);
    if (rc) {
      if (fresh) bc_data_destroy(d);
      else d->n_rows = 0;                            // (part of the rows may have been overwritten)
      return rc;
    }
  }
  d->n_rows = m;
  *inout = d;
  return BC_OK;
}
