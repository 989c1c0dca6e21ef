// bc_encode.hip -- the device feature encoder (include/beta_cores_encode.h): resident raw rows -> resident encoded rows.
//
// k_encode_mlp runs a whole network of L <= 4 layers  h <- act((W h + b) * s + t)  on a tile of R rows per block.  The tile's
// inputs are widened into an LDS panel; every layer but the last reads one panel and writes the other; the last layer's
// features go from the accumulators to HBM, beside the pass-through columns, which are copied from the source.  So HBM sees
// the raw rows once and the encoded rows once, whatever the depth.
//
// The contraction is v_mfma_f64_16x16x4_f64 with the activations as A (16 tile rows x 4 k) and the weights as B (4 k x 16
// outputs), accumulators in VGPRs: lane l holds, for output l & 15, the tile rows (l >> 4) + 4 * reg -- consecutive lanes
// write consecutive columns of a row, in LDS and in HBM alike.  A wave owns 16 outputs at a time and all R / 16 row tiles of
// them, so one weight fragment (read from global memory: the weights are L2-resident, 2 MB at most per layer) serves R rows.
// K runs in steps of 4 from 0 upwards, one accumulator chain per result: the additions of a dot product and their order are a
// function of the layer's input width alone -- not of n, the tile, the row's place in it, or the storage types.
//
// Ragged shapes are ZERO-padded on both operands: panel slots [d, kpad(d)) and the rows past n are written as zeros by the
// stage that fills the panel (never inherited from an earlier tile), weights outside d_out x d_in are read as zeros, and a
// padded output column is stored as 0, not as the (0-weight) product -- inf * 0 would be a NaN.  Shapes: bc_encode_tile.h.
#include "bc_internal.h"
#include "bc_encode_tile.h"
#include "../../include/beta_cores_encode.h"

typedef double enc_double4 __attribute__((ext_vector_type(4)));

#define BC_ENC_BLOCK 256
#define BC_ENC_WAVES (BC_ENC_BLOCK / BC_WAVE)

struct EncLayer {
  const double* W;      // dout x din, row-major
  const double* b;      // dout each
  const double* s;
  const double* t;
  int din, dout, relu;
};

struct EncArgs {
  EncLayer layer[BC_ENC_MAX_LAYERS];
  int n_layers;
  int pitch[2];         // row pitch of the two panels (doubles)
  long long n;          // rows
  int src_w, out_w;     // columns of a source / an output row
  int pass;             // pass-through columns
};

struct bc_encoder {
  bc_ctx* ctx = nullptr;
  int n_layers = 0;
  int32_t widths[BC_ENC_MAX_LAYERS + 1] = {};
  double* dev[BC_ENC_MAX_LAYERS] = {};          // W | b | s | t of a layer, one allocation
  double* pinned[BC_ENC_MAX_LAYERS] = {};       // its pinned staging area
  hipEvent_t ev[BC_ENC_MAX_LAYERS] = {};        // the last copy out of that area
  bool is_set[BC_ENC_MAX_LAYERS] = {};
  int relu[BC_ENC_MAX_LAYERS] = {};
  int rows = 0;                                 // rows per tile (bc_enc_tile_rows)
  size_t lds = 0;
};

// ReLU as torch and np.maximum(x, 0) have it: a NaN passes through (fmax would return 0)
__device__ __forceinline__ double enc_relu(double x) { return x > 0. ? x : (x != x ? x : 0.); }

template <typename TIn, typename TOut, int RT>
// (two blocks per CU: at most 256 registers per lane, which also makes the compiler keep the MFMA accumulators in VGPRs)
__global__ __launch_bounds__(BC_ENC_BLOCK, 2) void k_encode_mlp(const EncArgs a, const TIn* __restrict__ src, TOut* __restrict__ out) {
  extern __shared__ double enc_lds[];
  constexpr int R = RT * 16;
  const int tid = threadIdx.x, lane = tid & (BC_WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  double* panel[2] = {enc_lds, enc_lds + (size_t)R * a.pitch[0]};
  const int d0 = a.layer[0].din, kp0 = bc_enc_kpad(d0), dl = a.layer[a.n_layers - 1].dout;
  const long long ntiles = (a.n + R - 1) / R;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long row0 = tile * R;
    // ---- the tile's inputs, widened, into panel 0: every slot of [0, kpad(d0)) of every one of the R rows is written
    for (int e = tid; e < R * kp0; e += BC_ENC_BLOCK) {
      const int r = e / kp0, k = e - r * kp0;
      const long long row = row0 + r;
      double v = 0.;
      if (row < a.n && k < d0) v = (double)src[(size_t)row * (size_t)a.src_w + (size_t)k];
      panel[0][bc_enc_slot(r, k, a.pitch[0])] = v;
    }
    // ---- pass-through columns: source -> output (same type: the same bits; float -> double exact; double -> float rounds once)
    for (int e = tid; e < R * a.pass; e += BC_ENC_BLOCK) {
      const int r = e / a.pass, c = e - r * a.pass;
      const long long row = row0 + r;
      if (row < a.n) out[(size_t)row * (size_t)a.out_w + (size_t)(dl + c)] = (TOut)src[(size_t)row * (size_t)a.src_w + (size_t)(d0 + c)];
    }
    __syncthreads();
    for (int l = 0; l < a.n_layers; ++l) {
      const EncLayer& L = a.layer[l];
      const bool last = l == a.n_layers - 1;
      const double* __restrict__ in = panel[l & 1];
      double* __restrict__ nxt = panel[(l + 1) & 1];
      const int pin = a.pitch[l & 1], pout = a.pitch[(l + 1) & 1];
      const int ksteps = bc_enc_kpad(L.din) >> 2, kpo = bc_enc_kpad(L.dout);
      for (int ot = wave; ot < bc_enc_otiles(L.dout); ot += BC_ENC_WAVES) {
        const int o = bc_enc_lane_out(lane, ot);
        const bool o_ok = o < L.dout;
        const double* __restrict__ wrow = L.W + (size_t)(o_ok ? o : 0) * (size_t)L.din;
        const double* __restrict__ hrow = in + bc_enc_slot(bc_enc_lane_row(lane, 0), 0, pin);
        enc_double4 acc[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[rt] = (enc_double4){0., 0., 0., 0.};
        // the weight fragment of the NEXT k-step is requested before this step's MFMAs are issued (L2 latency under them)
        const int kq = bc_enc_lane_k(lane, 0);
        double wn = (o_ok && kq < L.din) ? wrow[kq] : 0.;
        for (int kk = 0; kk < ksteps; ++kk) {
          const int k = bc_enc_lane_k(lane, kk);
          const double wv = wn;
          const int k1 = k + 4;
          wn = (o_ok && kk + 1 < ksteps && k1 < L.din) ? wrow[k1] : 0.;
#pragma unroll
          for (int rt = 0; rt < RT; ++rt) {
            const double hv = hrow[bc_enc_slot(rt * 16, k, pin)];
            acc[rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(hv, wv, acc[rt], 0, 0, 0);
          }
        }
        // ---- epilogue, one rounding per op: (acc + b) * s + t, then the activation
        const double bb = o_ok ? L.b[o] : 0., ss = o_ok ? L.s[o] : 1., tt = o_ok ? L.t[o] : 0.;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            const int r = bc_enc_acc_row(lane, rt, reg);
            double v = (acc[rt][reg] + bb) * ss;
            v = v + tt;
            if (L.relu) v = enc_relu(v);
            if (last) {
              const long long row = row0 + r;
              if (o_ok && row < a.n) out[(size_t)row * (size_t)a.out_w + (size_t)o] = (TOut)v;
            } else if (o < kpo) {
              nxt[bc_enc_slot(r, o, pout)] = o_ok ? v : 0.;      // (the padded slots of the next layer's K: zeros)
            }
          }
        }
      }
      __syncthreads();      // the next layer reads what this one wrote; the next tile refills panel 0
    }
  }
}

template <typename TIn, typename TOut, int RT>
static hipError_t launch_encode_rt(const bc_encoder* enc, const EncArgs& a, const void* src, void* out, unsigned blocks) {
  auto kern = &k_encode_mlp<TIn, TOut, RT>;
  if (enc->lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)enc->lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(BC_ENC_BLOCK), enc->lds, enc->ctx->stream, a, (const TIn*)src, (TOut*)out);
  return hipGetLastError();
}

template <typename TIn, typename TOut>
static hipError_t launch_encode(const bc_encoder* enc, const EncArgs& a, const void* src, void* out, unsigned blocks) {
  switch (enc->rows) {
    case 64: return launch_encode_rt<TIn, TOut, 4>(enc, a, src, out, blocks);
    case 32: return launch_encode_rt<TIn, TOut, 2>(enc, a, src, out, blocks);
    default: return launch_encode_rt<TIn, TOut, 1>(enc, a, src, out, blocks);
  }
}

static size_t enc_layer_doubles(const bc_encoder* e, int l) {
  return (size_t)e->widths[l + 1] * (size_t)e->widths[l] + 3 * (size_t)e->widths[l + 1];
}

extern "C" int bc_encoder_create(bc_ctx* ctx, int32_t n_layers, const int32_t* widths, bc_encoder** out) {
  if (!ctx || !widths || !out) { bc_set_error("bc_encoder_create: bad argument"); return BC_INVALID_ARGUMENT; }
  if (n_layers < 1 || n_layers > BC_ENC_MAX_LAYERS) {
    bc_set_error("bc_encoder_create: %d layers (an encoder has 1..%d)", (int)n_layers, BC_ENC_MAX_LAYERS);
    return BC_INVALID_ARGUMENT;
  }
  for (int l = 0; l <= n_layers; ++l)
    if (widths[l] < 1 || widths[l] > BC_ENC_MAX_WIDTH) {
      bc_set_error("bc_encoder_create: width %d of %d (every width is in 1..%d)", l, (int)widths[l], BC_ENC_MAX_WIDTH);
      return BC_INVALID_ARGUMENT;
    }
  const int rows = bc_enc_tile_rows(widths, n_layers);
  const size_t lds = (size_t)bc_enc_lds_bytes(widths, n_layers, rows);
  if (rows < 16 || lds > (size_t)ctx->max_lds) {
    bc_set_error("bc_encoder_create: a 16-row tile of this network stages %zu bytes of LDS, the device allows %d", lds, ctx->max_lds);
    return BC_INVALID_ARGUMENT;
  }
  BC_HIP(hipSetDevice(ctx->device));
  bc_encoder* e = new bc_encoder();
  e->ctx = ctx;
  e->n_layers = n_layers;
  for (int l = 0; l <= n_layers; ++l) e->widths[l] = widths[l];
  e->rows = rows;
  e->lds = lds;
  for (int l = 0; l < n_layers; ++l) {
    const size_t bytes = enc_layer_doubles(e, l) * sizeof(double);
    hipError_t err = hipMalloc((void**)&e->dev[l], bytes);
    if (err == hipSuccess) err = hipHostMalloc((void**)&e->pinned[l], bytes, hipHostMallocDefault);
    if (err == hipSuccess) err = hipEventCreateWithFlags(&e->ev[l], hipEventDisableTiming);
    if (err != hipSuccess) {
      (void)bc_encoder_destroy(e);
      return bc_hip_fail(err, "bc_encoder_create", __FILE__, __LINE__);
    }
  }
  *out = e;
  return BC_OK;
}

extern "C" int bc_encoder_set_layer(bc_encoder* enc, int32_t layer, const double* W, const double* b, const double* s, const double* t,
                                    int32_t relu) {
  if (!enc || !W) { bc_set_error("bc_encoder_set_layer: bad argument"); return BC_INVALID_ARGUMENT; }
  if (layer < 0 || layer >= enc->n_layers) {
    bc_set_error("bc_encoder_set_layer: layer %d of an encoder of %d layers", (int)layer, enc->n_layers);
    return BC_INVALID_ARGUMENT;
  }
  bc_ctx* ctx = enc->ctx;
  BC_HIP(hipSetDevice(ctx->device));
  const size_t din = (size_t)enc->widths[layer], dout = (size_t)enc->widths[layer + 1];
  if (enc->is_set[layer]) BC_HIP(hipEventSynchronize(enc->ev[layer]));      // the previous copy out of the staging area
  double* st = enc->pinned[layer];
  for (size_t i = 0; i < dout * din; ++i) st[i] = W[i];
  double* pb = st + dout * din;
  for (size_t i = 0; i < dout; ++i) {
    pb[i] = b ? b[i] : 0.;
    pb[dout + i] = s ? s[i] : 1.;
    pb[2 * dout + i] = t ? t[i] : 0.;
  }
  BC_HIP(hipMemcpyAsync(enc->dev[layer], st, enc_layer_doubles(enc, layer) * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  BC_HIP(hipEventRecord(enc->ev[layer], ctx->stream));
  enc->relu[layer] = relu ? 1 : 0;
  enc->is_set[layer] = true;
  return BC_OK;
}

extern "C" int bc_encoder_destroy(bc_encoder* enc) {
  if (!enc) { bc_set_error("bc_encoder_destroy: bad argument"); return BC_INVALID_ARGUMENT; }
  (void)hipSetDevice(enc->ctx->device);
  (void)hipStreamSynchronize(enc->ctx->stream);      // an enqueued encode may still read the parameters
  for (int l = 0; l < BC_ENC_MAX_LAYERS; ++l) {
    if (enc->dev[l]) (void)hipFree(enc->dev[l]);
    if (enc->pinned[l]) (void)hipHostFree(enc->pinned[l]);
    if (enc->ev[l]) (void)hipEventDestroy(enc->ev[l]);
  }
  delete enc;
  return BC_OK;
}

extern "C" int bc_data_encode(const bc_encoder* enc, const bc_data* src, int32_t pass_cols, int32_t out_elem_bytes, bc_data** inout) {
  if (!enc || !src || !inout) { bc_set_error("bc_data_encode: bad argument"); return BC_INVALID_ARGUMENT; }
  if (pass_cols < 0) { bc_set_error("bc_data_encode: pass_cols %d is negative", (int)pass_cols); return BC_INVALID_ARGUMENT; }
  if (out_elem_bytes != 4 && out_elem_bytes != 8) {
    bc_set_error("bc_data_encode: out_elem_bytes %d (4 = float32 or 8 = float64)", (int)out_elem_bytes);
    return BC_INVALID_ARGUMENT;
  }
  for (int l = 0; l < enc->n_layers; ++l)
    if (!enc->is_set[l]) { bc_set_error("bc_data_encode: layer %d of the encoder was never set", l); return BC_INVALID_ARGUMENT; }
  bc_ctx* ctx = enc->ctx;
  if (src->ctx != ctx) { bc_set_error("bc_data_encode: the source belongs to another context than the encoder"); return BC_INVALID_ARGUMENT; }
  const int d0 = enc->widths[0], dl = enc->widths[enc->n_layers];
  if ((int64_t)src->dz != (int64_t)d0 + pass_cols) {
    bc_set_error("bc_data_encode: the source holds rows of %d columns, the encoder takes %d + %d pass-through", (int)src->dz, d0,
                 (int)pass_cols);
    return BC_INVALID_ARGUMENT;
  }
  const int32_t out_w = dl + pass_cols;
  bc_data* d = *inout;
  if (d) {
    if (d == src) { bc_set_error("bc_data_encode: the destination is the source"); return BC_INVALID_ARGUMENT; }
    if (!d->owned) { bc_set_error("bc_data_encode: the destination borrows its memory (only an owned handle can be refilled)"); return BC_INVALID_ARGUMENT; }
    if (d->ctx != ctx) { bc_set_error("bc_data_encode: the destination belongs to another context"); return BC_INVALID_ARGUMENT; }
    if (d->dz != out_w) {
      bc_set_error("bc_data_encode: the destination holds rows of %d columns, the encoded rows have %d", (int)d->dz, (int)out_w);
      return BC_INVALID_ARGUMENT;
    }
    if (d->elem != out_elem_bytes) {
      bc_set_error("bc_data_encode: the destination stores float%d rows, float%d was asked for", d->elem * 8, (int)out_elem_bytes * 8);
      return BC_INVALID_ARGUMENT;
    }
  }
  if ((uintptr_t)src->z & (uintptr_t)(src->elem - 1)) {
    bc_set_error("bc_data_encode: the source rows are not aligned to their element size");
    return BC_INVALID_ARGUMENT;
  }
  // ---- nothing has been enqueued or changed up to here.  From here on only a HIP failure can end the call early: a handle
  // made here is then destroyed (*inout stays NULL), a re-used one is left holding 0 rows if its old rows are gone
  BC_HIP(hipSetDevice(ctx->device));
  const int64_t n = src->n_rows;
  const size_t pitch = (size_t)out_w * (size_t)out_elem_bytes;
  const bool fresh = d == nullptr;
  if (fresh) {
    d = new bc_data();
    d->ctx = ctx;
    d->dz = out_w;
    d->elem = out_elem_bytes;
    d->cap_rows = n > 0 ? n : 1;
    hipError_t e = hipMalloc((void**)&d->z, (size_t)d->cap_rows * pitch);
    if (e != hipSuccess) { delete d; return bc_hip_fail(e, "hipMalloc(encode)", __FILE__, __LINE__); }
  } else if (n > d->cap_rows) {
    BC_HIP(hipStreamSynchronize(ctx->stream));      // an enqueued kernel may still read the old rows
    if (d->z) (void)hipFree(d->z);
    d->z = nullptr;
    d->n_rows = 0;
    const int64_t cap = d->cap_rows * 2 > n ? d->cap_rows * 2 : n;
    d->cap_rows = 0;
    BC_HIP(hipMalloc((void**)&d->z, (size_t)cap * pitch));
    d->cap_rows = cap;
  }
  if (n > 0) {
    EncArgs a;
    for (int l = 0; l < BC_ENC_MAX_LAYERS; ++l) a.layer[l] = EncLayer{nullptr, nullptr, nullptr, nullptr, 0, 0, 0};
    for (int l = 0; l < enc->n_layers; ++l) {
      const size_t din = (size_t)enc->widths[l], dout = (size_t)enc->widths[l + 1];
      const double* p = enc->dev[l];
      a.layer[l] = EncLayer{p, p + dout * din, p + dout * din + dout, p + dout * din + 2 * dout, (int)din, (int)dout, enc->relu[l]};
    }
    a.n_layers = enc->n_layers;
    a.pitch[0] = bc_enc_panel_pitch(enc->widths, enc->n_layers, 0);
    a.pitch[1] = bc_enc_panel_pitch(enc->widths, enc->n_layers, 1);
    a.n = (long long)n;
    a.src_w = src->dz;
    a.out_w = out_w;
    a.pass = pass_cols;
    const long long ntiles = ((long long)n + enc->rows - 1) / enc->rows;
    const long long blocks = (long long)bc_enc_grid_blocks((int64_t)enc->lds, ctx->n_cu, (int64_t)ntiles);
    hipError_t e;
    if (src->elem == 4)
      e = out_elem_bytes == 4 ? launch_encode<float, float>(enc, a, src->z, d->z, (unsigned)blocks)
                              : launch_encode<float, double>(enc, a, src->z, d->z, (unsigned)blocks);
    else
      e = out_elem_bytes == 4 ? launch_encode<double, float>(enc, a, src->z, d->z, (unsigned)blocks)
                              : launch_encode<double, double>(enc, a, src->z, d->z, (unsigned)blocks);
    if (e != hipSuccess) {
      if (fresh) bc_data_destroy(d);
      else d->n_rows = 0;                            // (part of the rows may have been overwritten)
      return bc_hip_fail(e, "k_encode_mlp", __FILE__, __LINE__);
    }
  }
  d->n_rows = n;
  *inout = d;
  return BC_OK;
}
