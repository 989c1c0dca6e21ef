// bc_encode_tile.h -- the shape arithmetic of k_encode_mlp (bc_encode.hip): how many rows a block owns, where its two LDS
// panels lie, which slot of a panel holds activation (row r, column k) and how many blocks are launched.  Plain C, shared by
// the kernel, its launch code and two host harnesses: tests/encode_tile_harness.c walks every width 1..512 and every depth 1..4
// without a GPU, tests/encode_shapes_harness.c prints the launch shapes that the long-walk GPU tests are sized by.
//
// A block runs all layers on a tile of R rows.  Layer l reads its input (width d[l]) from panel l & 1 and, unless it is the
// last one, writes its output into panel (l + 1) & 1; the last layer's features go to HBM from registers.  So panel 0 holds the
// widths d[0], d[2], panel 1 the widths d[1], d[3] -- d[L] is never staged.  The contraction walks K in steps of 4
// (v_mfma_f64_16x16x4_f64), so a row of width d occupies bc_enc_kpad(d) slots, the last ones ZERO; a panel's row pitch is the
// widest such row, made = 4 (mod 8) doubles so that the 16 rows x 4 columns one MFMA operand read touches fall into distinct
// bank pairs.
#ifndef BC_ENCODE_TILE_H
#define BC_ENCODE_TILE_H
#include <stdint.h>

#if defined(__HIPCC__)
#define BC_ENC __host__ __device__ __forceinline__
#else
#define BC_ENC static inline
#endif

#define BC_ENC_MAX_LAYERS 4
#define BC_ENC_MAX_WIDTH 512
#define BC_ENC_LDS_DEVICE (160 * 1024)        /* LDS of a gfx950 CU */
#define BC_ENC_LDS_BUDGET (BC_ENC_LDS_DEVICE / 2)  /* two blocks per CU where a 16-row tile allows it */
#define BC_ENC_MAX_ROWS 64                    /* rows per tile: 16, 32 or 64 (4 accumulator tiles of 8 VGPRs per wave at most) */

/* slots a row of width d takes in a panel: d rounded up to the MFMA's K step */
BC_ENC int bc_enc_kpad(int d) { return (d + 3) & ~3; }

/* 16-wide output tiles of a layer of d outputs */
BC_ENC int bc_enc_otiles(int d) { return (d + 15) >> 4; }

/* row pitch (doubles) of a panel whose widest row has width d: >= bc_enc_kpad(d), = 4 (mod 8) */
BC_ENC int bc_enc_pitch(int d) {
  const int k = bc_enc_kpad(d);
  return (k & 7) == 4 ? k : k + 4;
}

/* row pitch of panel p (0 or 1): over the layers l < n_layers with (l & 1) == p, the widest input d[l]; 0 if there is none */
BC_ENC int bc_enc_panel_pitch(const int32_t* widths, int n_layers, int p) {
  int l, w = 0;
  for (l = p; l < n_layers; l += 2)
    if (widths[l] > w) w = widths[l];
  return w > 0 ? bc_enc_pitch(w) : 0;
}

/* bytes of LDS a tile of `rows` rows takes */
BC_ENC int64_t bc_enc_lds_bytes(const int32_t* widths, int n_layers, int rows) {
  return (int64_t)rows * 8 * ((int64_t)bc_enc_panel_pitch(widths, n_layers, 0) + bc_enc_panel_pitch(widths, n_layers, 1));
}

/* Rows per tile: the largest of 64, 32, 16 whose panels fit BC_ENC_LDS_BUDGET (two blocks per CU); 16 rows of the widest
 * networks (two 512-wide panels: 132 096 bytes) do not, they take one block per CU within BC_ENC_LDS_DEVICE.
 * Returns 0 for arguments outside 1 <= n_layers <= 4, 1 <= width <= 512. */
BC_ENC int bc_enc_tile_rows(const int32_t* widths, int n_layers) {
  int l, r;
  if (n_layers < 1 || n_layers > BC_ENC_MAX_LAYERS) return 0;
  for (l = 0; l <= n_layers; ++l)
    if (widths[l] < 1 || widths[l] > BC_ENC_MAX_WIDTH) return 0;
  for (r = BC_ENC_MAX_ROWS; r > 16; r >>= 1)
    if (bc_enc_lds_bytes(widths, n_layers, r) <= BC_ENC_LDS_BUDGET) return r;
  return bc_enc_lds_bytes(widths, n_layers, 16) <= BC_ENC_LDS_DEVICE ? 16 : 0;
}

/* The grid of k_encode_mlp (a persistent kernel: block b walks the tiles b, b + blocks, ...): as many blocks per CU as their LDS
 * lets be resident, 1 .. 4, and never more blocks than tiles. */
BC_ENC int64_t bc_enc_per_cu(int64_t lds) {
  int64_t per_cu = BC_ENC_LDS_DEVICE / (lds > 0 ? lds : 1);
  if (per_cu > 4) per_cu = 4;
  if (per_cu < 1) per_cu = 1;
  return per_cu;
}
BC_ENC int64_t bc_enc_grid_blocks(int64_t lds, int n_cu, int64_t ntiles) {
  const int64_t blocks = (int64_t)n_cu * bc_enc_per_cu(lds);
  return blocks > ntiles ? ntiles : blocks;
}

/* offset (doubles, from the start of the dynamic LDS) of panel p of a tile of `rows` rows */
BC_ENC int64_t bc_enc_panel_base(const int32_t* widths, int n_layers, int rows, int p) {
  return p == 0 ? 0 : (int64_t)rows * bc_enc_panel_pitch(widths, n_layers, 0);
}

/* slot of activation (row r of the tile, column k) in a panel of row pitch `pitch`, relative to the panel's base */
BC_ENC int bc_enc_slot(int r, int k, int pitch) { return r * pitch + k; }

/* The MFMA operand maps of v_mfma_f64_16x16x4_f64, as the kernel uses them: lane `lane` of a wave supplies, in k-step kk of
 * row tile rt, activation (row, k) as A and weight (out, k) as B, and receives in accumulator register reg the result for
 * (row, out). */
BC_ENC int bc_enc_lane_row(int lane, int rt) { return rt * 16 + (lane & 15); }       /* A operand: tile row */
BC_ENC int bc_enc_lane_k(int lane, int kk) { return kk * 4 + (lane >> 4); }          /* A and B operands: k */
BC_ENC int bc_enc_lane_out(int lane, int ot) { return ot * 16 + (lane & 15); }       /* B operand and result: output */
BC_ENC int bc_enc_acc_row(int lane, int rt, int reg) { return rt * 16 + (lane >> 4) + 4 * reg; }   /* result: tile row */

#endif /* BC_ENCODE_TILE_H */
