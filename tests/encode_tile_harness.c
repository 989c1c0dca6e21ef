/* Host check of beta_cores_amd/csrc/bc_encode_tile.h, the header k_encode_mlp and its launch code share.  A stand-alone
 * program (built with -fsanitize=address,undefined by tests/test_encode_cpu.py; it is never loaded into another process).
 *
 * 1. The tile chooser, exhaustively: the panels' pitches depend on the widest input among the even layers (wa) and among the
 *    odd layers (wb) only, so every depth 1..4 x wa 1..512 x wb 1..512 covers every network of widths 1..512.  Rows per tile
 *    are 16, 32 or 64, the panels fit the device's LDS, more than 16 rows only within the two-blocks-per-CU budget, and no
 *    larger tile would have fitted that budget.
 * 2. The panel / padding index arithmetic, replayed on the host for a list of networks with the kernel's own loops over
 *    lanes, k-steps, row tiles and accumulator registers, in a heap block of EXACTLY bc_enc_lds_bytes (the sanitizer sees any
 *    slot outside it): every slot a contraction reads was written for THIS tile and layer, slots at k >= d hold zeros, every
 *    (row, output) of a layer is produced exactly once, and nothing is written past kpad(d_out).
 * Prints the number of chooser combinations and of simulated networks; exit status 0 when all hold. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "bc_encode_tile.h"

static int check_chooser(const int32_t* w, int L) {
  const int R = bc_enc_tile_rows(w, L);
  const int64_t bytes = bc_enc_lds_bytes(w, L, R);
  if (R < 16 || R > BC_ENC_MAX_ROWS || R % 16 || (R & (R - 1))) return 1;
  if (bytes <= 0 || bytes > BC_ENC_LDS_DEVICE) return 2;
  if (R > 16 && bytes > BC_ENC_LDS_BUDGET) return 3;
  if (R < BC_ENC_MAX_ROWS && bc_enc_lds_bytes(w, L, 2 * R) <= BC_ENC_LDS_BUDGET) return 4;
  return 0;
}

static int simulate(const int32_t* w, int L) {
  const int R = bc_enc_tile_rows(w, L);
  const int64_t n = bc_enc_lds_bytes(w, L, R) / 8;
  const int pitch[2] = {bc_enc_panel_pitch(w, L, 0), bc_enc_panel_pitch(w, L, 1)};
  const int64_t base[2] = {bc_enc_panel_base(w, L, R, 0), bc_enc_panel_base(w, L, R, 1)};
  double* lds = (double*)malloc((size_t)n * sizeof(double));
  unsigned char* wr = (unsigned char*)calloc((size_t)n, 1);
  int* made = (int*)malloc((size_t)R * 512 * sizeof(int));
  int l, e, ot, lane, kk, rt, reg, rc = 0;
  const int kp0 = bc_enc_kpad(w[0]);
  if (!lds || !wr || !made) return 100;
  for (e = 0; e < n; ++e) lds[e] = HUGE_VAL;           /* "leftovers of an earlier tile": infinities */
  for (e = 0; e < R * kp0; ++e) {                         /* the load stage */
    const int r = e / kp0, k = e - r * kp0;
    const int64_t i = base[0] + bc_enc_slot(r, k, pitch[0]);
    lds[i] = k < w[0] ? 1.0 : 0.0;
    wr[i] = 1;
  }
  for (l = 0; l < L && !rc; ++l) {
    const int din = w[l], dout = w[l + 1], last = l == L - 1;
    const int pin = pitch[l & 1], pout = pitch[(l + 1) & 1], ksteps = bc_enc_kpad(din) >> 2, kpo = bc_enc_kpad(dout);
    const int64_t bin = base[l & 1], bout = base[(l + 1) & 1];
    memset(made, 0, (size_t)R * 512 * sizeof(int));
    if (!last) memset(wr + bout, 0, (size_t)R * (size_t)pout);      /* this layer must write all that the next one reads */
    for (ot = 0; ot < bc_enc_otiles(dout) && !rc; ++ot)
      for (lane = 0; lane < 64 && !rc; ++lane) {
        const int o = bc_enc_lane_out(lane, ot);
        for (kk = 0; kk < ksteps; ++kk) {
          const int k = bc_enc_lane_k(lane, kk);
          for (rt = 0; rt < R / 16; ++rt) {
            const int64_t i = bin + bc_enc_slot(bc_enc_lane_row(lane, 0), 0, pin) + bc_enc_slot(rt * 16, k, pin);
            if (!wr[i]) { printf("layer %d reads a slot nobody wrote (row %d, k %d)\n", l, bc_enc_lane_row(lane, rt), k); rc = 5; }
            else if (k >= din && lds[i] != 0.0) { printf("layer %d: padding slot k %d is not zero\n", l, k); rc = 6; }
            else if (k < din && lds[i] != 1.0) { printf("layer %d: slot k %d holds something else\n", l, k); rc = 7; }
          }
        }
        for (rt = 0; rt < R / 16; ++rt)
          for (reg = 0; reg < 4; ++reg) {
            const int r = bc_enc_acc_row(lane, rt, reg);
            if (r < 0 || r >= R || o < 0 || o >= 512) { rc = 8; continue; }
            made[r * 512 + o]++;
            if (!last && o < kpo) {
              const int64_t i = bout + bc_enc_slot(r, o, pout);
              lds[i] = o < dout ? 1.0 : 0.0;
              wr[i] = 1;
            }
          }
      }
    for (e = 0; e < R * 512 && !rc; ++e) {
      const int o = e % 512, want = o < bc_enc_otiles(dout) * 16 ? 1 : 0;
      if (made[e] != want) { printf("layer %d: (row %d, output %d) produced %d times\n", l, e / 512, o, made[e]); rc = 9; }
    }
  }
  free(lds);
  free(wr);
  free(made);
  return rc;
}

int main(void) {
  static const int32_t nets[][6] = {      /* depth, then depth + 1 widths */
    {2, 13, 20, 20}, {1, 1, 1}, {2, 3, 5, 7}, {1, 32, 512}, {2, 13, 100, 100}, {2, 512, 512, 512}, {3, 33, 130, 4, 9},
    {4, 20, 20, 20, 20, 20}, {4, 512, 512, 512, 512, 512}, {4, 509, 511, 510, 1, 2}, {4, 1, 512, 1, 512, 1}, {1, 4, 4},
    {4, 5, 3, 17, 16, 15}, {3, 127, 129, 63, 65}, {2, 256, 255, 257}, {4, 8, 12, 16, 24, 28}};
  long checked = 0;
  int L, wa, wb, l, rc;
  unsigned i;
  for (L = 1; L <= 4; ++L)
    for (wa = 1; wa <= 512; ++wa)
      for (wb = 1; wb <= (L > 1 ? 512 : 1); ++wb) {
        int32_t w[5], w2[5];
        for (l = 0; l <= L; ++l) w[l] = w2[l] = (l & 1) ? wb : wa;
        w[L] = 1;
        w2[L] = 512;                                  /* the last width is never staged: it must not matter */
        rc = check_chooser(w, L);
        if (rc || bc_enc_tile_rows(w, L) != bc_enc_tile_rows(w2, L) || bc_enc_lds_bytes(w, L, 16) != bc_enc_lds_bytes(w2, L, 16)) {
          printf("chooser: depth %d, even widths %d, odd widths %d: check %d\n", L, wa, wb, rc);
          return 1;
        }
        ++checked;
      }
  {
    const int32_t bad1[2] = {0, 4}, bad2[2] = {4, 513}, ok[2] = {4, 4};
    if (bc_enc_tile_rows(bad1, 1) || bc_enc_tile_rows(bad2, 1) || bc_enc_tile_rows(ok, 0) || bc_enc_tile_rows(ok, 5)) return 2;
  }
  for (i = 0; i < sizeof(nets) / sizeof(nets[0]); ++i) {
    rc = simulate(nets[i] + 1, nets[i][0]);
    if (rc) { printf("network %u: %d\n", i, rc); return 3; }
  }
  printf("%ld chooser combinations, %u networks\n", checked, (unsigned)(sizeof(nets) / sizeof(nets[0])));
  return 0;
}
