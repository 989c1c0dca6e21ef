/* The launch shapes of k_encode_mlp (beta_cores_amd/csrc/bc_encode_tile.h), compiled for the host by
 * tests/test_encode_shapes_cpu.py.
 *   encode_shapes_harness nets N_CU:N:W0,W1,.. ...   one line per argument:   rows  lds_bytes  blocks
 *       rows = bc_enc_tile_rows, lds_bytes = bc_enc_lds_bytes at that many rows, blocks = bc_enc_grid_blocks for N rows on N_CU CUs
 *   encode_shapes_harness classes                    the distinct (rows, blocks per CU), one per line
 *       over every one-layer network (d0, 1) and every two-layer network (d0, d1, 1), d = 1 .. 512.  A panel's pitch is that of
 *       its widest row, so deeper networks stage no (pitch 0, pitch 1) pair that these do not. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "bc_encode_tile.h"

static int parse(const char* arg, int* n_cu, long long* n, int32_t* widths) {
  char* end;
  int k = 0;
  *n_cu = (int)strtol(arg, &end, 10);
  if (*end != ':') return -1;
  *n = strtoll(end + 1, &end, 10);
  if (*end != ':') return -1;
  while (k <= BC_ENC_MAX_LAYERS) {
    widths[k++] = (int32_t)strtol(end + 1, &end, 10);
    if (*end == 0) return k - 1;
    if (*end != ',') return -1;
  }
  return -1;
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "nets")) {
    for (int i = 2; i < argc; ++i) {
      int32_t widths[BC_ENC_MAX_LAYERS + 1];
      int n_cu;
      long long n;
      const int n_layers = parse(argv[i], &n_cu, &n, widths);
      if (n_layers < 1) { fprintf(stderr, "cannot read %s\n", argv[i]); return 1; }
      const int rows = bc_enc_tile_rows(widths, n_layers);
      if (rows < 16) { fprintf(stderr, "%s: no tile\n", argv[i]); return 1; }
      const int64_t lds = bc_enc_lds_bytes(widths, n_layers, rows);
      printf("%d %lld %lld\n", rows, (long long)lds, (long long)bc_enc_grid_blocks(lds, n_cu, (n + rows - 1) / rows));
    }
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "classes")) {
    static int seen[BC_ENC_MAX_ROWS + 1][5];
    for (int d0 = 1; d0 <= BC_ENC_MAX_WIDTH; ++d0)
      for (int d1 = 0; d1 <= BC_ENC_MAX_WIDTH; ++d1) {      /* d1 = 0: the one-layer network (d0, 1) */
        int32_t widths[3] = {d0, d1 ? d1 : 1, 1};
        const int n_layers = d1 ? 2 : 1;
        const int rows = bc_enc_tile_rows(widths, n_layers);
        if (rows < 16 || rows > BC_ENC_MAX_ROWS) { fprintf(stderr, "(%d, %d): %d rows\n", d0, d1, rows); return 1; }
        const int64_t per_cu = bc_enc_per_cu(bc_enc_lds_bytes(widths, n_layers, rows));
        if (per_cu < 1 || per_cu > 4) { fprintf(stderr, "(%d, %d): %lld blocks per CU\n", d0, d1, (long long)per_cu); return 1; }
        seen[rows][per_cu] = 1;
      }
    for (int rows = 0; rows <= BC_ENC_MAX_ROWS; ++rows)
      for (int p = 1; p <= 4; ++p)
        if (seen[rows][p]) printf("%d %d\n", rows, p);
    return 0;
  }
  fprintf(stderr, "usage: %s nets N_CU:N:W0,W1,.. ... | classes\n", argv[0]);
  return 2;
}
