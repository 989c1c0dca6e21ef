/* The shape classes of the two-level sweep (beta_cores_amd/csrc/bc_layout.h), compiled for the host by
 * tests/test_two_level_shapes_cpu.py: for S = 1 .. 256 one line
 *     S  U  batches  lines
 * with U = bc_lay_i4_batch(S) (the k_sweep_i4<MODE, U> instance the host launches), batches = bc_lay_i4_sp8(S, U) / U (batches
 * a wave consumes per 256-row tile) and lines = bc_lay_r8_bytes(S) / 128 (cache lines of a row's int8 record). */
#include <stdio.h>
#include "bc_layout.h"

int main(void) {
  for (int S = 1; S <= 256; ++S) {
    const int U = bc_lay_i4_batch(S);
    const int sp8 = bc_lay_i4_sp8(S, U), rb = bc_lay_r8_bytes(S);
    if (sp8 % U != 0 || rb % 128 != 0) { fprintf(stderr, "S = %d: sp8 %d, U %d, record %d bytes\n", S, sp8, U, rb); return 1; }
    printf("%d %d %d %d\n", S, U, sp8 / U, rb / 128);
  }
  return 0;
}
