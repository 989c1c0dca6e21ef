/* Prints the index arithmetic of csrc/bc_layout.h that tests/pref_model.py restates, for tests/test_pref_cases_cpu.py:
 * one line per S = 1 .. 300: S sp4 batch sp8 r8_bytes, then sample words "w8 t g r sp4 index" / "w4 ..." / "phi row k S index". */
#include <stdio.h>
#include "bc_layout.h"

int main(void) {
  for (int S = 1; S <= 300; ++S)
    printf("S %d %d %d %d %d\n", S, bc_lay_i8_sp4(S), bc_lay_i4_batch(S), bc_lay_i4_sp8(S, bc_lay_i4_batch(S)), bc_lay_r8_bytes(S));
  const long long ts[3] = {0, 1, 11};
  const int gs[3] = {0, 3, 9}, rs[3] = {0, 77, 255};
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b)
      for (int c = 0; c < 3; ++c) {
        printf("w8 %lld %d %d %d %zu\n", ts[a], gs[b], rs[c], 25, bc_lay_i8_word(ts[a], gs[b], rs[c], 25));
        printf("w4 %lld %d %d %d %zu\n", ts[a], gs[b], rs[c], 13, bc_lay_i4_word(ts[a], gs[b], rs[c], 13));
        printf("phi %lld %d %d %zu\n", ts[a] * 100 + rs[c], gs[b], 37, bc_lay_phi_elem(ts[a] * 100 + rs[c], gs[b], 37));
      }
  printf("tiles %lld %lld %lld\n", bc_lay_i8_tiles(0), bc_lay_i8_tiles(256), bc_lay_i8_tiles(257));
  return 0;
}
