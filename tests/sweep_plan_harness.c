/* Host access to beta_cores_amd/csrc/bc_sweep_plan.h, the header bc_sweep_grid (bc_core.hip) sizes the K3 sweep's grid with.
 * Reads lines "ntiles s n_cu per_cu_override" from standard input and prints the number of blocks for each, after checking what
 * the kernels rely on: at least one block, and no block without a tile unless there is no tile at all.  Exit status 0 when every
 * line was read and held. */
#include <stdio.h>
#include "bc_sweep_plan.h"

int main(void) {
  long long ntiles;
  int s, n_cu, over, got;
  while ((got = scanf("%lld %d %d %d", &ntiles, &s, &n_cu, &over)) == 4) {
    const int g = bc_sweep_plan(ntiles, s, n_cu, over);
    if (g < 1 || (g > 1 && (long long)(g - 1) * BC_SWEEP_WAVES >= ntiles)) {
      printf("bad plan for %lld %d %d %d: %d\n", ntiles, s, n_cu, over, g);
      return 1;
    }
    printf("%d\n", g);
  }
  return got == EOF ? 0 : 2;
}
