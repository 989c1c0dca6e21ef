/* Prints the pre-filter's control block as beta_cores_amd/csrc/bc_pref_ctrl.h names it, for tests/test_pref_ctrl_cpu.py:
 * "block <bytes> <ints>", then one line per field: "field <name> <word index> <width in words>". */
#include <stdio.h>
#include "bc_pref_ctrl.h"

#define FIELD(name, words) printf("field %s %d %d\n", #name, name, words)

int main(void) {
  printf("block %d %d\n", BC_PCTL_BYTES, BC_PCTL_INTS);
  FIELD(BC_PCTL_OVERFLOWED, 1);
  FIELD(BC_PCTL_OVERFLOWS, 1);
  FIELD(BC_PCTL_SWEEPS, 2);
  FIELD(BC_PCTL_RESCORED, 2);
  FIELD(BC_PCTL_RING_POS, 1);
  FIELD(BC_PCTL_L1_PASSED, 2);
  FIELD(BC_PCTL_SPILL_N, 1);
  FIELD(BC_PCTL_BB_THETA, 2);
  return 0;
}
