/* A plain-C consumer of include/beta_cores_take.h: compiles as C99 against the headers and links the entry point the
 * extension header declares; run without a GPU it checks that NULL arguments are refused with a message. */
#include <stdio.h>
#include "beta_cores_take.h"

int main(void) {
  void* syms[] = {(void*)bc_data_take_rows};
  bc_data* out = NULL;
  int64_t idx[1] = {0};
  printf("abi %d, %d extension entry points\n", bc_version(), (int)(sizeof(syms) / sizeof(syms[0])));
  if (bc_data_take_rows(NULL, NULL, 0, NULL) != BC_INVALID_ARGUMENT) return 2;
  if (!bc_last_error() || !bc_last_error()[0]) return 3;
  if (bc_data_take_rows(NULL, idx, 1, &out) != BC_INVALID_ARGUMENT || out != NULL) return 4;
  return 0;
}
