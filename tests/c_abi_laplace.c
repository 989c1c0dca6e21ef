/* A plain-C consumer of include/beta_cores_laplace.h: compiles as C99 against both headers and links every entry point the
 * extension header declares; run without a GPU it checks that all-NULL arguments are refused with a message. */
#include <stdio.h>
#include "beta_cores_laplace.h"

int main(void) {
  void* syms[] = {(void*)bc_logistic_newton_pass};
  printf("abi %d, %d extension entry points\n", bc_version(), (int)(sizeof(syms) / sizeof(syms[0])));
  if (bc_logistic_newton_pass(NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) != BC_INVALID_ARGUMENT) return 2;
  if (!bc_last_error() || !bc_last_error()[0]) return 3;
  return 0;
}
