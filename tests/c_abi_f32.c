/* A plain-C consumer of include/beta_cores_f32.h: compiles as C99 against the headers and links every entry point the
 * extension header declares; run without a GPU it checks that all-NULL arguments are refused with a message. */
#include <stdio.h>
#include "beta_cores_f32.h"

int main(void) {
  void* syms[] = {(void*)bc_data_from_host_f32, (void*)bc_data_from_device_f32, (void*)bc_project_from_host_f32,
                  (void*)bc_data_elem_bytes};
  printf("abi %d, %d extension entry points\n", bc_version(), (int)(sizeof(syms) / sizeof(syms[0])));
  if (bc_data_from_host_f32(NULL, NULL, 0, 0, NULL) != BC_INVALID_ARGUMENT) return 2;
  if (!bc_last_error() || !bc_last_error()[0]) return 3;
  if (bc_data_from_device_f32(NULL, NULL, 0, 0, NULL) != BC_INVALID_ARGUMENT) return 4;
  if (bc_project_from_host_f32(NULL, NULL, 0, 0, 0, NULL, 0, NULL, 0, 0, NULL, NULL) != BC_INVALID_ARGUMENT) return 5;
  if (bc_data_elem_bytes(NULL, NULL) != BC_INVALID_ARGUMENT) return 6;
  if (!bc_last_error() || !bc_last_error()[0]) return 7;
  return 0;
}
