// K1 over float32 rows: the instantiations of the kernels of bc_project_k1.h with ZT = float (include/beta_cores_f32.h).  The
// rows are widened to double in registers (exact); Theta, the accumulators, the epilogue and every output are the float64 path's.
#include "bc_project_k1.h"

int bc_k1_launch_f32(bc_ctx* ctx, const ProjArgs& a, int kind, long long count, int model, int ntsel) {
  return bc_k1_launch<float>(ctx, a, kind, count, model, ntsel);
}
