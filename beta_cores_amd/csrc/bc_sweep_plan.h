// bc_sweep_plan.h -- how many blocks the K3 sweep (bc_sweep.hip, bc_sweep_dev.h) launches over the tiles of a Phi.  Plain C,
// shared by bc_sweep_grid (bc_core.hip) and a host harness (tests/sweep_plan_harness.c) that lets the tests place rows by the
// block, wave and grid stride that sweep them, without a GPU.
#ifndef BC_SWEEP_PLAN_H
#define BC_SWEEP_PLAN_H

#define BC_SWEEP_WAVES 4            /* waves per sweep block: one 128-row tile per wave and grid stride */

/* Memory-bound sweep, one wave per tile and a grid-stride loop.  FEWER resident waves stream better: at N = 10M, S = 100 one
 * 4-wave block per CU (each wave keeps 10 KiB in flight) reaches 0.886 of the HBM spec, two 0.873, four 0.857, eight 0.846
 * (profiles/r02_notes.md); a wave of a narrow Phi has fewer bytes per tile to keep in flight and needs company (S = 16: four
 * blocks per CU are best, one loses 40 %).  per_cu_override > 0 replaces the blocks per CU chosen by s. */
static inline int bc_sweep_plan(long long ntiles, int s, int n_cu, int per_cu_override) {
  long long per_cu = s >= 64 ? 1 : (s >= 24 ? 2 : 4);
  long long want, cap, g;
  if (per_cu_override > 0) per_cu = per_cu_override;
  want = (ntiles + BC_SWEEP_WAVES - 1) / BC_SWEEP_WAVES;
  cap = (long long)n_cu * per_cu;
  g = want < cap ? want : cap;
  return (int)(g < 1 ? 1 : g);
}

#endif /* BC_SWEEP_PLAN_H */
