// bc_gram_plan.h -- how run_gram (bc_gram.hip) cuts the rows of a weighted Gram into splits: the rows per split, the number
// of splits (one block per split and tile, one partial tile each) and the number of runs the first reduction level adds them
// in.  Plain C, shared by the launch code and a host harness (tests/gram_plan_harness.c) that lets the tests pick row counts
// by the split count they produce, without a GPU.
#ifndef BC_GRAM_PLAN_H
#define BC_GRAM_PLAN_H

#define BC_GRAM_SEG 16              /* splits per run of k_gram_reduce1 */

/* Row splits, in units of the n_cu * slots resident block slots times `waves` rounds, shared among the ntri tiles, and at
 * least 2 slabs of kr rows per split; rows_per_split is a multiple of kr, and the last split holds what is left
 * (1 .. rows_per_split rows).  n_rows >= 1, ntri >= 1, kr >= 1. */
static inline void bc_gram_plan(long long n_rows, int ntri, int n_cu, int slots, int waves, int kr, long long* rows_per_split,
                                long long* splits_out, long long* nruns) {
  const long long want_splits = ((long long)n_cu * slots * (waves > 0 ? waves : 1) + ntri - 1) / ntri;
  const long long max_splits = (n_rows + 2 * kr - 1) / (2 * kr);
  long long splits = want_splits < max_splits ? want_splits : max_splits;
  long long rps;
  if (splits < 1) splits = 1;
  rps = (n_rows + splits - 1) / splits;
  rps = ((rps + kr - 1) / kr) * kr;
  if (rps < kr) rps = kr;
  splits = (n_rows + rps - 1) / rps;
  if (splits < 1) splits = 1;
  *rows_per_split = rps;
  *splits_out = splits;
  *nruns = (splits + BC_GRAM_SEG - 1) / BC_GRAM_SEG;
}

#endif /* BC_GRAM_PLAN_H */
