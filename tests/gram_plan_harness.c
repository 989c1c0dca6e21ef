/* Host access to beta_cores_amd/csrc/bc_gram_plan.h, the header run_gram (bc_gram.hip) cuts the rows of a weighted Gram into
 * splits with.  Reads lines "n_rows ntri n_cu slots waves kr" from standard input and prints "rows_per_split splits nruns" for
 * each, after checking what the kernels rely on: rows_per_split is a positive multiple of kr, the splits cover the rows with
 * none of them empty, and the runs cover the splits.  Exit status 0 when every line was read and held. */
#include <stdio.h>
#include "bc_gram_plan.h"

int main(void) {
  long long n, rps, splits, nruns;
  int ntri, n_cu, slots, waves, kr, got;
  while ((got = scanf("%lld %d %d %d %d %d", &n, &ntri, &n_cu, &slots, &waves, &kr)) == 6) {
    bc_gram_plan(n, ntri, n_cu, slots, waves, kr, &rps, &splits, &nruns);
    if (rps < kr || rps % kr || splits < 1 || splits * rps < n || (splits - 1) * rps >= n || nruns < 1 ||
        nruns * BC_GRAM_SEG < splits || (nruns - 1) * BC_GRAM_SEG >= splits) {
      printf("bad plan for %lld %d %d %d %d %d: %lld %lld %lld\n", n, ntri, n_cu, slots, waves, kr, rps, splits, nruns);
      return 1;
    }
    printf("%lld %lld %lld\n", rps, splits, nruns);
  }
  return got == EOF ? 0 : 2;
}
