// The block-wide NNLS of beta_cores_amd/csrc/bc_nnls_dev.h compiled for the host as a single "thread" (tid 0 of 1, empty
// barrier): the algorithm's text is the device's, so its logic can be checked against SciPy without a GPU
// (tests/test_nnls_cpu.py).  Input (binary doubles): n, s, enter, all, then cols[n][s], b[s], val[n].
// Output (text): status, refits, solves, rejected, then the n weights in %.17g.
#include <cstdio>
#include <cstdlib>
#include <vector>

#define BC_NNLS_FN
#define BC_NNLS_TID 0
#define BC_NNLS_NT 1
#define BC_NNLS_SYNC() ((void)0)
#include "../beta_cores_amd/csrc/bc_nnls_dev.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  double hdr[4];
  if (fread(hdr, sizeof(double), 4, f) != 4) return 2;
  const int n = (int)hdr[0], s = (int)hdr[1], enter = (int)hdr[2], all = (int)hdr[3];
  if (n < 0 || n > BC_NNLS_MAXP || s < 1) return 2;
  std::vector<double> cols((size_t)n * s), b(s), val(n);
  if (fread(cols.data(), sizeof(double), cols.size(), f) != cols.size()) return 2;
  if (fread(b.data(), sizeof(double), b.size(), f) != b.size()) return 2;
  if (n && fread(val.data(), sizeof(double), val.size(), f) != val.size()) return 2;
  fclose(f);
  std::vector<double> G((size_t)BC_NNLS_MAXP * BC_NNLS_MAXP, 0.), c(BC_NNLS_MAXP, 0.), ws(BC_NNLS_WS_DOUBLES, 0.);
  // the Gram state grows the way the step kernel grows it: a first block of rows, then one row at a time
  const int half = n / 2;
  bc_nnls_gram_rows(cols.data(), s, b.data(), G.data(), c.data(), half, 0, half);
  for (int i = half; i < n; ++i) bc_nnls_gram_rows(cols.data(), s, b.data(), G.data(), c.data(), i + 1, i, i + 1);
  double bn = 0.;
  for (int k = 0; k < s; ++k) bn += b[k] * b[k];
  long long stats[3] = {0, 0, 0};
  const int status = bc_nnls_solve(G.data(), c.data(), n, val.data(), enter, all, sqrt(bn), bc_nnls_ws(ws.data()), stats);
  printf("%d %lld %lld %lld\n", status, stats[0], stats[1], stats[2]);
  for (int j = 0; j < n; ++j) printf("%.17g\n", val[j]);
  return 0;
}
