// The host build of beta_cores_amd/csrc/bc_diag_dev.h: the chain summary of ONE problem by the library's own block functions, with
// tid = 0, nt = 1, one lane per wave and empty barriers.  Stand-alone (its own main): tests/diag_cases.py builds and runs it, once
// more under -fsanitize=address,undefined.
//   in : n C D max_lag staged | x [n][C][D]                (doubles)
//   out: status | mean [D] | cov [D][D] | W [D] | varplus [D] | rhat [D] | ess [D] | truncated [D] | rho [D][L + 1]
#define BC_DG_FN static
#define BC_DG_TID 0
#define BC_DG_NT 1
#define BC_DG_LANES 1
#define BC_DG_SYNC() do {} while (0)
#define BC_DG_WAVE_SUM(v) (v)
#define BC_DG_BLOCK_SUM(v, red) (v)
#include "../beta_cores_amd/csrc/bc_diag_dev.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define COV_CHUNK 2048      // BC_DIAG_COV_CHUNK of include/beta_cores_diag.h

static std::vector<double> read_all(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<double> v((size_t)bytes / sizeof(double));
  if (fread(v.data(), sizeof(double), v.size(), f) != v.size()) { fprintf(stderr, "short read\n"); exit(2); }
  fclose(f);
  return v;
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: diag_harness in.bin out.bin\n"); return 2; }
  const std::vector<double> in = read_all(argv[1]);
  const int n = (int)in[0], c = (int)in[1], d = (int)in[2];
  const long long max_lag = (long long)in[3];
  const bool staged = in[4] != 0.;
  if (in.size() != 5 + (size_t)n * c * d) { fprintf(stderr, "bad input size\n"); return 2; }
  const int h = n / 2, N = n * c, L = max_lag < h - 1 ? (int)max_lag : h - 1;
  // the retained layout [j][c][i]
  std::vector<double> keep((size_t)d * N);
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < c; ++k)
      for (int j = 0; j < d; ++j) keep[((size_t)j * c + k) * n + i] = in[5 + ((size_t)i * c + k) * d + j];
  std::vector<double> mean(d), cov((size_t)d * d), w(d), vp(d), rhat(d), ess(d), trunc(d), rho((size_t)d * (L + 1));
  std::vector<double> lds(BC_DG_WS_DOUBLES(c) + 2 * (size_t)c * h);
  int status = 0;
  for (int j = 0; j < d; ++j) {
    const double* x = keep.data() + (size_t)j * N;
    const DgWs W = bc_dg_ws(lds.data(), c, staged);
    if (bc_dg_mean(x, N, W.red, &mean[j])) status = 1;
    if (staged) bc_dg_stage(x, n, c, lds.data() + BC_DG_WS_DOUBLES(c));
    double o[3];
    int tr;
    bc_dg_moments(x, n, c, W, o);
    bc_dg_ess(x, n, c, max_lag, W, o, rho.data() + (size_t)j * (L + 1), &ess[j], &tr);
    w[j] = o[0], vp[j] = o[1], rhat[j] = o[2], trunc[j] = tr;
  }
  const int chunks = (N + COV_CHUNK - 1) / COV_CHUNK, T = bc_dg_tiles(d);
  std::vector<double> part((size_t)chunks * T * BC_DG_TILE_DOUBLES);
  for (int ch = 0; ch < chunks; ++ch) {
    const int r0 = ch * COV_CHUNK, r1 = r0 + COV_CHUNK < N ? r0 + COV_CHUNK : N;
    bc_dg_cov_chunk_host(keep.data(), mean.data(), d, N, r0, r1, part.data() + (size_t)ch * T * BC_DG_TILE_DOUBLES);
  }
  for (int a = 0; a < d; ++a)
    for (int b = 0; b < d; ++b) cov[(size_t)a * d + b] = bc_dg_cov_entry(part.data(), chunks, d, a, b, N);
  FILE* f = fopen(argv[2], "wb");
  if (!f) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
  const double st = status;
  fwrite(&st, sizeof(double), 1, f);
  for (const std::vector<double>* v : {&mean, &cov, &w, &vp, &rhat, &ess, &trunc, &rho}) fwrite(v->data(), sizeof(double), v->size(), f);
  fclose(f);
  return 0;
}
