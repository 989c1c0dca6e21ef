// Host build of csrc/bc_predict_dev.h (the arithmetic and every summation order of k_linreg_predict that does not need the matrix
// cores), walked the way the kernel walks it: per posterior the blocks of BC_PRED_ROWS_PER_BLOCK rows, per block the staged chunks
// of BC_PRED_STAGE_ROWS(D) rows, per row the eight chains of the mean, the lanes' sums of squares over their waves' column groups,
// the butterfly over a row's 16 lanes and the sum over the waves, then the one-thread-per-staged-row sums, the butterfly over the
// block's threads and the combine stage over the blocks.  The contraction is bc_predict_dot, the stand-in for the MFMA chain.
//   predict_harness in.bin out.bin
// in:  Nt, D, T, per_row | Z [Nt][D + 1] | mu [T][D] | F [T][D][D] | noise [T] | scale [T]      (doubles)
// out: ll [T] | sse [T] | with per_row: mean [T][Nt] | var [T][Nt]                             (doubles)
// Exit status 2: the shape is outside the limits (1 <= D <= BC_PRED_MAX_DIM, Nt >= 1, T >= 1) or the file is short.
// Every staged array has exactly the size the kernel gives it, so a sanitized build sees any index past it.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define BC_PREDICT_FN static
#include "../beta_cores_amd/csrc/bc_predict_dev.h"

typedef std::vector<double> vec;

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  double head[4];
  if (fread(head, sizeof(double), 4, f) != 4) return 2;
  const long long nt = (long long)head[0], T = (long long)head[2];
  const int d = (int)head[1];
  const bool per_row = head[3] != 0.;
  if (nt < 1 || d < 1 || d > BC_PRED_MAX_DIM || T < 1) return 2;
  auto rd = [&](vec& v) { return fread(v.data(), sizeof(double), v.size(), f) == v.size(); };
  vec z((size_t)nt * (d + 1)), mu((size_t)T * d), fac((size_t)T * d * d), noise((size_t)T), scale((size_t)T);
  if (!rd(z) || !rd(mu) || !rd(fac) || !rd(noise) || !rd(scale)) return 2;
  fclose(f);
  const int rc = BC_PRED_STAGE_ROWS(d), groups = BC_PRED_GROUPS(d), dcols = BC_PRED_TILE * groups;
  const long long chunks = (nt + BC_PRED_ROWS_PER_BLOCK - 1) / BC_PRED_ROWS_PER_BLOCK;
  vec out((size_t)2 * T + (per_row ? (size_t)2 * T * nt : 0), 0.);
  vec phi((size_t)d), v((size_t)dcols), qw((size_t)BC_PRED_WAVES), part((size_t)chunks * 2);
  for (long long t = 0; t < T; ++t) {
    const double* F = &fac[(size_t)t * d * d];
    const double* m = &mu[(size_t)t * d];
    for (long long c = 0; c < chunks; ++c) {
      const long long row0 = c * BC_PRED_ROWS_PER_BLOCK, row1 = row0 + BC_PRED_ROWS_PER_BLOCK < nt ? row0 + BC_PRED_ROWS_PER_BLOCK : nt;
      double acc_ll[64], acc_sse[64];
      for (int i = 0; i < 64; ++i) acc_ll[i] = acc_sse[i] = 0.;
      for (long long c0 = row0; c0 < row1; c0 += rc) {
        for (int i = 0; i < rc && c0 + i < row1; ++i) {
          const long long n = c0 + i;
          for (int k = 0; k < d; ++k) phi[k] = z[(size_t)n * (d + 1) + k];
          double parts[BC_PRED_MEAN_PARTS];
          for (int p = 0; p < BC_PRED_MEAN_PARTS; ++p) parts[p] = bc_predict_mean_part(phi.data(), m, d, p);
          const double mean = bc_predict_tree(parts, BC_PRED_MEAN_PARTS);
          for (int j = 0; j < dcols; ++j) v[j] = bc_predict_dot(phi.data(), F, d, j);
          for (int w = 0; w < BC_PRED_WAVES; ++w) {
            double lanes[BC_PRED_TILE];
            for (int col = 0; col < BC_PRED_TILE; ++col) lanes[col] = bc_predict_lane_q(v.data(), groups, w, col);
            qw[w] = bc_predict_tree(lanes, BC_PRED_TILE);
          }
          const double q = bc_predict_wave_q(qw.data(), 1);
          double var, r2;
          const double term = bc_predict_row(z[(size_t)n * (d + 1) + d], mean, q, noise[t], scale[t], &var, &r2);
          acc_ll[i] += term;
          acc_sse[i] += r2;
          if (per_row) {
            out[(size_t)2 * T + (size_t)t * nt + n] = mean;
            out[(size_t)2 * T + (size_t)T * nt + (size_t)t * nt + n] = var;
          }
        }
      }
      part[2 * c] = bc_predict_tree(acc_ll, 64);
      part[2 * c + 1] = bc_predict_tree(acc_sse, 64);
    }
    bc_predict_chunks(part.data(), chunks, &out[t], &out[T + t]);
  }
  f = fopen(argv[2], "wb");
  if (!f) return 2;
  if (fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 2;
  fclose(f);
  return 0;
}
