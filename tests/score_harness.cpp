// Host build of csrc/bc_score_dev.h (the arithmetic of k_lr_score that does not need the matrix cores), walked the way a wave
// walks it: per theta the four lane groups h = 0 .. 3, each over the tiles of 16 rows in ascending order with its rows
// h, h + 4, h + 8, h + 12, combined at the end.  The contraction is bc_score_dot, the host's stand-in for the MFMA chain.
//   score_harness in.bin out.bin
// in:  Nt, D, T | Z [Nt][D] | y [Nt] | theta [T][D]      (doubles)
// out: correct [T] | ll [T]                              (doubles)
// Exit status 2: the shape is outside the limits (1 <= D <= BC_HMC_MAX_DIM, Nt >= 1, T >= 1) or the file is short.
// A tile is staged as the kernel stages it -- 16 rows of the padded length, zero-filled -- in a vector of exactly that size, so a
// sanitized build sees any index past it.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define BC_SCORE_FN static
#include "../beta_cores_amd/csrc/bc_score_dev.h"
#include "../include/beta_cores_hmc.h"      // BC_HMC_MAX_DIM

typedef std::vector<double> vec;

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  double head[3];
  if (fread(head, sizeof(double), 3, f) != 3) return 2;
  const long long nt = (long long)head[0], T = (long long)head[2];
  const int d = (int)head[1];
  if (nt < 1 || d < 1 || d > BC_HMC_MAX_DIM || T < 1) return 2;
  auto rd = [&](vec& v) { return fread(v.data(), sizeof(double), v.size(), f) == v.size(); };
  vec z((size_t)nt * d), y((size_t)nt), th((size_t)T * d);
  if (!rd(z) || !rd(y) || !rd(th)) return 2;
  fclose(f);
  const int kp = BC_SCORE_KPAD(d);
  vec out((size_t)2 * T, 0.);
  vec tile((size_t)BC_SCORE_TILE * kp), ty((size_t)BC_SCORE_TILE), thp((size_t)kp);
  for (long long t = 0; t < T; ++t) {
    for (int k = 0; k < kp; ++k) thp[k] = k < d ? th[(size_t)t * d + k] : 0.;
    double acc[4] = {0., 0., 0., 0.};
    int cnt[4] = {0, 0, 0, 0};
    for (long long r0 = 0; r0 < nt; r0 += BC_SCORE_TILE) {
      for (int i = 0; i < BC_SCORE_TILE; ++i) {
        const long long gr = r0 + i;
        for (int k = 0; k < kp; ++k) tile[(size_t)i * kp + k] = (gr < nt && k < d) ? z[(size_t)gr * d + k] : 0.;
        ty[i] = gr < nt ? y[gr] : 0.;
      }
      for (int h = 0; h < 4; ++h) {
        double s[4], yy[4];
        for (int reg = 0; reg < 4; ++reg) {
          s[reg] = bc_score_dot(&tile[(size_t)(h + 4 * reg) * kp], thp.data(), kp);
          yy[reg] = ty[h + 4 * reg];
        }
        bc_score_lane_tile(s, yy, r0, h, nt, &acc[h], &cnt[h]);
      }
    }
    out[t] = (double)(cnt[0] + cnt[1] + cnt[2] + cnt[3]);
    out[T + t] = bc_score_combine(acc[0], acc[1], acc[2], acc[3]);
  }
  f = fopen(argv[2], "wb");
  if (!f) return 2;
  if (fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 2;
  fclose(f);
  return 0;
}
