// Host build of csrc/bc_hmc_dev.h: the leapfrog and accept arithmetic of the multi-chain HMC run, chained as
// bc_hmc_chunk_begin chains the device kernels, around a plain C++ rows pass.
//   hmc_harness in.bin out.bin
// in:  n, D, C, L, T, eps | Z [n][D] | w [n] | start [C][D] | inv_mass [D] | E [T][C][D] | logU [T][C]      (doubles)
// out: status (0; 1 = the start's log-joint or gradient is not finite) | samples [T][C][D] | logjoint [T][C] | accept [T][C]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define BC_HMC_FN static
#define BC_HMC_TID 0
#define BC_HMC_NT 1
#define BC_HMC_SYNC() do { } while (0)
#include "../beta_cores_amd/csrc/bc_hmc_dev.h"

// value | grad [d] of the weighted likelihood at one theta (lr_terms of csrc/bc_lr_terms.h, restated for the host)
static void rows_pass(const double* z, const double* w, long n, int d, const double* th, double* red) {
  for (int k = 0; k <= d; ++k) red[k] = 0.;
  for (long i = 0; i < n; ++i) {
    double s = 0.;
    for (int k = 0; k < d; ++k) s = fma(z[i * d + k], th[k], s);
    const double m = -s;
    double ll, p;
    if (m < 100.) {
      const double e = exp(-fabs(m)), ope = 1. + e;
      ll = -(fmax(m, 0.) + log1p(e));
      p = m >= 0. ? 1. / ope : e / ope;
    } else {
      ll = -m;
      p = 1.;
    }
    red[0] = fma(w[i], ll, red[0]);
    const double wp = w[i] * p;
    for (int k = 0; k < d; ++k) red[1 + k] = fma(wp, z[i * d + k], red[1 + k]);
  }
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  double head[6];
  if (fread(head, sizeof(double), 6, f) != 6) return 2;
  const long n = (long)head[0];
  const int d = (int)head[1], c = (int)head[2], L = (int)head[3], T = (int)head[4];
  const double eps = head[5];
  if (n < 0 || d < 1 || d > BC_HMC_MAX_DIM || c < 1 || c > BC_HMC_MAX_CHAINS || L < 1 || T < 1) return 2;
  std::vector<double> z((size_t)n * d), w((size_t)n), th((size_t)c * d), im((size_t)d), E((size_t)T * c * d), U((size_t)T * c);
  auto rd = [&](std::vector<double>& v) { return v.empty() || fread(v.data(), sizeof(double), v.size(), f) == v.size(); };
  if (!rd(z) || !rd(w) || !rd(th) || !rd(im) || !rd(E) || !rd(U)) return 2;
  fclose(f);
  const double hdl = 0.5 * d * log(2. * M_PI);
  std::vector<double> thp((size_t)c * d), r((size_t)c * d), g((size_t)c * d), gp((size_t)c * d), lj((size_t)c), ljp((size_t)c), h0((size_t)c), red((size_t)1 + d);
  std::vector<double> ws((size_t)BC_HMC_WS_DOUBLES(d));
  std::vector<double> out(1, 0.);
  int bad = 0;
  for (int ch = 0; ch < c; ++ch) {
    rows_pass(z.data(), w.data(), n, d, &th[(size_t)ch * d], red.data());
    bad |= bc_hmc_logjoint_chain(red.data(), &th[(size_t)ch * d], d, hdl, &lj[ch], &g[(size_t)ch * d], ws.data());
  }
  if (bad) {
    out[0] = 1.;
  } else {
    out.resize(1 + (size_t)T * c * d + 2 * (size_t)T * c);
    double* o_s = out.data() + 1;
    double* o_l = o_s + (size_t)T * c * d;
    double* o_a = o_l + (size_t)T * c;
    for (int t = 0; t < T; ++t) {
      for (int ch = 0; ch < c; ++ch) {
        const size_t o = (size_t)ch * d;
        bc_hmc_start_chain(&th[o], &lj[ch], &g[o], &E[((size_t)t * c + ch) * d], im.data(), eps, d, &r[o], &thp[o], &h0[ch], ws.data());
        for (int l = 1; l <= L; ++l) {
          rows_pass(z.data(), w.data(), n, d, &thp[o], red.data());
          if (l < L) bc_hmc_inner_chain(red.data(), eps, im.data(), d, &r[o], &thp[o]);
        }
        const int acc = bc_hmc_last_chain(red.data(), eps, im.data(), d, hdl, &h0[ch], U[(size_t)t * c + ch], &r[o], &thp[o], &gp[o], &ljp[ch],
                                          &th[o], &lj[ch], &g[o], ws.data());
        for (int k = 0; k < d; ++k) o_s[((size_t)t * c + ch) * d + k] = th[o + k];
        o_l[(size_t)t * c + ch] = lj[ch];
        o_a[(size_t)t * c + ch] = acc;
      }
    }
  }
  f = fopen(argv[2], "wb");
  if (!f) return 2;
  if (fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 2;
  fclose(f);
  return 0;
}
