// Host build of csrc/bc_hmc_small_dev.h (the in-block rows pass) and csrc/bc_hmc_dev.h (the leapfrog and accept arithmetic),
// chained per (problem, chain) as k_hmc_small chains them in one block, on draws shared by all problems.
//   hmc_small_harness in.bin out.bin
// in:  P, D, C, L, T | row_ptr [P + 1] | Z [sum n][D] | w [sum n] | start [P][C][D] | inv_mass [P][D] | eps [P] | E [T][C][D] |
//      logU [T][C]                                                                                                    (doubles)
// out: status [P] (0; 1 = a chain's log-joint or gradient at the start is not finite: that problem's outputs stay 0) |
//      samples [P][T][C][D] | logjoint [P][T][C] | accept [P][T][C]
// Every region of the block's work space is a vector of exactly the size the device lays out, so a sanitized build sees any
// index past a region's end.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define BC_HMC_FN static
#define BC_HMC_TID 0
#define BC_HMC_NT 1
#define BC_HMC_SYNC() do { } while (0)
#include "../beta_cores_amd/csrc/bc_hmc_dev.h"
#include "../beta_cores_amd/csrc/bc_hmc_small_dev.h"

typedef std::vector<double> vec;

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  double head[5];
  if (fread(head, sizeof(double), 5, f) != 5) return 2;
  const int P = (int)head[0], d = (int)head[1], c = (int)head[2], L = (int)head[3], T = (int)head[4];
  if (P < 1 || d < 1 || d > BC_HMC_MAX_DIM || c < 1 || c > BC_HMC_MAX_CHAINS || L < 1 || T < 1) return 2;
  auto rd = [&](vec& v) { return v.empty() || fread(v.data(), sizeof(double), v.size(), f) == v.size(); };
  vec ptr((size_t)P + 1);
  if (!rd(ptr)) return 2;
  for (int p = 0; p < P; ++p)
    if (ptr[p + 1] - ptr[p] < 1.) return 2;
  const size_t n_all = (size_t)ptr[P];
  vec z(n_all * d), w(n_all), start((size_t)P * c * d), im_all((size_t)P * d), eps_all((size_t)P), E((size_t)T * c * d), U((size_t)T * c);
  if (!rd(z) || !rd(w) || !rd(start) || !rd(im_all) || !rd(eps_all) || !rd(E) || !rd(U)) return 2;
  fclose(f);
  const double hdl = 0.5 * d * log(2. * M_PI);
  const int ld = BC_HMC_SMALL_LD(d);
  const size_t ptcd = (size_t)P * T * c * d, ptc = (size_t)P * T * c;
  vec out((size_t)P + ptcd + 2 * ptc, 0.);
  double* o_s = out.data() + P;
  double* o_l = o_s + ptcd;
  double* o_a = o_l + ptc;
  for (int p = 0; p < P; ++p) {
    const size_t r0 = (size_t)ptr[p];
    const int n = (int)(ptr[p + 1] - ptr[p]);
    // the block's work space, laid out as k_hmc_small lays it out (one vector per region)
    vec zs((size_t)n * ld, 0.), ws_w(w.begin() + r0, w.begin() + r0 + n), wp((size_t)n), ll((size_t)n), part((size_t)BC_HMC_SMALL_NSEG(n) * (d + 1));
    if (zs.size() + ws_w.size() != BC_HMC_SMALL_ROWS_DOUBLES(n, d) || wp.size() + ll.size() + part.size() != BC_HMC_SMALL_CHAIN_DOUBLES(n, d)) return 3;
    for (int i = 0; i < n; ++i)
      for (int k = 0; k < d; ++k) zs[(size_t)i * ld + k] = z[(r0 + i) * d + k];
    const double* im = &im_all[(size_t)p * d];
    const double eps = eps_all[p];
    // the start pass of every chain first: a problem with one bad chain is marked as a whole
    std::vector<vec> th(c, vec(d)), g(c, vec(d));
    vec lj(c);
    vec red((size_t)1 + d, 0.), ws((size_t)BC_HMC_WS_DOUBLES(d));
    int bad = 0;
    for (int ch = 0; ch < c; ++ch) {
      for (int k = 0; k < d; ++k) th[ch][k] = start[((size_t)p * c + ch) * d + k];
      bc_hmc_small_rows_pass(zs.data(), ws_w.data(), n, d, th[ch].data(), 1, wp.data(), ll.data(), part.data(), red.data());
      bad |= bc_hmc_logjoint_chain(red.data(), th[ch].data(), d, hdl, &lj[ch], g[ch].data(), ws.data());
    }
    if (bad) {
      out[p] = 1.;
      continue;
    }
    for (int ch = 0; ch < c; ++ch) {
      vec thp(d), r(d), gp(d);
      double ljp = 0., h0 = 0.;
      for (int t = 0; t < T; ++t) {
        const size_t tc = (size_t)t * c + ch;
        bc_hmc_start_chain(th[ch].data(), &lj[ch], g[ch].data(), &E[tc * d], im, eps, d, r.data(), thp.data(), &h0, ws.data());
        for (int l = 1; l <= L; ++l) {
          bc_hmc_small_rows_pass(zs.data(), ws_w.data(), n, d, thp.data(), l == L, wp.data(), ll.data(), part.data(), red.data());
          if (l < L) bc_hmc_inner_chain(red.data(), eps, im, d, r.data(), thp.data());
        }
        const int acc = bc_hmc_last_chain(red.data(), eps, im, d, hdl, &h0, U[tc], r.data(), thp.data(), gp.data(), &ljp, th[ch].data(), &lj[ch],
                                          g[ch].data(), ws.data());
        const size_t o = (size_t)p * T * c + tc;
        for (int k = 0; k < d; ++k) o_s[o * d + k] = th[ch][k];
        o_l[o] = lj[ch];
        o_a[o] = acc;
      }
    }
  }
  f = fopen(argv[2], "wb");
  if (!f) return 2;
  if (fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 2;
  fclose(f);
  return 0;
}
