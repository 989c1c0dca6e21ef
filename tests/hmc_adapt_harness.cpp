// Host build of csrc/bc_hmc_adapt_dev.h (the per-chain warm-up) behind csrc/bc_hmc_small_dev.h (the in-block rows pass) and
// csrc/bc_hmc_dev.h (the leapfrog and accept arithmetic), chained per (problem, chain) as k_hmc_small<CPB, 1> chains them in one
// slot: W warm-up iterations by the plan, then K kept iterations at the chain's frozen step and mass, on draws shared by all problems.
//   hmc_adapt_harness in.bin out.bin
// in:  P, D, C, L, W, K, delta, log10 | row_ptr [P + 1] | Z [sum n][D] | w [sum n] | start [P][C][D] | inv_mass [P][D] | log_step [P] |
//      plan [W][4] = eta | sg | zeta | flags | E [W + K][C][D] | logU [W + K][C]                                          (doubles)
// out: status [P] (0; 1 = a chain's log-joint or gradient at the start is not finite: that problem's outputs stay 0) |
//      samples [P][W + K][C][D] | logjoint [P][W + K][C] | accept [P][W + K][C] | step [P][W][C] | alpha [P][W][C] |
//      mass after every window end [P][ends][C][D] | frozen step [P][C] | frozen mass [P][C][D]
// Every region of the slot's work space is a vector of exactly the size the device lays out, so a sanitized build sees any
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
#include "../beta_cores_amd/csrc/bc_hmc_adapt_dev.h"

typedef std::vector<double> vec;

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  double head[8];
  if (fread(head, sizeof(double), 8, f) != 8) return 2;
  const int P = (int)head[0], d = (int)head[1], c = (int)head[2], L = (int)head[3], W = (int)head[4], K = (int)head[5], T = W + K;
  const double delta = head[6], log10 = head[7];
  if (P < 1 || d < 1 || d > BC_HMC_MAX_DIM || c < 1 || c > BC_HMC_MAX_CHAINS || L < 1 || W < 1 || K < 0) return 2;
  auto rd = [&](vec& v) { return v.empty() || fread(v.data(), sizeof(double), v.size(), f) == v.size(); };
  vec ptr((size_t)P + 1);
  if (!rd(ptr)) return 2;
  for (int p = 0; p < P; ++p)
    if (ptr[p + 1] - ptr[p] < 1.) return 2;
  const size_t n_all = (size_t)ptr[P];
  vec z(n_all * d), w(n_all), start((size_t)P * c * d), im_all((size_t)P * d), ls_all((size_t)P), plan((size_t)W * 4), E((size_t)T * c * d),
      U((size_t)T * c);
  if (!rd(z) || !rd(w) || !rd(start) || !rd(im_all) || !rd(ls_all) || !rd(plan) || !rd(E) || !rd(U)) return 2;
  fclose(f);
  int ends = 0;
  for (int i = 0; i < W; ++i) ends += ((int)plan[4 * (size_t)i + 3] & BC_HMC_ADAPT_WEND) != 0;
  const double hdl = 0.5 * d * log(2. * M_PI);
  const int ld = BC_HMC_SMALL_LD(d);
  const size_t ptcd = (size_t)P * T * c * d, ptc = (size_t)P * T * c, pwc = (size_t)P * W * c, pecd = (size_t)P * ends * c * d;
  vec out((size_t)P + ptcd + 2 * ptc + 2 * pwc + pecd + (size_t)P * c + (size_t)P * c * d, 0.);
  double* o_s = out.data() + P;
  double* o_l = o_s + ptcd;
  double* o_a = o_l + ptc;
  double* o_st = o_a + ptc;
  double* o_al = o_st + pwc;
  double* o_ms = o_al + pwc;
  double* o_fs = o_ms + pecd;
  double* o_fm = o_fs + (size_t)P * c;
  for (int p = 0; p < P; ++p) {
    const size_t r0 = (size_t)ptr[p];
    const int n = (int)(ptr[p + 1] - ptr[p]);
    vec zs((size_t)n * ld, 0.), ws_w(w.begin() + r0, w.begin() + r0 + n), wp((size_t)n), ll((size_t)n), part((size_t)BC_HMC_SMALL_NSEG(n) * (d + 1));
    if (zs.size() + ws_w.size() != BC_HMC_SMALL_ROWS_DOUBLES(n, d) || wp.size() + ll.size() + part.size() != BC_HMC_SMALL_CHAIN_DOUBLES(n, d)) return 3;
    for (int i = 0; i < n; ++i)
      for (int k = 0; k < d; ++k) zs[(size_t)i * ld + k] = z[(r0 + i) * d + k];
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
      const size_t b = (size_t)p * c + ch;
      // the chain's own state: its scalars, its inverse mass (in the slot's LDS on the device), its window sums (global memory there)
      bc_hmc_adapt_scalars st = {ls_all[p], 0., 0., log10 + ls_all[p], 0., 0.};
      vec im(im_all.begin() + (size_t)p * d, im_all.begin() + (size_t)(p + 1) * d), mean((size_t)d, 0.), m2((size_t)d, 0.);
      vec thp(d), r(d), gp(d);
      double ljp = 0., h0 = 0., eps = bc_hmc_adapt_exp(st.x);
      int we = 0;
      for (int t = 0; t < T; ++t) {
        if (t == W) eps = bc_hmc_adapt_exp(bc_hmc_adapt_frozen_log_step(st.x, st.xbar, st.t));
        const size_t tc = (size_t)t * c + ch;
        bc_hmc_start_chain(th[ch].data(), &lj[ch], g[ch].data(), &E[tc * d], im.data(), eps, d, r.data(), thp.data(), &h0, ws.data());
        for (int l = 1; l <= L; ++l) {
          bc_hmc_small_rows_pass(zs.data(), ws_w.data(), n, d, thp.data(), l == L, wp.data(), ll.data(), part.data(), red.data());
          if (l < L) bc_hmc_inner_chain(red.data(), eps, im.data(), d, r.data(), thp.data());
        }
        const int acc = bc_hmc_last_chain(red.data(), eps, im.data(), d, hdl, &h0, U[tc], r.data(), thp.data(), gp.data(), &ljp, th[ch].data(),
                                          &lj[ch], g[ch].data(), ws.data());
        const size_t o = (size_t)p * T * c + tc;
        for (int k = 0; k < d; ++k) o_s[o * d + k] = th[ch][k];
        o_l[o] = lj[ch];
        o_a[o] = acc;
        if (t >= W) continue;
        // the adaptation stage, as the kernel has it
        const double* pl = &plan[4 * (size_t)t];
        const int fl = (int)pl[3];
        st.t += 1.;
        const double alpha = bc_hmc_adapt_alpha(ws[2 * (size_t)d + 1]);
        const size_t ow = ((size_t)p * W + t) * c + ch;
        o_st[ow] = eps;
        o_al[ow] = alpha;
        bc_hmc_adapt_step_size(alpha, delta, pl[0], pl[1], pl[2], &st);
        if (fl & BC_HMC_ADAPT_FOLD) {
          st.nw += 1.;
          bc_hmc_adapt_fold(th[ch].data(), d, st.nw, mean.data(), m2.data());
        }
        if (fl & BC_HMC_ADAPT_WEND) {
          bc_hmc_adapt_window_end(d, st.nw, mean.data(), m2.data(), im.data());
          st.t = st.nw = 0.;
          bc_hmc_adapt_restart(log10, &st);
          for (int k = 0; k < d; ++k) o_ms[(((size_t)p * ends + we) * c + ch) * d + k] = im[k];
          ++we;
        }
        eps = bc_hmc_adapt_exp(st.x);
      }
      o_fs[b] = T > W ? eps : bc_hmc_adapt_exp(bc_hmc_adapt_frozen_log_step(st.x, st.xbar, st.t));
      for (int k = 0; k < d; ++k) o_fm[b * d + k] = im[k];
    }
  }
  f = fopen(argv[2], "wb");
  if (!f) return 2;
  if (fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 2;
  fclose(f);
  return 0;
}
