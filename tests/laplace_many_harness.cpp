// The four stages of beta_cores_amd/csrc/bc_vi_laplace_dev.h compiled for the host as a single "thread" (tid 0 of 1, empty
// barrier) and run over a PACKED BATCH the way k_laplace_many (csrc/bc_laplace_small.hip) runs them, one problem after the
// other: mode search, H at the mode (its diagonal is taken before the factorisation overwrites it), factor and inverse, draw.
// What the kernel stores per problem is written out, so the split functions can be held to the long-double reference without a
// GPU (tests/test_laplace_many_cpu.py).  Files are raw doubles.
//   laplace_many_harness IN OUT
//     IN : d, P, s, diag, shared (1: one E for all problems), then row_ptr[P + 1], rows[sum n][d], w[sum n], start[P][d],
//          E[s][d] (shared) or E[P][s][d]
//     OUT: per problem a block of 1 + d + 1 + d + 2 d d + 3 + s d doubles:
//          status | mu[d] | value | hdiag[d] | chol[d][d] | inv[d][d] | counts[3] | draws[s][d]
//          (status != 0: the rest of the block keeps the 7.0 it was filled with; diag: chol and inv keep it too)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define BC_VIL_FN
#define BC_VIL_TID 0
#define BC_VIL_NT 1
#define BC_VIL_SYNC() ((void)0)
#include "../beta_cores_amd/csrc/bc_vi_laplace_dev.h"

static bool read_all(const char* path, std::vector<double>* out) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  out->resize((size_t)bytes / sizeof(double));
  const bool ok = fread(out->data(), sizeof(double), out->size(), f) == out->size();
  fclose(f);
  return ok;
}

static bool write_all(const char* path, const std::vector<double>& v) {
  FILE* f = fopen(path, "wb");
  if (!f) return false;
  const bool ok = fwrite(v.data(), sizeof(double), v.size(), f) == v.size();
  return fclose(f) == 0 && ok;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::vector<double> in;
  if (!read_all(argv[1], &in) || in.size() < 5) return 2;
  const int d = (int)in[0], P = (int)in[1], s = (int)in[2], diag = (int)in[3], shared = (int)in[4];
  if (d < 1 || d > BC_VIL_MAXD || P < 1 || s < 0) return 2;
  if (in.size() < 5 + (size_t)P + 1) return 2;
  std::vector<long> row_ptr(P + 1);
  for (int p = 0; p <= P; ++p) row_ptr[p] = (long)in[5 + p];
  if (row_ptr[0] != 0) return 2;
  for (int p = 0; p < P; ++p)
    if (row_ptr[p + 1] <= row_ptr[p]) return 2;
  const size_t n_all = (size_t)row_ptr[P], sd = (size_t)s * d;
  if (in.size() != 5 + (size_t)P + 1 + n_all * d + n_all + (size_t)P * d + (shared ? sd : P * sd)) return 2;
  const double* rows = in.data() + 5 + P + 1;
  const double* w = rows + n_all * d;
  const double* start = w + n_all;
  const double* E = start + (size_t)P * d;
  const size_t block = 1 + d + 1 + d + 2 * (size_t)d * d + 3 + sd;
  std::vector<double> out((size_t)P * block, 7.0), rowc(BC_VIL_ROW_DOUBLES(n_all), 0.), ws(BC_VIL_WS_DOUBLES(d), 0.);
  for (int p = 0; p < P; ++p) {
    double* o = out.data() + (size_t)p * block;
    double *o_mu = o + 1, *o_val = o_mu + d, *o_hd = o_val + 1, *o_chol = o_hd + d, *o_inv = o_chol + (size_t)d * d;
    double *o_cnt = o_inv + (size_t)d * d, *o_th = o_cnt + 3;
    std::vector<double> mode(start + (size_t)p * d, start + (size_t)(p + 1) * d), hd(d);
    VilArgs a;
    memset(&a, 0, sizeof(a));
    a.d = d; a.m = (int)(row_ptr[p + 1] - row_ptr[p]); a.dz = d; a.s = s; a.dk = d; a.diag = diag;
    a.core = rows + (size_t)row_ptr[p] * d;
    a.w = w + row_ptr[p];
    a.E = E + (shared ? 0 : (size_t)p * sd);
    a.theta = o_th;
    a.mode = mode.data();
    a.rowc = rowc.data() + 3 * (size_t)row_ptr[p];
    a.counts = nullptr;
    const VilWs W = bc_vil_ws(ws.data(), d);
    VilFit fit;
    int bad = bc_vil_mode(a, W, &fit);
    if (!bad) {
      bc_vil_hessian(a, W);
      for (int j = 0; j < d; ++j) hd[j] = W.A[bc_vil_tri(j, j)];
      bad = bc_vil_factor(a, W);
    }
    o[0] = (double)bad;
    if (bad) continue;
    bc_vil_draw(a, W);
    for (int j = 0; j < d; ++j) { o_mu[j] = W.mu[j]; o_hd[j] = hd[j]; }
    *o_val = fit.f;
    if (!diag)
      for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j) {
          o_chol[(size_t)i * d + j] = j <= i ? W.A[bc_vil_tri(i, j)] : 0.;
          o_inv[(size_t)i * d + j] = j <= i ? W.Li[bc_vil_tri(i, j)] : 0.;
        }
    o_cnt[0] = fit.steps; o_cnt[1] = fit.halvings; o_cnt[2] = fit.halvings_all;
  }
  return write_all(argv[2], out) ? 0 : 2;
}
