// beta_cores_amd/csrc/bc_vi_sampler_dev.h compiled for the host as a single "thread" (tid 0 of 1, empty barrier): the text is
// the device's, so the posterior draw and the ADAM body can be checked against the oracle without a GPU
// (tests/test_vi_sampler_cpu.py).  Files are raw doubles.
//   vi_sampler_harness sampler IN OUT
//     IN : kind, d, m, s, then core[m][dz], w[m], Sig0inv[d][d], th0[d], (kind 0: sigsq | kind 1: Siginv[d][d]), E[s][d]
//          (b0 = Sig0inv . th0 is formed here by bc_vi_prior_rhs, the function bc_vi_optimize_begin calls)
//     OUT: status, then (status 0) theta[s][dk] with dk = d + 3 (the padding keeps the 7.0 it was filled with), saux[s], raw[s][d]
//   vi_sampler_harness adam IN OUT
//     IN : m, itrs, q[m], c[m], x0[m], step[3][itrs]          gradient of the separable quadratic: g = q * x - c
//     OUT: x after every step, [itrs][m]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define BC_VIS_FN
#define BC_VIS_TID 0
#define BC_VIS_NT 1
#define BC_VIS_SYNC() ((void)0)
#include "../beta_cores_amd/csrc/bc_vi_sampler_dev.h"

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

static int run_sampler(const std::vector<double>& in, std::vector<double>* out) {
  if (in.size() < 4) return 2;
  const int kind = (int)in[0], d = (int)in[1], m = (int)in[2], s = (int)in[3];
  if ((kind != BC_VIS_LINREG && kind != BC_VIS_GAUSS) || d < 1 || d > BC_VIS_MAXD || m < 1 || s < 1) return 2;
  const int dz = d + (kind == BC_VIS_LINREG ? 1 : 0), dk = d + 3;
  const size_t dd = (size_t)d * d;
  const size_t need = 4 + (size_t)m * dz + m + dd + d + (kind == BC_VIS_GAUSS ? dd : 1) + (size_t)s * d;
  if (in.size() != need) return 2;
  const double* p = in.data() + 4;
  VisArgs a;
  memset(&a, 0, sizeof(a));
  a.kind = kind; a.d = d; a.m = m; a.dz = dz; a.s = s; a.dk = dk;
  a.core = p; p += (size_t)m * dz;
  a.w = p; p += m;
  a.sig0inv = p; p += dd;
  std::vector<double> b0(d, 0.);
  bc_vi_prior_rhs(a.sig0inv, p, d, b0.data()); p += d;
  a.b0 = b0.data();
  if (kind == BC_VIS_GAUSS) { a.siginv = p; p += dd; } else { a.sigsq = *p; p += 1; }
  a.E = p;
  std::vector<double> theta((size_t)s * dk, 7.0), saux(s, 0.), raw((size_t)s * d, 0.), ws(BC_VIS_WS_DOUBLES(d), 0.);
  a.theta = theta.data();
  a.saux = saux.data();
  a.raw = raw.data();
  const int status = bc_vi_sampler(a, ws.data());
  out->push_back((double)status);
  if (status == 0) {
    out->insert(out->end(), theta.begin(), theta.end());
    out->insert(out->end(), saux.begin(), saux.end());
    out->insert(out->end(), raw.begin(), raw.end());
  }
  return 0;
}

static int run_adam(const std::vector<double>& in, std::vector<double>* out) {
  if (in.size() < 2) return 2;
  const int m = (int)in[0], itrs = (int)in[1];
  if (m < 1 || itrs < 1 || in.size() != 2 + 3 * (size_t)m + 3 * (size_t)itrs) return 2;
  const double* q = in.data() + 2;
  const double* c = q + m;
  const double* step = c + 2 * (size_t)m;
  std::vector<double> x(c + m, c + 2 * (size_t)m), mom1(m, 0.), mom2(m, 0.);
  const double b1 = 0.9, b2 = 0.999, eps = 1e-8;
  for (int i = 0; i < itrs; ++i) {
    for (int j = 0; j < m; ++j) {
      const double g = q[j] * x[j] - c[j];
      bc_vi_adam_elem(g, &x[j], &mom1[j], &mom2[j], b1, 1. - b1, b2, 1. - b2, eps, step[i], step[itrs + i], step[2 * (size_t)itrs + i]);
    }
    out->insert(out->end(), x.begin(), x.end());
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  std::vector<double> in, out;
  if (!read_all(argv[2], &in)) return 2;
  int rc = 2;
  if (!strcmp(argv[1], "sampler")) rc = run_sampler(in, &out);
  else if (!strcmp(argv[1], "adam")) rc = run_adam(in, &out);
  if (rc) return rc;
  return write_all(argv[3], out) ? 0 : 2;
}
