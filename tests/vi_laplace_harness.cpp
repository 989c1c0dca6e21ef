// beta_cores_amd/csrc/bc_vi_laplace_dev.h compiled for the host as a single "thread" (tid 0 of 1, empty barrier): the text is
// the device's but for the parts under __HIPCC__, whose plain loops stand in here, so the logistic Laplace sampler can be
// checked against a long-double reference without a GPU (tests/test_vi_laplace_cpu.py).  Files are raw doubles.
//   vi_laplace_harness IN OUT
//     IN : d, m, s, diag, then core[m][d], w[m], start[d], E[s][d]
//     OUT: status, then (status 0) theta[s][dk] with dk = d + 3 (the padding keeps the 7.0 it was filled with), mode[d],
//          the decrement of the last Newton system, counts[4]
//          (status != 0: then 1.0 if theta, mode and counts are all as they were filled, else 0.0)
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
  std::vector<double> in, out;
  if (!read_all(argv[1], &in) || in.size() < 4) return 2;
  const int d = (int)in[0], m = (int)in[1], s = (int)in[2], diag = (int)in[3];
  if (d < 1 || d > BC_VIL_MAXD || m < 1 || s < 1) return 2;
  if (in.size() != 4 + (size_t)m * d + m + d + (size_t)s * d) return 2;
  const int dk = d + 3;
  const double* p = in.data() + 4;
  VilArgs a;
  memset(&a, 0, sizeof(a));
  a.d = d; a.m = m; a.dz = d; a.s = s; a.dk = dk; a.diag = diag;
  a.core = p; p += (size_t)m * d;
  a.w = p; p += m;
  std::vector<double> mode(p, p + d);
  mode.push_back(-1.);
  const std::vector<double> mode0 = mode;
  p += d;
  a.E = p;
  std::vector<double> theta((size_t)s * dk, 7.0), rowc(BC_VIL_ROW_DOUBLES(m), 0.), ws(BC_VIL_WS_DOUBLES(d), 0.);
  int counts[4] = {-1, -1, 0, -1};
  a.theta = theta.data();
  a.mode = mode.data();
  a.rowc = rowc.data();
  a.counts = counts;
  const int status = bc_vi_laplace(a, ws.data());
  out.push_back((double)status);
  if (status == 0) {
    out.insert(out.end(), theta.begin(), theta.end());
    out.insert(out.end(), mode.begin(), mode.end());
    for (int c : counts) out.push_back((double)c);
  } else {
    bool same = counts[0] == -1 && counts[1] == -1 && counts[2] == 0 && counts[3] == -1 && memcmp(mode.data(), mode0.data(), mode.size() * sizeof(double)) == 0;
    for (double x : theta) same = same && x == 7.0;
    out.push_back(same ? 1. : 0.);
  }
  return write_all(argv[2], out) ? 0 : 2;
}
