// beta_cores_amd/csrc/bc_psvi_dev.h compiled for the host as a single "thread" (tid 0 of 1, one lane per "wave", empty barrier,
// reductions that are the identity): the text is the device's, so BatchPSVICoreset's point-gradient can be checked against the
// reference's expression without a GPU (tests/test_psvi_grad_cpu.py).  Files are raw doubles.
//   psvi_grad_harness IN OUT
//     IN : kind, m, s, d, dk, sigsq, then pts[m][dz], w[m], theta[s][dk], (kind 2: Siginv[d][d]), resid[s]
//          (dz = d + 1 for kind 0, d otherwise; theta is what K1's staging holds: zero-padded rows, Theta' for kind 2)
//     OUT: g_p[m][dz]
// Every input lives in an allocation of exactly its size, so a read past an end is seen by the sanitized build.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define BC_PSVI_FN
#define BC_PSVI_TID 0
#define BC_PSVI_NT 1
#define BC_PSVI_LANES 1
#define BC_PSVI_SYNC() ((void)0)
#define BC_PSVI_WAVE_SUM(v) (v)
#define BC_PSVI_BLOCK_SUM(v, red) ((void)(red), (v))
#include "../beta_cores_amd/csrc/bc_psvi_dev.h"

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
  if (!read_all(argv[1], &in) || in.size() < 6) return 2;
  const int kind = (int)in[0], m = (int)in[1], s = (int)in[2], d = (int)in[3], dk = (int)in[4];
  if (kind < BC_PSVI_LINREG || kind > BC_PSVI_GAUSS || m < 1 || s < 1 || d < 1 || dk < d) return 2;
  const int dz = d + (kind == BC_PSVI_LINREG ? 1 : 0);
  if (dz > BC_PSVI_MAX_DZ) return 2;
  const size_t n_pts = (size_t)m * dz, n_th = (size_t)s * dk, n_sg = kind == BC_PSVI_GAUSS ? (size_t)d * d : 0;
  if (in.size() != 6 + n_pts + m + n_th + n_sg + s) return 2;
  const double* p = in.data() + 6;
  const std::vector<double> pts(p, p + n_pts); p += n_pts;
  const std::vector<double> w(p, p + m); p += m;
  const std::vector<double> theta(p, p + n_th); p += n_th;
  const std::vector<double> siginv(p, p + n_sg); p += n_sg;
  const std::vector<double> resid(p, p + s);
  std::vector<double> out(n_pts, 7.0), ws(BC_PSVI_WS_DOUBLES(dz, s), 0.);
  PsviArgs a;
  memset(&a, 0, sizeof(a));
  a.kind = kind; a.m = m; a.s = s; a.d = d; a.dz = dz; a.dk = dk;
  a.pts = pts.data(); a.w = w.data(); a.theta = theta.data(); a.siginv = n_sg ? siginv.data() : nullptr;
  a.resid = resid.data(); a.sigsq = in[5]; a.out = out.data();
  for (int i = 0; i < m; ++i) bc_psvi_point_grad(a, i, ws.data());
  return write_all(argv[2], out) ? 0 : 2;
}
