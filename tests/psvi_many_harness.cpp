// One full step of the batched BatchPSVI run for ONE problem, stages 2-5 of include/beta_cores_psvi_many.h, with the device
// functions compiled for the host as a single "thread" (tid 0 of 1, empty barriers), called in the order the kernels of
// csrc/bc_psvi_many.hip call them: bc_pm_fit and the draw of bc_vi_laplace_dev.h, bc_pm_ll_tile over the tiles of the gathered rows
// (column sums) and of the points (stored), bc_pm_resid, bc_psvi_point_grad per point, bc_pm_adam.  Files are raw doubles.
//   psvi_many_harness IN OUT
//     IN : d, m, s, diag, n_sub, scale, step, c1, c2, then pts[m][d], w[m], start[d], E[s][d], rows[n_sub][d], mom1_w[m],
//          mom1_p[m][d], mom2_w[m], mom2_p[m][d]
//     OUT: status | mode[d] | theta[s][d] | target[s] | resid[s] | gw[m] | gp[m][d] | w[m] | pts[m][d] | mom1_w | mom1_p | mom2_w | mom2_p
//          status: 0, or the stage that marked the problem (1 fit, 2 residual, 3 ADAM); what the stages behind it would have
//          written keeps the 7.0 it was filled with (the state and the moments: their input values)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define BC_VIL_FN
#define BC_VIL_TID 0
#define BC_VIL_NT 1
#define BC_VIL_SYNC() ((void)0)
#include "../beta_cores_amd/csrc/bc_vi_laplace_dev.h"
#define BC_PSVI_FN
#define BC_PSVI_TID 0
#define BC_PSVI_NT 1
#define BC_PSVI_LANES 1
#define BC_PSVI_SYNC() ((void)0)
#define BC_PSVI_WAVE_SUM(v) (v)
#define BC_PSVI_BLOCK_SUM(v, red) ((void)(red), (v))
#include "../beta_cores_amd/csrc/bc_psvi_dev.h"
#define BC_PM_FN
#define BC_PM_TID 0
#define BC_PM_NT 1
#define BC_PM_SYNC() ((void)0)
#define BC_PM_ANY(x) (x)
#include "../beta_cores_amd/csrc/bc_psvi_many_dev.h"

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
  if (!read_all(argv[1], &in) || in.size() < 9) return 2;
  const int d = (int)in[0], m = (int)in[1], s = (int)in[2], diag = (int)in[3], n_sub = (int)in[4];
  const double scale = in[5], step = in[6], c1 = in[7], c2 = in[8];
  if (d < 1 || d > BC_VIL_MAXD || m < 1 || s < 1 || n_sub < 1) return 2;
  const size_t md = (size_t)m * d, sd = (size_t)s * d;
  if (in.size() != 9 + md + m + d + sd + (size_t)n_sub * d + 2 * (m + md)) return 2;
  const double* p = in.data() + 9;
  std::vector<double> pts(p, p + md); p += md;
  std::vector<double> w(p, p + m); p += m;
  std::vector<double> mode(p, p + d); p += d;
  std::vector<double> E(p, p + sd); p += sd;
  std::vector<double> rows(p, p + (size_t)n_sub * d); p += (size_t)n_sub * d;
  std::vector<double> m1w(p, p + m); p += m;
  std::vector<double> m1p(p, p + md); p += md;
  std::vector<double> m2w(p, p + m); p += m;
  std::vector<double> m2p(p, p + md);
  const int tiles = (n_sub + BC_PM_TILE - 1) / BC_PM_TILE, pt_tiles = (m + BC_PM_TILE - 1) / BC_PM_TILE;
  std::vector<double> theta(sd, 7.0), target(s, 7.0), resid(s, 7.0), gw(m, 7.0), gp(md, 7.0);
  std::vector<double> rowc(BC_VIL_ROW_DOUBLES(m), 0.), ws(BC_VIL_WS_DOUBLES(d), 0.), tile(BC_PM_TILE_DOUBLES(s), 0.);
  std::vector<double> part((size_t)tiles * s, 0.), cv((size_t)m * s, 0.), pg(BC_PSVI_WS_DOUBLES(d, s), 0.);
  int status = 0;
  // ---- stage 2: fit and draw (k_pm_fit)
  VilArgs a;
  memset(&a, 0, sizeof(a));
  a.d = d; a.m = m; a.dz = d; a.s = s; a.dk = d; a.diag = diag;
  a.core = pts.data(); a.w = w.data(); a.E = E.data(); a.theta = theta.data(); a.mode = mode.data(); a.rowc = rowc.data();
  const VilWs W = bc_vil_ws(ws.data(), d);
  VilFit fit;
  if (bc_pm_fit(a, W, &fit)) status = 1;
  if (!status) {
    bc_vil_draw(a, W);
    for (int j = 0; j < d; ++j) mode[j] = W.mu[j];
    // ---- stage 3 and the corevecs (k_pm_ll)
    PmTileArgs t;
    t.d = d; t.s = s; t.theta = theta.data();
    t.rows = rows.data(); t.elem = 8; t.n = n_sub;
    for (int y = 0; y < tiles; ++y) {
      bc_pm_ll_tile(t, y, tile.data());
      bc_pm_tile_colsum(t, y, tile.data(), part.data() + (size_t)y * s);
    }
    t.rows = pts.data(); t.n = m;
    for (int y = 0; y < pt_tiles; ++y) {
      bc_pm_ll_tile(t, y, tile.data());
      bc_pm_tile_store(t, y, tile.data(), cv.data());
    }
    // ---- stage 4 (k_pm_resid, k_pm_pgrad)
    PmResidArgs r;
    r.m = m; r.s = s; r.tiles = tiles; r.scale = scale; r.part = part.data(); r.cv = cv.data(); r.w = w.data();
    r.target = target.data(); r.resid = resid.data(); r.gw = gw.data();
    if (bc_pm_resid(r)) status = 2;
  }
  if (!status) {
    PsviArgs g;
    memset(&g, 0, sizeof(g));
    g.kind = BC_PSVI_LOGISTIC; g.m = m; g.s = s; g.d = d; g.dz = d; g.dk = d;
    g.pts = pts.data(); g.w = w.data(); g.theta = theta.data(); g.resid = resid.data(); g.sigsq = 1.; g.out = gp.data();
    for (int i = 0; i < m; ++i) bc_psvi_point_grad(g, i, pg.data());
    // ---- stage 5 (k_pm_adam)
    PmAdamArgs o;
    o.m = m; o.d = d; o.gw = gw.data(); o.gp = gp.data(); o.w = w.data(); o.pts = pts.data();
    o.m1w = m1w.data(); o.m1p = m1p.data(); o.m2w = m2w.data(); o.m2p = m2p.data();
    o.step = step; o.c1 = c1; o.c2 = c2;
    if (bc_pm_adam(o)) status = 3;
  }
  std::vector<double> out;
  out.push_back((double)status);
  for (const std::vector<double>* v : {&mode, &theta, &target, &resid, &gw, &gp, &w, &pts, &m1w, &m1p, &m2w, &m2p}) out.insert(out.end(), v->begin(), v->end());
  return write_all(argv[2], out) ? 0 : 2;
}
