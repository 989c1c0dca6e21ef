// One full step of the Gaussian-location kind of the batched BatchPSVI run for ONE problem (include/beta_cores_psvi_many.h), with
// the device functions compiled for the host as a single "thread" (tid 0 of 1, empty barriers), called in the order the kernels of
// csrc/bc_psvi_many.hip call them: bc_pm_rowaux_tile over the tiles of the gathered rows and of the points, bc_vi_sampler
// (BC_VIS_GAUSS; with no samples and bc_pm_post_products behind it unless `chains`), bc_pm_gauss_tile over the tiles of the
// gathered rows (column sums) and of the points (stored), bc_pm_resid, bc_psvi_point_grad (BC_PSVI_GAUSS) per point, bc_pm_adam.
// Files are raw doubles.
//   psvi_many_gauss_harness IN OUT
//     IN : d, m, s, n_sub, scale, step, c1, c2, logdet, chains (1: bc_vi_sampler's own products), then pts[m][d], w[m], mu0[d],
//          Sig0inv[d][d], Siginv[d][d], E[s][d], rows[n_sub][d], mom1_w[m], mom1_p[m][d], mom2_w[m], mom2_p[m][d]
//     OUT: status | mode[d] | theta[s][d] (the draw) | thp[s][d] (Theta') | sa[s] | ra_sub[n_sub] | ra_pts[m] | target[s] | resid[s] |
//          gw[m] | gp[m][d] | w[m] | pts[m][d] | mom1_w | mom1_p | mom2_w | mom2_p
//          status: 0, or the stage that marked the problem (1 posterior, 2 residual, 3 ADAM); what the stages behind it would have
//          written keeps the 7.0 it was filled with (the state and the moments: their input values)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define BC_VIS_FN
#define BC_VIS_TID 0
#define BC_VIS_NT 1
#define BC_VIS_SYNC() ((void)0)
#include "../beta_cores_amd/csrc/bc_vi_sampler_dev.h"
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
  if (!read_all(argv[1], &in) || in.size() < 10) return 2;
  const int d = (int)in[0], m = (int)in[1], s = (int)in[2], n_sub = (int)in[3];
  const double scale = in[4], step = in[5], c1 = in[6], c2 = in[7], logdet = in[8];
  const int chains = (int)in[9];
  if (d < 1 || d > BC_VIS_MAXD || m < 1 || s < 1 || n_sub < 1) return 2;
  const size_t md = (size_t)m * d, sd = (size_t)s * d, dd = (size_t)d * d;
  if (in.size() != 10 + md + m + d + 2 * dd + sd + (size_t)n_sub * d + 2 * (m + md)) return 2;
  const double* p = in.data() + 10;
  std::vector<double> pts(p, p + md); p += md;
  std::vector<double> w(p, p + m); p += m;
  std::vector<double> mu0(p, p + d); p += d;
  std::vector<double> sig0inv(p, p + dd); p += dd;
  std::vector<double> siginv(p, p + dd); p += dd;
  std::vector<double> E(p, p + sd); p += sd;
  std::vector<double> rows(p, p + (size_t)n_sub * d); p += (size_t)n_sub * d;
  std::vector<double> m1w(p, p + m); p += m;
  std::vector<double> m1p(p, p + md); p += md;
  std::vector<double> m2w(p, p + m); p += m;
  std::vector<double> m2p(p, p + md);
  const int tiles = (n_sub + BC_PM_TILE - 1) / BC_PM_TILE, pt_tiles = (m + BC_PM_TILE - 1) / BC_PM_TILE;
  std::vector<double> mode(d, 7.0), theta(sd, 7.0), thp(sd, 7.0), sa(s, 7.0), ra_sub(n_sub, 7.0), ra_pts(m, 7.0);
  std::vector<double> target(s, 7.0), resid(s, 7.0), gw(m, 7.0), gp(md, 7.0);
  std::vector<double> ws(BC_VIS_WS_DOUBLES(d), 0.), tile(BC_PM_TILE_DOUBLES(s), 0.), raws(BC_PM_ROWAUX_DOUBLES(d), 0.), b0(d, 0.);
  std::vector<double> part((size_t)tiles * s, 0.), cv((size_t)m * s, 0.), pg(BC_PSVI_WS_DOUBLES(d, s), 0.);
  // the model's constant as bc_proj_model_constants writes it (csrc/bc_project.hip)
  const double pi = 3.141592653589793;
  const double c0 = -(double)d / 2 * log(2 * pi) - 1. / 2. * logdet;
  int status = 0;
  // ---- the row aux (k_pm_rowaux)
  for (int y = 0; y < tiles; ++y) bc_pm_rowaux_tile(rows.data(), 8, n_sub, d, siginv.data(), y, raws.data(), ra_sub.data());
  for (int y = 0; y < pt_tiles; ++y) bc_pm_rowaux_tile(pts.data(), 8, m, d, siginv.data(), y, raws.data(), ra_pts.data());
  // ---- posterior and draw (k_pm_post)
  bc_vi_prior_rhs(sig0inv.data(), mu0.data(), d, b0.data());
  VisArgs a;
  memset(&a, 0, sizeof(a));
  a.kind = BC_VIS_GAUSS; a.d = d; a.m = m; a.dz = d; a.s = chains ? s : 0; a.dk = d;
  a.core = pts.data(); a.w = w.data(); a.sig0inv = sig0inv.data(); a.b0 = b0.data(); a.siginv = siginv.data(); a.sigsq = 1.;
  a.E = E.data(); a.theta = thp.data(); a.saux = sa.data(); a.raw = theta.data();
  if (bc_vi_sampler(a, ws.data())) status = 1;
  if (!status) {
    static_assert(BC_PM_VIS_DOUBLES(BC_VIS_MAXD) == BC_VIS_WS_DOUBLES(BC_VIS_MAXD), "the work-space layout bc_psvi_many_dev.h restates");
    const double* mu = ws.data() + BC_PM_VIS_MU(d);
    if (!chains) {
      PmPostArgs b;
      b.d = d; b.s = s; b.E = E.data(); b.Li = ws.data() + BC_PM_VIS_LI(d); b.mu = mu; b.siginv = siginv.data();
      b.raw = theta.data(); b.thp = thp.data(); b.sa = sa.data();
      bc_pm_post_products(b);
    }
    for (int j = 0; j < d; ++j) mode[j] = mu[j];
    // ---- target and corevecs (k_pm_ll)
    PmTileArgs t;
    memset(&t, 0, sizeof(t));
    t.d = d; t.s = s; t.theta = thp.data(); t.sa = sa.data(); t.c0 = c0;
    t.rows = rows.data(); t.elem = 8; t.n = n_sub; t.ra = ra_sub.data();
    for (int y = 0; y < tiles; ++y) {
      bc_pm_gauss_tile(t, y, tile.data());
      bc_pm_tile_colsum(t, y, tile.data(), part.data() + (size_t)y * s);
    }
    t.rows = pts.data(); t.n = m; t.ra = ra_pts.data();
    for (int y = 0; y < pt_tiles; ++y) {
      bc_pm_gauss_tile(t, y, tile.data());
      bc_pm_tile_store(t, y, tile.data(), cv.data());
    }
    // ---- residual, g_w (k_pm_resid)
    PmResidArgs r;
    r.m = m; r.s = s; r.tiles = tiles; r.scale = scale; r.part = part.data(); r.cv = cv.data(); r.w = w.data();
    r.target = target.data(); r.resid = resid.data(); r.gw = gw.data();
    if (bc_pm_resid(r)) status = 2;
  }
  if (!status) {
    // ---- point-gradient (k_pm_pgrad), ADAM (k_pm_adam)
    PsviArgs g;
    memset(&g, 0, sizeof(g));
    g.kind = BC_PSVI_GAUSS; g.m = m; g.s = s; g.d = d; g.dz = d; g.dk = d;
    g.pts = pts.data(); g.w = w.data(); g.theta = thp.data(); g.siginv = siginv.data(); g.resid = resid.data(); g.sigsq = 1.; g.out = gp.data();
    for (int i = 0; i < m; ++i) bc_psvi_point_grad(g, i, pg.data());
    PmAdamArgs o;
    o.m = m; o.d = d; o.gw = gw.data(); o.gp = gp.data(); o.w = w.data(); o.pts = pts.data();
    o.m1w = m1w.data(); o.m1p = m1p.data(); o.m2w = m2w.data(); o.m2p = m2p.data();
    o.step = step; o.c1 = c1; o.c2 = c2;
    if (bc_pm_adam(o)) status = 3;
  }
  std::vector<double> out;
  out.push_back((double)status);
  for (const std::vector<double>* v : {&mode, &theta, &thp, &sa, &ra_sub, &ra_pts, &target, &resid, &gw, &gp, &w, &pts, &m1w, &m1p, &m2w, &m2p})
    out.insert(out.end(), v->begin(), v->end());
  return write_all(argv[2], out) ? 0 : 2;
}
