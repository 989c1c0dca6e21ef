/* Host-side accuracy check of the two beta-gradient bodies of beta_cores_amd/csrc/bc_k1_math.h (bc_linreg_beta_grad_value,
 * bc_logistic_beta_grad_value: what K1 models 7 and 8 evaluate per element) against their closed forms in 80-bit long double
 * arithmetic.  Grid: m in [-1500, 1500] and q in [0, 1e4], dense near 0 and near the points where the bodies switch (the clamp
 * of the exp argument at -800, the bound of |m| for the log1p at 800, np.exp's overflow at 709.78, which the gradient ignores);
 * beta in {0.01, 0.1, 0.5, 2, 32}, sigsq in {0.3, 1, 2.5}.  Bar: absolute error <= 1e-13 * (1 + max|g| over the grid), per beta
 * (and per sigsq).  Prints the measured maxima; exit status 1 if the bar or a special value is missed.
 * Built and driven by tests/test_betagrad_cpu.py. */
#include <stdio.h>
#include <stdlib.h>
#include "bc_k1_math.h"

static long double logistic_ref(long double m, long double beta) {
  const long double ls = log1pl(expl(-fabsl(m)));
  const long double a = (m > 0 ? m : 0) + ls, b = (m < 0 ? -m : 0) + ls;
  return expl(-beta * a) / (beta * beta) + (beta + 1) / beta * a * expl(-beta * a) - a * expl(-(beta + 1) * a) - b * expl(-(beta + 1) * b);
}

static long double linreg_ref(long double q, long double beta, long double sigsq) {
  const long double L = logl(2 * 3.14159265358979323846264338327950288L * sigsq), C = expl(-beta * L / 2);
  const long double E = expl(-beta * q / (2 * sigsq));
  const long double f = C * (-(beta + 1) / beta * E + 1 / sqrtl(1 + beta));
  return -(L / 2) * f + C * (E / (beta * beta) + (beta + 1) / beta * q / (2 * sigsq) * E - powl(1 + beta, -1.5L) / 2);
}

/* the grid of one signed axis [-hi, hi] (or [0, hi]): a uniform sweep, geometric points towards 0, and clusters around `marks` */
static int fill_grid(double* g, int cap, double hi, int two_sided, const double* marks, int nmarks) {
  int n = 0;
  for (int i = 0; i <= 3000 && n < cap; ++i) g[n++] = (two_sided ? -hi : 0.) + (two_sided ? 2. : 1.) * hi * i / 3000.;
  for (double v = hi; v > 1e-12 && n + 2 <= cap; v *= 0.93) { g[n++] = v; if (two_sided) g[n++] = -v; }
  for (int k = 0; k < nmarks; ++k)
    for (int i = -40; i <= 40 && n + 2 <= cap; ++i) {
      const double v = marks[k] * (1. + i * 2.5e-4) + i * 1e-9;
      if (v >= 0. && v <= hi) { g[n++] = v; if (two_sided) g[n++] = -v; }
    }
  g[n++] = 0.;
  return n;
}

int main(void) {
  const unsigned long long tabbits[BC_K1_TAB_DOUBLES] = BC_K1_TABLE_INIT;
  double tab[BC_K1_TAB_DOUBLES];
  memcpy(tab, tabbits, sizeof(tab));
  static double grid[8192];
  const double betas[5] = {0.01, 0.1, 0.5, 2., 32.};
  const double sigs[3] = {0.3, 1., 2.5};
  int bad = 0;
  double worst_log = 0., worst_lin = 0.;      /* error / (1 + max|g|), the quantity the bar is on */

  for (int bi = 0; bi < 5; ++bi) {
    const double beta = betas[bi];
    /* ---- logistic */
    {
      const double marks[6] = {800., 709.782712893384, 745., 800. / beta > 1500. ? 1499. : 800. / beta, 800. / (beta + 1.), 36.7};
      const int n = fill_grid(grid, 8192, 1500., 1, marks, 6);
      double k[4];
      bc_logistic_beta_grad_consts(beta, k);
      long double gmax = 0;
      for (int i = 0; i < n; ++i) { const long double r = fabsl(logistic_ref(grid[i], beta)); if (r > gmax) gmax = r; }
      double emax = 0., at = 0.;
      for (int i = 0; i < n; ++i) {
        const double got = bc_logistic_beta_grad_value(grid[i], k[0], k[1], k[2], k[3], tab);
        const double err = (double)fabsl((long double)got - logistic_ref(grid[i], beta));
        if (!(err <= emax)) { emax = err; at = grid[i]; }
      }
      const double rel = emax / (1. + (double)gmax);
      printf("logistic beta %-5g: max|g| %.6g  max abs err %.3g (at m = %.17g)  err/(1+max|g|) %.3g\n", beta, (double)gmax, emax, at, rel);
      if (!(rel <= 1e-13)) bad = 1;
      if (rel > worst_log) worst_log = rel;
      /* limits: exactly 1/beta^2 once m << 0 has saturated, exactly 0 far out on the other side, finite in between, NaN kept */
      if (bc_logistic_beta_grad_value(-1500., k[0], k[1], k[2], k[3], tab) != k[0] || bc_logistic_beta_grad_value(-800., k[0], k[1], k[2], k[3], tab) != k[0] ||
          bc_logistic_beta_grad_value(-120., k[0], k[1], k[2], k[3], tab) != k[0]) { printf("logistic m << 0 limit BAD at beta %g\n", beta); bad = 1; }
      if (bc_logistic_beta_grad_value(1e6, k[0], k[1], k[2], k[3], tab) != 0. || bc_logistic_beta_grad_value(1e300, k[0], k[1], k[2], k[3], tab) != 0.) {
        printf("logistic m >> 0 limit BAD at beta %g\n", beta); bad = 1; }
      if (!isfinite(bc_logistic_beta_grad_value(-1e300, k[0], k[1], k[2], k[3], tab)) || !isfinite(bc_logistic_beta_grad_value(709.79, k[0], k[1], k[2], k[3], tab))) {
        printf("logistic not finite at beta %g\n", beta); bad = 1; }
      if (!isnan(bc_logistic_beta_grad_value(NAN, k[0], k[1], k[2], k[3], tab))) { printf("logistic NaN BAD at beta %g\n", beta); bad = 1; }
    }
    /* ---- linear regression */
    for (int si = 0; si < 3; ++si) {
      const double sigsq = sigs[si];
      double k[4];
      bc_linreg_beta_grad_consts(sigsq, beta, k);
      const double marks[3] = {800. / -k[2], 1. / -k[2], 36.7 / -k[2]};
      const int n = fill_grid(grid, 8192, 1e4, 0, marks, 3);
      long double gmax = 0;
      for (int i = 0; i < n; ++i) { const long double r = fabsl(linreg_ref(grid[i], beta, sigsq)); if (r > gmax) gmax = r; }
      double emax = 0., at = 0.;
      for (int i = 0; i < n; ++i) {
        const double got = bc_linreg_beta_grad_value(grid[i], k[0], k[1], k[2], k[3], tab);
        const double err = (double)fabsl((long double)got - linreg_ref(grid[i], beta, sigsq));
        if (!(err <= emax)) { emax = err; at = grid[i]; }
      }
      const double rel = emax / (1. + (double)gmax);
      printf("linreg beta %-5g sigsq %-4g: max|g| %.6g  max abs err %.3g (at q = %.17g)  err/(1+max|g|) %.3g\n", beta, sigsq, (double)gmax, emax, at, rel);
      if (!(rel <= 1e-13)) bad = 1;
      if (rel > worst_lin) worst_lin = rel;
      if (!isnan(bc_linreg_beta_grad_value(NAN, k[0], k[1], k[2], k[3], tab))) { printf("linreg NaN BAD\n"); bad = 1; }
      if (bc_linreg_beta_grad_value(1e300, k[0], k[1], k[2], k[3], tab) != -k[3]) { printf("linreg q >> 0 limit BAD\n"); bad = 1; }
    }
  }
  printf("betagrad: logistic worst %.3g linreg worst %.3g of the bar's unit (1 + max|g|); bar 1e-13 %s\n", worst_log, worst_lin, bad ? "MISSED" : "ok");
  return bad;
}
