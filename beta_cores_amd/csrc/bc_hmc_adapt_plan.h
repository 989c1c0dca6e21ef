/* The window plan of the per-chain warm-up of the batched small-problem HMC run (include/beta_cores_hmc_adapt.h): which warm-up
 * iterations fold the position into the running variance, which end a window, and the three coefficients of the dual-averaging
 * step of each.  Plain C, host only; the library exports it as bc_hmc_adapt_plan, so Python and the tests read the schedule
 * from there instead of restating it.
 *
 * The rule is Stan's windowed_adaptation.  With W = n_warmup iterations, numbered i = 0 .. W - 1:
 *   W < 20: no windows at all (only the step is adapted).
 *   init + term + base > W:  init = floor(0.15 W), term = floor(0.1 W), base = W - init - term.
 *   Iteration i folds iff init <= i < W - term.
 *   The first window ends with iteration init + base - 1.  At a window end that is not iteration W - term - 1 the window size
 *   doubles and the next end is (this end) + size; if the window after THAT one (of twice the size again) would reach W - term,
 *   the next end is W - term - 1 instead: the last window is stretched to the end of the slow phase.
 * E.g. W = 1000 with 75 / 50 / 25: windows end after 100, 150, 250, 450 and 950 iterations.
 *
 * The dual-averaging counter t restarts at every window end, so it is a function of i alone: t(i) = 1 + the iterations since the
 * last window end before i (or since the start).  Per iteration the plan holds
 *   eta = 1 / (t + t0)      sg = sqrt(t) / gamma      zeta = t^-kappa
 * each evaluated in long double and rounded once -- the device evaluates no transcendental but exp (csrc/bc_hmc_adapt_dev.h). */
#ifndef BC_HMC_ADAPT_PLAN_H
#define BC_HMC_ADAPT_PLAN_H

#include <math.h>
#include <stdint.h>

#define BC_HMC_ADAPT_FOLD 1 /* the position after this iteration is folded into the running mean and M2 */
#define BC_HMC_ADAPT_WEND 2 /* this iteration ends a window: new inverse mass, the step's averaging restarts */
#define BC_HMC_ADAPT_MIN_WINDOWED 20

/* out_flags [W], out_coef [W][3] = eta | sg | zeta.  Returns 0, or 1 for arguments outside the rule's domain (nothing is written):
 * W >= 0, the buffers >= 0, base >= 1, gamma > 0, t0 >= 0, kappa > 0, all finite.  W = 0 writes nothing and returns 0. */
static inline int bc_hmc_adapt_plan_fill(int32_t n_warmup, int32_t init_buffer, int32_t term_buffer, int32_t base_window, double gamma,
                                         double t0, double kappa, int32_t* out_flags, double* out_coef) {
  if (n_warmup < 0 || init_buffer < 0 || term_buffer < 0 || base_window < 1) return 1;
  if (!(gamma > 0.) || !(t0 >= 0.) || !(kappa > 0.) || !(gamma < INFINITY) || !(t0 < INFINITY) || !(kappa < INFINITY)) return 1;
  const int64_t W = n_warmup;
  int64_t init = init_buffer, term = term_buffer, base = base_window;
  const int windowed = W >= BC_HMC_ADAPT_MIN_WINDOWED;
  if (windowed && init + term + base > W) {
    init = (int64_t)(0.15 * (double)W);
    term = (int64_t)(0.1 * (double)W);
    base = W - init - term;
  }
  const int64_t slow_end = W - term; /* the first iteration of the terminal buffer */
  int64_t next_end = init + base - 1, size = base, t = 0;
  for (int64_t i = 0; i < W; ++i) {
    int32_t fl = 0;
    if (windowed && i >= init && i < slow_end) fl |= BC_HMC_ADAPT_FOLD;
    ++t;
    out_coef[3 * i] = (double)(1.0L / ((long double)t + (long double)t0));
    out_coef[3 * i + 1] = (double)(sqrtl((long double)t) / (long double)gamma);
    out_coef[3 * i + 2] = (double)powl((long double)t, -(long double)kappa);
    if (windowed && i == next_end) {
      fl |= BC_HMC_ADAPT_WEND;
      t = 0;
      if (next_end != slow_end - 1) {
        size *= 2;
        next_end = i + size;
        if (next_end != slow_end - 1 && next_end + 2 * size >= slow_end) next_end = slow_end - 1;
      } else {
        next_end = -1; /* the slow phase is over */
      }
    }
    out_flags[i] = fl;
  }
  return 0;
}

#endif /* BC_HMC_ADAPT_PLAN_H */
