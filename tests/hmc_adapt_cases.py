"""The NumPy restatement of the per-chain warm-up of the batched small-problem HMC run (include/beta_cores_hmc_adapt.h,
csrc/bc_hmc_adapt_dev.h) on top of hmc_cases.logjoint, parametrised by dtype (np.float64, or np.longdouble as the reference); the
cases the tests share; the two sharp recomputations (the step from a trace of alphas, a window's mass from its samples); a
NumPy stand-in engine for samplers.logistic_hmc_many(adapt='stan'); and the build of tests/hmc_adapt_harness.cpp.  The window
plan is NOT restated here: it is read from the library (bc_hmc_adapt_plan), as the product reads it.
Test infrastructure only: the product never imports this module."""
import ctypes
import functools
import os
import subprocess

import numpy as np

import hmc_cases as hc

ROOT = hc.ROOT
FOLD, WEND = 1, 2
STAN = dict(delta=0.8, gamma=0.05, t0=10., kappa=0.75)
LOG10 = float(np.log(10.))      # (the double the library's host side hands to the device)


# ------------------------------------------------------------------ the plan, from the library
def plan(n_warmup, init_buffer=75, term_buffer=50, base_window=25, gamma=0.05, t0=10., kappa=0.75):
    """(flags [W] int32, coef [W, 3] = eta | sqrt(t) / gamma | t^-kappa) of bc_hmc_adapt_plan; needs no device."""
    from beta_cores_amd import _native as N
    flags, coef = np.zeros(max(n_warmup, 1), dtype=np.int32), np.zeros((max(n_warmup, 1), 3))
    rc = N.load().bc_hmc_adapt_plan(int(n_warmup), int(init_buffer), int(term_buffer), int(base_window), float(gamma), float(t0), float(kappa),
                                    flags.ctypes.data_as(ctypes.c_void_p), coef.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, N.last_error()
    return flags[:n_warmup], coef[:n_warmup]


def window_ends(flags):
    """The 1-based iteration counts after which a window ends."""
    return [int(i) + 1 for i in np.nonzero(np.asarray(flags) & WEND)[0]]


# ------------------------------------------------------------------ the formulas
def alpha_of(dh):
    """alpha = 0 where dh = H0 - H1 is not finite, 1 where dh >= 0, exp(dh) otherwise and exactly 0 below -700."""
    with np.errstate(all='ignore'):
        fin = np.isfinite(dh)
        safe = np.where(fin & (dh < 0) & (dh >= -700), dh, 0)
        return np.where(~fin, 0, np.where(dh >= 0, 1, np.where(dh < -700, 0, np.exp(safe)))).astype(dh.dtype)


class AdaptRun:
    """One problem's chains with the warm-up state of csrc/bc_hmc_adapt_dev.h, advanced chunk by chunk.  warm(E, logU): the next
    warm-up iterations; kept(E, logU): kept iterations at the frozen state.  Both return a dict like hc.hmc_run's (samples, logjoint,
    accept, margin -- nan where H1 is not finite), warm() also step [k, C] (the step every iteration ran with), alpha [k, C] and
    masses: a list with the inverse masses [C, D] after every window end of the chunk."""

    def __init__(self, Z, w, start, inv_mass, log_step, n_leapfrog, flags, coef, delta=0.8, dtype=np.longdouble):
        self.Z, self.w, self.L, self.dtype, self.delta = Z, w, n_leapfrog, dtype, dtype(delta)
        self.flags, self.coef, self.i = np.asarray(flags), np.asarray(coef).astype(dtype), 0
        self.th = np.array(start).astype(dtype)
        C, D = self.th.shape
        self.im = np.tile(np.asarray(inv_mass).astype(dtype), (C, 1))
        self.x = np.full(C, dtype(log_step))
        self.mu = dtype(LOG10) + self.x
        self.xbar, self.hbar = np.zeros(C, dtype=dtype), np.zeros(C, dtype=dtype)
        self.t = self.nw = 0
        self.mean, self.m2 = np.zeros((C, D), dtype=dtype), np.zeros((C, D), dtype=dtype)
        self.lj, self.g = hc.logjoint(Z, w, self.th, dtype)

    def frozen(self):
        """(step [C], inverse mass [C, D]) of the kept iterations."""
        return np.exp(self.x if self.t == 0 else self.xbar), self.im

    def _iterate(self, eps, e, logu):
        dtype, im = self.dtype, self.im
        eps = eps[:, None]
        r = e.astype(dtype) / np.sqrt(im)
        h0 = -self.lj + (im * r * r).sum(axis=1) / 2
        r = r + eps / 2 * self.g
        thp = self.th + eps * (im * r)
        with np.errstate(all='ignore'):
            for l in range(1, self.L + 1):
                ljp, gp = hc.logjoint(self.Z, self.w, thp, dtype)
                if l < self.L:
                    r = r + eps * gp
                    thp = thp + eps * (im * r)
                else:
                    r = r + eps / 2 * gp
            h1 = -ljp + (im * r * r).sum(axis=1) / 2
            fin = np.isfinite(h1)
            dh = h0 - h1
            acc = np.logical_and(fin, logu.astype(dtype) < dh)
            margin = np.where(fin, logu.astype(dtype) - dh, np.nan).astype(np.float64)
        self.th = np.where(acc[:, None], thp, self.th)
        self.g = np.where(acc[:, None], gp, self.g)
        self.lj = np.where(acc, ljp, self.lj)
        return acc, margin, np.where(fin, dh, dtype(np.nan))

    def _chunk(self, E, logU, warm):
        k, C, D = E.shape
        dtype = self.dtype
        out = dict(samples=np.empty((k, C, D), dtype=dtype), logjoint=np.empty((k, C), dtype=dtype), accept=np.zeros((k, C), dtype=bool),
                   margin=np.full((k, C), np.nan))
        if warm:
            out.update(step=np.empty((k, C), dtype=dtype), alpha=np.empty((k, C), dtype=dtype), masses=[])
        else:
            eps = self.frozen()[0]
        for j in range(k):
            if warm:
                eps = np.exp(self.x)
            acc, margin, dh = self._iterate(eps, E[j], logU[j])
            out['samples'][j], out['logjoint'][j], out['accept'][j], out['margin'][j] = self.th, self.lj, acc, margin
            if not warm:
                continue
            assert self.i < len(self.flags), 'more warm-up iterations than planned'
            fl, (eta, sg, zeta) = int(self.flags[self.i]), self.coef[self.i]
            alpha = alpha_of(dh)
            out['step'][j], out['alpha'][j] = eps, alpha
            self.t += 1
            self.hbar = (1 - eta) * self.hbar + eta * (self.delta - alpha)
            self.x = self.mu - self.hbar * sg
            self.xbar = (1 - zeta) * self.xbar + zeta * self.x
            if fl & FOLD:
                self.nw += 1
                dk = self.th - self.mean
                self.mean = self.mean + dk / dtype(self.nw)
                self.m2 = self.m2 + dk * (self.th - self.mean)
            if fl & WEND:
                if self.nw >= 2:
                    self.im = window_mass(self.m2, self.nw, dtype)
                out['masses'].append(self.im.copy())
                self.mean, self.m2, self.nw = np.zeros_like(self.mean), np.zeros_like(self.m2), 0
                self.mu = dtype(LOG10) + self.x
                self.hbar, self.xbar, self.t = np.zeros_like(self.hbar), np.zeros_like(self.xbar), 0
            self.i += 1
        return out

    def warm(self, E, logU):
        return self._chunk(E, logU, True)

    def kept(self, E, logU):
        return self._chunk(E, logU, False)


def window_mass(m2, nw, dtype):
    nw = dtype(nw)
    return (nw / (nw + 5)) * (m2 / (nw - 1)) + dtype(1e-3) * (5 / (nw + 5))


def adapt_trace(case, dtype=np.longdouble):
    """A whole case: the warm-up in one chunk, then the kept iterations.  Returns (warm dict, kept dict or None, frozen step, mass)."""
    W = len(case['flags'])
    run = AdaptRun(case['Z'], case['w'], case['start'], case['inv_mass'], case['log_step'], case['L'], case['flags'], case['coef'],
                   case['delta'], dtype)
    warm = run.warm(case['E'][:W], case['logU'][:W])
    step, im = run.frozen()
    kept = run.kept(case['E'][W:], case['logU'][W:]) if case['E'].shape[0] > W else None
    return warm, kept, step, im.copy()


# ------------------------------------------------------------------ the two sharp recomputations
def step_from_alphas(alpha, flags, coef, log_step, delta, dtype=np.longdouble):
    """The step trace [W, C] and the frozen step [C] of the dual-averaging recurrence ALONE, from a given trace of alphas [W, C]."""
    alpha, coef = np.asarray(alpha).astype(dtype), np.asarray(coef).astype(dtype)
    W, C = alpha.shape
    x = np.full(C, dtype(log_step))
    mu, xbar, hbar, t = dtype(LOG10) + x, np.zeros(C, dtype=dtype), np.zeros(C, dtype=dtype), 0
    steps = np.empty((W, C), dtype=dtype)
    for i in range(W):
        steps[i] = np.exp(x)
        eta, sg, zeta = coef[i]
        t += 1
        hbar = (1 - eta) * hbar + eta * (dtype(delta) - alpha[i])
        x = mu - hbar * sg
        xbar = (1 - zeta) * xbar + zeta * x
        if int(flags[i]) & WEND:
            mu, hbar, xbar, t = dtype(LOG10) + x, np.zeros_like(hbar), np.zeros_like(xbar), 0
    return steps, np.exp(x if t == 0 else xbar)


def masses_from_samples(samples, flags, inv_mass, dtype=np.longdouble):
    """The inverse masses [C, D] after every window end, by Welford's recurrence ALONE over a given trace of positions [W, C, D]."""
    s = np.asarray(samples).astype(dtype)
    W, C, D = s.shape
    im = np.tile(np.asarray(inv_mass).astype(dtype), (C, 1))
    mean, m2, nw, out = np.zeros((C, D), dtype=dtype), np.zeros((C, D), dtype=dtype), 0, []
    for i in range(W):
        if int(flags[i]) & FOLD:
            nw += 1
            dk = s[i] - mean
            mean = mean + dk / dtype(nw)
            m2 = m2 + dk * (s[i] - mean)
        if int(flags[i]) & WEND:
            if nw >= 2:
                im = window_mass(m2, nw, dtype)
            out.append(im.copy())
            mean, m2, nw = np.zeros_like(mean), np.zeros_like(m2), 0
    return out


def tol(f64, ref):
    """The project's trace rule (hc.trace_tolerance): 64 x the float64 restatement's deviation from the long-double one, floor
    1e-13, relative (hc.rel_dev)."""
    return max(64. * hc.rel_dev(f64, ref), 1e-13)


def check_sharp(got_step, got_frozen, got_alpha, got_samples, got_masses, case, label=''):
    """Both sharp checks on one problem's outputs (of the harness or of the device): the step trace recomputed in long double
    from the alphas it reports, every window's mass recomputed in long double from the samples it reports; each under the 64 x
    rule applied to that recurrence alone (the float64 recomputation against the long-double one, from the same inputs)."""
    fl, cf = case['flags'], case['coef']
    ref_s, ref_f = step_from_alphas(got_alpha, fl, cf, case['log_step'], case['delta'], np.longdouble)
    f64_s, f64_f = step_from_alphas(got_alpha, fl, cf, case['log_step'], case['delta'], np.float64)
    ts, tf = tol(f64_s, ref_s), tol(f64_f, ref_f)
    ds, df = hc.rel_dev(got_step, ref_s), hc.rel_dev(got_frozen, ref_f)
    print('%s: step trace %.3g (tol %.3g), frozen step %.3g (tol %.3g)' % (label, ds, ts, df, tf))
    assert ds <= ts and df <= tf, (label, ds, ts, df, tf)
    ref_m = masses_from_samples(got_samples, fl, case['inv_mass'], np.longdouble)
    f64_m = masses_from_samples(got_samples, fl, case['inv_mass'], np.float64)
    assert len(got_masses) == len(ref_m) == len(window_ends(fl))
    for i, (g, r, f) in enumerate(zip(got_masses, ref_m, f64_m)):
        tm, dm = tol(f, r), hc.rel_dev(g, r)
        print('%s: mass of window %d %.3g (tol %.3g)' % (label, i, dm, tm))
        assert dm <= tm, (label, i, dm, tm)


# ------------------------------------------------------------------ cases
# (name, (n_p ...), D, C, L, W, (init, term, base), kept, log of the start step per problem, seed).  Problem p: rows and weights
# hc.make_data(n_p, D, seed + p); r = RandomState(seed + 200 + p): start = r.randn(C, D) * 0.1, inv_mass = 0.5 + r.rand(D).  Shared
# draws: RandomState(seed + 100): randn(W + kept, C, D), then log(rand(W + kept, C)).  The windows are compressed -- Stan's rule at
# (init, term, base) = (6, 4, 5), which needs W >= 20 -- so that two window ends fall into a short trace.
#   one      the smallest run there is
#   small    several chains; 'w1' beside it has a first window of ONE sample (the mass is kept there) before windows of 2, 4, ...
#   seg2     70 rows: two row segments of the rows pass
#   wide     130 x 128: the largest dimension of the curve
#   huge     a start step of 1e3: every early proposal is refused with alpha = 0 and the step falls until proposals are accepted
#   blowup   a start step of 1e25: H1 overflows in float64, the non-finite branch of alpha, until the step has fallen
#   prior    an all-zero-weight problem: the prior alone
#   batch    three problems of different sizes and start steps in one run
CASES = [
    ('one', (1,), 1, 1, 3, 40, (6, 4, 5), 6, (np.log(1.2),), 51),
    ('small', (5,), 3, 4, 4, 32, (6, 4, 5), 6, (np.log(0.5),), 52),
    ('w1', (5,), 3, 4, 4, 32, (6, 4, 1), 4, (np.log(0.5),), 52),
    ('seg2', (70,), 17, 2, 4, 30, (6, 4, 5), 4, (np.log(0.2),), 53),
    ('wide', (130,), 128, 4, 3, 24, (6, 4, 5), 3, (np.log(0.05),), 54),
    ('huge', (5,), 3, 4, 4, 40, (6, 4, 5), 4, (np.log(1e3),), 55),
    ('blowup', (5,), 3, 2, 4, 40, (6, 4, 5), 2, (np.log(1e25),), 56),
    ('prior', (4,), 3, 3, 4, 30, (6, 4, 5), 4, (np.log(1.0),), 57),
    ('batch', (5, 70, 1), 5, 4, 3, 30, (6, 4, 5), 4, (np.log(0.5), np.log(0.2), np.log(1.0)), 58),
]
CASE_NAMES = [t[0] for t in CASES]


@functools.lru_cache(maxsize=None)
def make_case(name):
    """dict(name, d, c, L, W, flags, coef, delta, E, logU, problems): every problem a case dict for adapt_trace."""
    _, ns, d, c, L, W, bufs, kept, log_steps, seed = [t for t in CASES if t[0] == name][0]
    flags, coef = plan(W, *bufs)
    rng = np.random.RandomState(seed + 100)
    E = rng.randn(W + kept, c, d)
    logU = np.log(rng.rand(W + kept, c))
    problems = []
    for p, n in enumerate(ns):
        Z, w = hc.make_data(n, d, seed + p)
        if name == 'prior':
            w = np.zeros(n)
        r = np.random.RandomState(seed + 200 + p)
        problems.append(dict(name='%s[%d]' % (name, p), Z=Z, w=w, start=r.randn(c, d) * 0.1, inv_mass=0.5 + r.rand(d), log_step=float(log_steps[p]),
                             L=L, E=E, logU=logU, flags=flags, coef=coef, delta=STAN['delta']))
    return dict(name=name, d=d, c=c, L=L, W=W, kept=kept, bufs=bufs, flags=flags, coef=coef, delta=STAN['delta'], E=E, logU=logU, problems=problems)


@functools.lru_cache(maxsize=None)
def reference(name):
    """Per problem (long-double trace, float64 trace) of adapt_trace: computed once, shared, never modified."""
    return [(adapt_trace(pr, np.longdouble), adapt_trace(pr, np.float64)) for pr in make_case(name)['problems']]


def check_condition(name, pair):
    """The condition on a case's inputs, on the long-double trace of `pair` = (long-double trace, float64 trace), warm-up and kept
    iterations together: decisions of both kinds, none within 1e-6 of flipping (hc.check_trace_condition), at least two window
    ends.  A proposal whose H1 is not finite in float64 has no margin there (nan) and an astronomic one in long double (it is
    refused whatever logU is, so it cannot flip); only 'blowup' may hold such, and must."""
    (warm, kept), (fwarm, fkept) = pair[0][:2], pair[1][:2]
    acc = np.concatenate([warm['accept'], kept['accept']])
    margin = np.concatenate([warm['margin'], kept['margin']])
    overflow = np.isnan(np.concatenate([fwarm['margin'], fkept['margin']]))
    assert overflow.any() == (name == 'blowup')
    if name == 'blowup':
        assert not acc[overflow].any() and np.all(margin[overflow] > 1e300) and (fwarm['alpha'][np.isnan(fwarm['margin'])] == 0).all()
        margin = np.where(overflow, 1., margin)
    hc.check_trace_condition(dict(accept=acc, margin=margin))
    assert len(window_ends(make_case(name)['flags'])) >= 2


def compare(got, name, p, label):
    """One problem's outputs `got` (dict: samples, logjoint, accept, step, alpha [W + kept or W, ...], masses, frozen_step, frozen_mass)
    against the long-double restatement: decisions equal; samples, log-joints, the step trace and the final mass within the 64 x
    rule; a rejected chain keeps its bits."""
    (rw, rk, rstep, rim), (fw, fk, fstep, fim) = reference(name)[p]
    case = make_case(name)['problems'][p]
    cat = lambda a, b, key: np.concatenate([a[key], b[key]])
    ref_acc, f_acc = cat(rw, rk, 'accept'), cat(fw, fk, 'accept')
    assert np.array_equal(ref_acc, f_acc), 'the float64 and the long-double restatement decide differently: not a case'
    assert np.array_equal(got['accept'] != 0, ref_acc), label
    pairs = [('samples', got['samples'], cat(fw, fk, 'samples'), cat(rw, rk, 'samples')),
             ('logjoint', got['logjoint'], cat(fw, fk, 'logjoint'), cat(rw, rk, 'logjoint')),
             ('step trace', got['step'], fw['step'], rw['step']), ('frozen step', got['frozen_step'], fstep, rstep),
             ('final mass', got['frozen_mass'], fim, rim)]
    for what, g, f, r in pairs:
        t, dv = tol(f, r), hc.rel_dev(g, r)
        print('%s: %s %.3g (tol %.3g)' % (label, what, dv, t))
        assert dv <= t, (label, what, dv, t)
    acc = got['accept'] != 0
    prev = np.vstack((np.asarray(case['start'])[None], got['samples'][:-1]))
    assert np.array_equal(got['samples'][~acc], prev[~acc]), label


# ------------------------------------------------------------------ the host build of csrc/bc_hmc_adapt_dev.h
def build_harness(outdir, extra=(), name='hmc_adapt_harness'):
    exe = os.path.join(str(outdir), name)
    cmd = ['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-Wall', '-Werror'] + list(extra) \
        + [os.path.join(ROOT, 'tests', 'hmc_adapt_harness.cpp'), '-o', exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def run_harness(exe, case, tmp):
    """The host build on a case: per problem a dict for compare() / check_sharp()."""
    import hmc_many_cases as mc
    problems = case['problems']
    rows, w, row_ptr, start, im, _ = mc.pack([dict(pr, eps=0.) for pr in problems])
    P, c, d = start.shape
    W, T = case['W'], case['W'] + case['kept']
    nwe = len(window_ends(case['flags']))
    head = np.array([P, d, c, case['L'], W, case['kept'], case['delta'], LOG10], dtype=np.float64)
    plan4 = np.hstack((case['coef'], case['flags'][:, None].astype(np.float64)))
    parts = [head, row_ptr, rows, w, start, im, np.array([pr['log_step'] for pr in problems]), plan4, case['E'], case['logU']]
    fin, fout = os.path.join(str(tmp), 'hmc_adapt_in.bin'), os.path.join(str(tmp), 'hmc_adapt_out.bin')
    np.concatenate([np.asarray(x, dtype=np.float64).ravel() for x in parts]).tofile(fin)
    out = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stderr == '', (out.returncode, out.stderr[-2000:])
    res = np.fromfile(fout)
    sizes = [P, P * T * c * d, P * T * c, P * T * c, P * W * c, P * W * c, P * nwe * c * d, P * c, P * c * d]
    assert res.size == sum(sizes), (res.size, sizes)
    cut = np.split(res, np.cumsum(sizes)[:-1])
    status = cut[0].astype(int)
    s, lj, acc = cut[1].reshape(P, T, c, d), cut[2].reshape(P, T, c), cut[3].reshape(P, T, c) != 0
    stp, al, ms = cut[4].reshape(P, W, c), cut[5].reshape(P, W, c), cut[6].reshape(P, nwe, c, d)
    fs, fm = cut[7].reshape(P, c), cut[8].reshape(P, c, d)
    return [dict(status=int(status[p]), samples=s[p], logjoint=lj[p], accept=acc[p], step=stp[p], alpha=al[p], masses=list(ms[p]),
                 frozen_step=fs[p], frozen_mass=fm[p]) for p in range(P)]


# ------------------------------------------------------------------ a stand-in engine for samplers.logistic_hmc_many(adapt='stan')
class NumpyAdaptEngine(hc.NumpyHMCEngine):
    """hc.NumpyHMCEngine plus the per-chain warm-up on the float64 restatement, as samplers._SingleAsBatch drives it:
    adapt_begin / adapt_chunk / adapt_state / adapted_chunk.  `calls` keeps the name and size of every engine call in order."""

    def __init__(self, Z, wts):
        super().__init__(Z, wts)
        self.calls = []

    def begin(self, start, inv_mass, n_leapfrog, n_iter):
        self.calls.append(('begin', n_iter))
        super().begin(start, inv_mass, n_leapfrog, n_iter)

    def chunk(self, normals, log_u, step):
        self.calls.append(('chunk', normals.shape[0]))
        return super().chunk(normals, log_u, step)

    def adapt_begin(self, log_step, target_accept, warmup):
        self.calls.append(('adapt_begin', warmup))
        flags, coef = plan(warmup)
        self.run = AdaptRun(self.Z, self.w, self.th, self.im[0] if self.im.ndim == 2 else self.im, log_step, self.L, flags, coef, target_accept,
                            np.float64)

    def adapt_chunk(self, normals, log_u):
        self.calls.append(('adapt_chunk', normals.shape[0]))
        out = self.run.warm(normals, log_u)
        self.done += normals.shape[0]
        return out['logjoint'], out['accept'].astype(np.int32), out['step'], out['alpha']

    def adapt_state(self):
        self.calls.append(('adapt_state', 0))
        step, im = self.run.frozen()
        return step.copy(), im.copy()

    def adapted_chunk(self, normals, log_u):
        self.calls.append(('adapted_chunk', normals.shape[0]))
        out = self.run.kept(normals, log_u)
        self.done += normals.shape[0]
        return out['samples'], out['logjoint'], out['accept'].astype(np.int32)

    def end(self):
        self.calls.append(('end', 0))
        return super().end()


class AdaptEngines:
    """An engine factory that keeps the NumpyAdaptEngines it made, in order."""

    def __init__(self):
        self.made = []

    def __call__(self, Z, wts):
        self.made.append(NumpyAdaptEngine(Z, wts))
        return self.made[-1]


# ------------------------------------------------------------------ the statistical guard (CPU: on the restatement; GPU: on the device)
GUARD_WARMUP, GUARD_STEPS, GUARD_SEED = 200, (0.01, 2.0), 98


def guard_runs(engine=None, **extra):
    """The runs of the statistical guard: mc.guard_problems() with inv_mass=None, warm-up 200, from the start steps 0.01 and 2.0."""
    import hmc_many_cases as mc
    from beta_cores_amd import samplers
    g = mc.GUARD
    probs, fits = mc.guard_problems()
    runs = []
    for step in GUARD_STEPS:
        rng = np.random.RandomState(GUARD_SEED)
        if engine is not None:      # (the device run draws its start from its own Laplace fits: the same rule)
            e0 = rng.randn(g['c'], g['d'])
            extra['start'] = np.array([mode + e0.dot(LSig.T) for mode, _, LSig in fits])
        runs.append(samplers.logistic_hmc_many(probs, n_samples=g['n_samples'], n_chains=g['c'], step_size=step, n_leapfrog=g['L'], inv_mass=None,
                                               warmup=GUARD_WARMUP, rng=rng, adapt='stan', target_accept=STAN['delta'], engine=engine, **extra))
    return runs, fits


def check_guard_runs(runs, fits, label):
    """mc.check_guard's bars for both runs; per problem the kept mean alpha in [delta, 0.99] -- estimated by the accepted fraction
    of the kept proposals, whose expectation it is (a proposal is accepted with probability alpha; 4800 per problem: a standard
    error below 0.006) -- and the median adapted steps of the two runs within a factor 1.5 of each other."""
    import hmc_many_cases as mc
    for run, step in zip(runs, GUARD_STEPS):
        mc.check_guard(run, fits, '%s, start step %g' % (label, step))
    for p, (a, b) in enumerate(zip(*runs)):
        ma, mb = float(np.median(a.step_size)), float(np.median(b.step_size))
        print('%s guard, problem %d: kept acceptance %.3f / %.3f, median step %.3f / %.3f' % (label, p, a.accept.mean(), b.accept.mean(), ma, mb))
        for r in (a, b):
            assert STAN['delta'] <= r.accept.mean() <= 0.99, (p, r.accept.mean())
        assert max(ma / mb, mb / ma) <= 1.5, (p, ma, mb)


# ------------------------------------------------------------------ a stand-in BATCH engine for samplers._run_hmc_group
class BatchAdaptEngine:
    """samplers._run_hmc_group's batched engine protocol on one NumpyAdaptEngine per problem, as samplers._DeviceHMCMany serves it:
    begin / adapt_begin / adapt_chunk / adapt_state / chunk / end on P problems at once.  The problems in `marked` report the
    status 1 from their first chunk on and nothing else (their slices stay 0), as the device does for a start that is not finite.
    `steps_seen` keeps the `steps` argument of every kept chunk."""

    adapted = False

    def __init__(self, problems, marked=()):
        self.engines, self.marked, self.steps_seen = [NumpyAdaptEngine(Z, w) for Z, w in problems], set(marked), []

    def begin(self, starts, inv_mass, n_leapfrog, n_iter):
        for e, s, im in zip(self.engines, starts, inv_mass):
            e.begin(s, im, n_leapfrog, n_iter)

    def auto_chunk(self, c, d):
        return 7

    def _status(self):
        return np.array([1 if p in self.marked else 0 for p in range(len(self.engines))], dtype=np.int32)

    def _each(self, fn, normals, log_u, shared):
        outs = [None if p in self.marked else fn(e, normals if shared else normals[p], log_u if shared else log_u[p])
                for p, e in enumerate(self.engines)]
        good = [o for o in outs if o is not None][0]
        return [np.array([np.zeros_like(good[i]) if o is None else o[i] for o in outs]) for i in range(len(good))]

    def adapt_begin(self, log_steps, target_accept, warmup):
        for e, ls in zip(self.engines, log_steps):
            e.adapt_begin(float(ls), target_accept, warmup)

    def adapt_chunk(self, normals, log_u, shared):
        lj, acc, stp, alpha = self._each(lambda e, n, u: e.adapt_chunk(n, u), normals, log_u, shared)
        return lj, acc, self._status(), stp, alpha

    def adapt_state(self):
        st = [e.adapt_state() for e in self.engines]
        return np.array([s for s, _ in st]), np.array([m for _, m in st])

    def chunk(self, normals, log_u, steps, shared):
        self.steps_seen.append(steps)
        if self.adapted:
            s, lj, acc = self._each(lambda e, n, u: e.adapted_chunk(n, u), normals, log_u, shared)
        else:
            s, lj, acc = self._each(lambda e, n, u: e.chunk(n, u, float(steps[self.engines.index(e)])), normals, log_u, shared)
        return s, lj, acc, self._status()

    def end(self):
        for e in self.engines:
            e.end()
        return None
