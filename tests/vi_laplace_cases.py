"""Shared by tests/test_vi_laplace_cpu.py and tests/test_gpu_vi_laplace.py (no test collects from this file): the seeded inputs
of the logistic Laplace sampler of the device weight optimisation, a long-double evaluation of its formulas (nothing from
LAPACK or BLAS), the bounds both builds are held to, and a runner for tests/vi_laplace_harness.cpp."""
import functools
import os
import subprocess

import numpy as np

import vi_sampler_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = (1, 2, 3, 16, 33, 64, 127, 128)
SHAPES = ((1, 1), (7, 5), (130, 100), (300, 256))
SCALES = (1., 50., 1e4)
ld = np.longdouble

# The mode's bound: max|mu - mu*| <= C_MODE 2^-53 (1 + max|mu*| + max_j sum_n w_n |z_nj|).  The host's
# samplers._lr_mode_newton, cold from mu0, against reference_mode over grid() + extra_cases() has a worst ratio of 8.91e4
# (test_host_newton_sets_the_constant prints it; profiles/vi_laplace_notes.md); 16 times that -- the margin of
# vc.draw_bound -- rounded up to a power of two.  The ratio is that large because of the host's stopping rule, not of its
# arithmetic: a last line search that backtracks in the rounding noise of f ends the iteration ~1e-9 from the mode (D = 1,
# m = 130), where a full last step ends within a few units.
HOST_WORST_RATIO = 8.91e4
C_MODE = 2. ** 21


def build_harness(outdir, extra=()):
    exe = os.path.join(str(outdir), 'vi_laplace_harness')
    cmd = ['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-Wall', '-Werror'] + list(extra) \
        + [os.path.join(ROOT, 'tests', 'vi_laplace_harness.cpp'), '-o', exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def make_case(d, m, s, variant=0, diag=False):
    """Rows z = y * x of a logistic model, weights in [0, 2] times SCALES[variant % 3] with some exactly 0 (never all of them),
    column 1 = column 0 * (1 + 1e-6 randn) for d > 1, start = 0."""
    rng = np.random.RandomState(31000 + 1000 * d + 10 * m + s)
    x = rng.randn(m, d)
    if d > 1:
        x[:, 1] = x[:, 0] * (1. + 1e-6 * rng.randn(m))
    y = np.where(rng.rand(m) < 1. / (1. + np.exp(-x.dot(rng.randn(d)) / np.sqrt(d))), 1., -1.)
    w = rng.rand(m) * 2.
    w[rng.rand(m) < 0.3] = 0.
    if m > 1:
        w[0], w[m // 2] = 1.25, 0.
    else:
        w[0] = 1.25
    return {'d': d, 'm': m, 's': s, 'Z': y[:, None] * x, 'w': w * SCALES[variant % 3], 'start': np.zeros(d), 'E': rng.randn(s, d),
            'diag': bool(diag), 'variant': variant % 3, 'key': ('grid', d, m, s, variant % 3)}


def grid():
    return [make_case(d, m, s, variant=i + d) for d in DIMS for i, (m, s) in enumerate(SHAPES)]


def far_start_case():
    """start = 50 * ones: the first Newton steps overshoot, the line search must halve."""
    c = make_case(16, 130, 5, variant=0)
    c['start'] = 50. * np.ones(16)
    c['key'] = ('far',)
    return c


def large_margin_case():
    """Rows scaled so that -z . start >= 100 for some of them (the branch model_lr.py takes at m >= 100)."""
    c = make_case(16, 130, 5, variant=1)
    c['start'] = np.ones(16)
    zs = c['Z'].dot(c['start'])
    Z = c['Z'].copy()
    for n in (3, 40, 77):
        Z[n] *= -150. / zs[n]
    c['Z'] = Z
    c['w'][[3, 40, 77]] = [0.5, 1.0, 2.0]
    assert (-Z.dot(c['start']) >= 100.).sum() >= 3
    c['key'] = ('margin',)
    return c


def extra_cases():
    return [far_start_case(), large_margin_case()]


# ---------------------------------------------------------------- the formulas in long double
def _chol_ld(A):
    d = A.shape[0]
    Cf = np.zeros((d, d), dtype=ld)
    for k in range(d):
        col = A[k:, k] - Cf[k:, :k].dot(Cf[k, :k])
        if not (col[0] > 0. and np.isfinite(col[0])):
            raise np.linalg.LinAlgError('pivot %d is not finite and positive' % k)
        piv = np.sqrt(col[0])
        Cf[k:, k] = col / piv
        Cf[k, k] = piv
    return Cf


def _solve_lower(Cf, b):
    x = np.zeros_like(b)
    for i in range(Cf.shape[0]):
        x[i] = (b[i] - Cf[i, :i].dot(x[:i])) / Cf[i, i]
    return x


def _solve_upper(U, b):
    x = np.zeros_like(b)
    for i in range(U.shape[0] - 1, -1, -1):
        x[i] = (b[i] - U[i, i + 1:].dot(x[i + 1:])) / U[i, i]
    return x


def _rows(c):
    keep = c['w'] > 0
    return np.asarray(c['Z'][keep], dtype=ld), np.asarray(c['w'][keep], dtype=ld)


def hessian_ld(c, mu):
    """H(mu) = I + Z^T diag(w p (1 - p)) Z in long double."""
    Z, w = _rows(c)
    mm = -Z.dot(np.asarray(mu, dtype=ld))
    p = ld(0.5) * (ld(1.) + np.tanh(ld(0.5) * mm))
    return np.eye(c['d'], dtype=ld) + (Z * (w * p * (ld(1.) - p))[:, None]).T.dot(Z)


@functools.lru_cache(maxsize=None)
def _reference_mode(key, maker):
    return compute_reference_mode(maker())


def compute_reference_mode(c):
    Z, w = _rows(c)
    d = c['d']
    mu = np.zeros(d, dtype=ld)

    def value(th):
        mm = -Z.dot(th)
        return -(w * (np.maximum(mm, 0.) + np.log1p(np.exp(-np.fabs(mm))))).sum() - ld(0.5) * th.dot(th)
    f = value(mu)
    floor_scale = 1. + (w[:, None] * np.fabs(Z)).sum(axis=0).max()
    for _ in range(500):
        mm = -Z.dot(mu)
        p = ld(0.5) * (ld(1.) + np.tanh(ld(0.5) * mm))
        g = -mu + Z.T.dot(w * p)
        Cf = _chol_ld(hessian_ld(c, mu))
        step = _solve_upper(Cf.T, _solve_lower(Cf, g))
        t, dec = ld(1.), g.dot(step)
        while True:
            cand = mu + t * step
            fc = value(cand)
            if fc >= f + ld(1e-4) * t * dec or t < 1e-10:
                break
            t *= ld(0.5)
        mu, f = cand, fc
        # (the second form is the same rule at long double's own rounding floor: with weights of 1e4 the gradient carries
        # eps_ld sum_n w_n |z_nj| of noise, which H^-1 hands on undamped along a nearly collinear direction -- the step
        # then never falls below 1e-17.  64 eps_ld of the bound's scale is at most 1/16 of ONE unit of C_MODE.)
        if np.fabs(step).max() <= max(ld(1e-17) * (1. + np.fabs(mu).max()), 64. * np.finfo(ld).eps * floor_scale):
            return mu
    raise AssertionError('the long-double Newton iteration did not converge')


def reference_mode(c):
    """mu* (long double): the iteration of the header in np.longdouble from mu0 = 0 until max|step| <= 1e-17 (1 + max|mu|)
    (backtracking as in the header, so that a far start cannot diverge).  Cached per case key (the cases are deterministic); a
    case without a key is evaluated as it stands."""
    if 'key' not in c:
        return compute_reference_mode(c)
    makers = {'grid': lambda: make_case(*c['key'][1:]), 'far': far_start_case, 'margin': large_margin_case}
    return _reference_mode(c['key'], makers[c['key'][0]])


def mode_bound(c, mu_ref):
    return C_MODE * 2. ** -53 * mode_scale(c, mu_ref)


def mode_scale(c, mu_ref):
    return float(1. + np.abs(mu_ref).max() + (c['w'][:, None] * np.abs(c['Z'])).sum(axis=0).max())


def reference_draw(c, mu, diag=None):
    """(Theta - mu in long double, rounded to double; kappa) around the GIVEN mu: E . C(mu)^-T with kappa_2(H(mu)), or for the
    diagonal form E / sqrt(diag H(mu)) with kappa = max / min of that diagonal."""
    diag = c['diag'] if diag is None else diag
    H = hessian_ld(c, mu)
    E = np.asarray(c['E'], dtype=ld)
    if diag:
        h = np.diag(H)
        return (E / np.sqrt(h)).astype(np.float64), float(h.max() / h.min())
    Cf = _chol_ld(H)
    d = c['d']
    L = np.zeros((d, d), dtype=ld)
    for i in range(d):
        e = np.zeros(d, dtype=ld)
        e[i] = 1.
        L[i] = (e - Cf[i, :i].dot(L[:i])) / Cf[i, i]
    Hd = H.astype(np.float64)
    return E.dot(L.T).astype(np.float64), float(np.linalg.cond((Hd + Hd.T) / 2., 2))


def check_mode_and_draw(c, mu, theta, label=''):
    """Checks 1 and 2 of the sampler on a returned (mu, Theta); returns (mode ratio, draw ratio) of error / bound."""
    assert vc.LD_OK
    mu_ref = reference_mode(c).astype(np.float64)
    err_m, bound_m = np.abs(mu - mu_ref).max(), mode_bound(c, mu_ref)
    ref, kappa = reference_draw(c, mu)
    err_d, bound_d = np.abs((theta - mu) - ref).max(), vc.draw_bound(c['d'], kappa, ref)
    print('%s D %3d m %3d S %3d max w %g: mode error %.3e (bound %.3e), draw error %.3e (bound %.3e), kappa %.3e'
          % (label, c['d'], c['m'], c['s'], c['w'].max(), err_m, bound_m, err_d, bound_d, kappa))
    assert err_m <= bound_m, (label, c.get('key'), err_m, bound_m)
    assert err_d <= bound_d, (label, c.get('key'), err_d, bound_d)
    return err_m / bound_m, err_d / bound_d


def run_laplace(exe, c, tmp):
    """dict(status, theta [s][d], pad [s][3], mode [d], dec, counts [4]: Newton steps, halvings of the last
    line search, the running total of steps, halvings of all line searches) of the host build of bc_vi_laplace on case c; after a
    failure dict(status, untouched)."""
    d, s = c['d'], c['s']
    parts = [np.array([d, c['m'], s, 1. if c['diag'] else 0.]), c['Z'].ravel(), c['w'], c['start'], c['E'].ravel()]
    fin, fout = os.path.join(str(tmp), 'lap_in.bin'), os.path.join(str(tmp), 'lap_out.bin')
    np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in parts]).tofile(fin)
    out = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stderr == '', (out.returncode, out.stderr[-2000:])
    res = np.fromfile(fout)
    if int(res[0]) != 0:
        assert res.size == 2
        return {'status': int(res[0]), 'untouched': bool(res[1])}
    dk = d + 3
    theta = res[1:1 + s * dk].reshape(s, dk)
    tail = res[1 + s * dk:]
    assert tail.size == d + 1 + 4
    return {'status': 0, 'theta': theta[:, :d], 'pad': theta[:, d:], 'mode': tail[:d], 'dec': tail[d], 'counts': tail[d + 1:].astype(int)}
