"""Shared by tests/test_vi_sampler_cpu.py, tests/test_vi_sampler_sanitized_cpu.py and tests/test_gpu_vi_optimize.py (no test
collects from this file): the seeded inputs of the posterior draw (identity and general priors), the oracle's answer, a
long-double evaluation of the same formulas, and a runner for tests/vi_sampler_harness.cpp."""
import os
import subprocess

import numpy as np

from oracle import models_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINREG, GAUSS = 0, 1
DIMS, ROWS, SAMPLES = (1, 2, 3, 16, 33, 64, 128), (1, 7, 130), (1, 5, 100)


def build_harness(outdir, extra=()):
    exe = os.path.join(str(outdir), 'vi_sampler_harness')
    cmd = ['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-Wall', '-Werror'] + list(extra) \
        + [os.path.join(ROOT, 'tests', 'vi_sampler_harness.cpp'), '-o', exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def make_case(kind, d, m, s, sig0_sign=1.):
    """Sig0inv = I (times sig0_sign), weights in [0, 2] with some exactly 0 (never all of them)."""
    rng = np.random.RandomState(1000 * d + 10 * m + s + kind)
    x = rng.randn(m, d)
    w = rng.rand(m) * 2.
    w[rng.rand(m) < 0.3] = 0.
    if m > 1:
        w[0], w[m // 2] = 1.25, 0.
    th0 = rng.randn(d)
    E = rng.randn(s, d)
    c = {'kind': kind, 'd': d, 'm': m, 's': s, 'w': w, 'th0': th0, 'Sig0inv': sig0_sign * np.eye(d), 'E': E}
    if kind == LINREG:
        y = x.dot(rng.randn(d)) + rng.randn(m)
        c['rows'] = np.hstack((x, y[:, None]))
        c['sigsq'] = 1.5
    else:
        q = rng.randn(d, d)
        Sig = q.dot(q.T) / d + np.eye(d)
        c['rows'] = x
        c['Siginv'] = np.linalg.inv(Sig)
        c['Siginv'] = (c['Siginv'] + c['Siginv'].T) / 2.
    return c


def reference(c):
    """(Theta_ref = mu + E . L^T, kappa_2(A)) from the oracle's weighted posterior."""
    if c['kind'] == LINREG:
        mu, Ci, C = models_ref.linreg_weighted_post(c['th0'], c['Sig0inv'], c['sigsq'], c['rows'], c['w'])
    else:
        mu, Ci, C = models_ref.gauss_weighted_post(c['th0'], c['Sig0inv'], c['Siginv'], c['rows'], c['w'])
    return mu + c['E'].dot(Ci.T), np.linalg.cond(C.dot(C.T), 2)


# ---------------------------------------------------------------- general priors
# (sigsq, weight scale, column 1 nearly collinear with column 0): every sigsq, every scale and the collinear form occur
VARIANTS = ((0.37, 1., False), (2.5, 50., False), (0.37, 1e4, False), (2.5, 1., True), (0.37, 50., True), (2.5, 1e4, True))
MORE_DIMS = tuple(sorted(set(DIMS) | {127}))
SHAPES = tuple((m, s) for m in ROWS for s in SAMPLES) + ((300, 256),)


def make_general_case(kind, d, m, s, variant=0):
    """make_case's rows, weights and normals with a prior that is not the identity: Sig0inv = Q diag(lambda) Q^T (symmetrised,
    lambda log-spaced over [1e-2, 1e2]), th0 = 3 randn + 1, and VARIANTS[variant]: sigsq (linear regression), the weights
    times a scale, column 1 = column 0 * (1 + 1e-6 randn) (for d > 1)."""
    sigsq, scale, collinear = VARIANTS[variant % len(VARIANTS)]
    c = make_case(kind, d, m, s)
    rng = np.random.RandomState(77000 + 1000 * d + 10 * m + s + kind)
    q = np.linalg.qr(rng.randn(d, d))[0]
    S0 = (q * np.logspace(-2., 2., d)).dot(q.T)
    c['Sig0inv'] = (S0 + S0.T) / 2.
    c['th0'] = 3. * rng.randn(d) + 1.
    c['w'] = c['w'] * scale
    if collinear and d > 1:
        c['rows'] = c['rows'].copy()
        c['rows'][:, 1] = c['rows'][:, 0] * (1. + 1e-6 * rng.randn(m))
    if kind == LINREG:
        c['sigsq'] = sigsq
    c['variant'] = variant % len(VARIANTS)
    return c


LD_OK = np.finfo(np.longdouble).nmant >= 63      # x87 extended or wider: 11 bits or more below double's rounding


def reference_ld(c):
    """The header comment of csrc/bc_vi_sampler_dev.h evaluated in np.longdouble, nothing from LAPACK or BLAS: A and rhs
    summed in long double, an explicit left-looking Cholesky of A's LOWER triangle, L = C^-1 by forward substitution,
    mu = (L . L^T) . rhs (the reference's expression, not C^-T C^-1), Theta = mu + E . L^T; rhs takes the FULL Sig0inv.
    Returns a dict of float64 arrays: theta, mu, kappa (kappa_2 of A, symmetric from its lower triangle) and, for the Gaussian
    kind, thp = Theta . Siginv^T and saux = theta^T Siginv theta.  Raises np.linalg.LinAlgError on a pivot that is not
    finite and positive."""
    ld = np.longdouble
    d = c['d']
    w, rows, S0, th0, E = [np.asarray(c[k], dtype=ld) for k in ('w', 'rows', 'Sig0inv', 'th0', 'E')]
    if c['kind'] == LINREG:
        X, y, sigsq = rows[:, :d], rows[:, d], ld(c['sigsq'])
        A = S0 + (X * w[:, None]).T.dot(X) / sigsq
        rhs = S0.dot(th0) + (X * (w * y)[:, None]).sum(axis=0) / sigsq
    else:
        Si = np.asarray(c['Siginv'], dtype=ld)
        A = S0 + w.sum() * Si
        rhs = S0.dot(th0) + Si.dot((rows * w[:, None]).sum(axis=0))
    Cf = np.zeros((d, d), dtype=ld)
    for k in range(d):
        col = A[k:, k] - Cf[k:, :k].dot(Cf[k, :k])
        if not (col[0] > 0. and np.isfinite(col[0])):
            raise np.linalg.LinAlgError('pivot %d is not finite and positive' % k)
        piv = np.sqrt(col[0])
        Cf[k:, k] = col / piv
        Cf[k, k] = piv
    L = np.zeros((d, d), dtype=ld)
    for i in range(d):
        e = np.zeros(d, dtype=ld)
        e[i] = 1.
        L[i] = (e - Cf[i, :i].dot(L[:i])) / Cf[i, i]
    mu = L.dot(L.T).dot(rhs)
    theta = mu + E.dot(L.T)
    Al = np.tril(A).astype(np.float64)
    out = {'theta': theta.astype(np.float64), 'mu': mu.astype(np.float64),
           'kappa': np.linalg.cond(Al + np.tril(Al, -1).T, 2)}
    if c['kind'] == GAUSS:
        out['thp'] = theta.dot(Si.T).astype(np.float64)
        out['saux'] = (theta * theta.dot(Si)).sum(axis=1).astype(np.float64)
    return out


def high_precision_reference(c):
    """(Theta_ref, kappa_2(A)): reference_ld where long double is wider than double, else the oracle (and says so)."""
    if LD_OK:
        r = reference_ld(c)
        return r['theta'], r['kappa']
    print('np.longdouble has only %d mantissa bits here: the reference is the oracle (LAPACK, double)' % np.finfo(np.longdouble).nmant)
    return reference(c)


def draw_bound(d, kappa, ref):
    """The project's bound of the draw: the forward-error form of a Cholesky solve with a margin of 16."""
    return 16. * d * 2. ** -53 * kappa * (1. + np.abs(ref).max())


def run_sampler(exe, c, tmp):
    """(status, theta [s][d], pad [s][3], saux [s], raw [s][d]) of the host build of bc_vi_sampler on case c."""
    d, m, s = c['d'], c['m'], c['s']
    parts = [np.array([c['kind'], d, m, s], dtype=np.float64), c['rows'].ravel(), c['w'], c['Sig0inv'].ravel(),
             c['th0']]
    parts.append(np.array([c['sigsq']]) if c['kind'] == LINREG else c['Siginv'].ravel())
    parts.append(c['E'].ravel())
    fin, fout = os.path.join(str(tmp), 'in.bin'), os.path.join(str(tmp), 'out.bin')
    np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in parts]).tofile(fin)
    out = subprocess.run([exe, 'sampler', fin, fout], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stderr == '', (out.returncode, out.stderr[-2000:])
    res = np.fromfile(fout)
    if int(res[0]) != 0:
        assert res.size == 1
        return int(res[0]), None, None, None, None
    dk = d + 3
    theta = res[1:1 + s * dk].reshape(s, dk)
    saux = res[1 + s * dk:1 + s * dk + s]
    raw = res[1 + s * dk + s:].reshape(s, d)
    return 0, theta[:, :d], theta[:, d:], saux, raw


def run_adam(exe, q, c, x0, step, tmp):
    itrs = step.shape[1]
    fin, fout = os.path.join(str(tmp), 'adam_in.bin'), os.path.join(str(tmp), 'adam_out.bin')
    np.concatenate([np.array([q.shape[0], itrs], dtype=np.float64), q, c, x0, step.ravel()]).tofile(fin)
    out = subprocess.run([exe, 'adam', fin, fout], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stderr == '', (out.returncode, out.stderr[-2000:])
    return np.fromfile(fout).reshape(itrs, q.shape[0])
