"""Shared by tests/test_psvi_grad_cpu.py, tests/test_psvi_grad_sanitized_cpu.py and tests/test_gpu_psvi_fused.py (no test
collects from this file): the seeded inputs of BatchPSVICoreset's point-gradient, the reference's expression in np.longdouble,
the forward-error bound, and a runner for tests/psvi_grad_harness.cpp.

The bound.  The device forms, per point i (csrc/bc_psvi_dev.h),
    V[c] = sum_s coef_s T[s, c],  coef_s = r_s fac_s,  mean = (sum_c V[c]) / W,  g[c] = -(w_i / S) (V[c] - mean)
where fac_s hangs on a D-term dot product p_s = x_i . th_s (Gaussian: T and x_i . Siginv are D-term chains themselves).
Let Gabs[i, s, c] be the un-centred gradient Gu[i, s, c] "with every term's absolute value", the terms of the inner D-term sums
included:
    linear regression    (|y| + sum_k |x_k th_sk|) / sigsq * |[th_s, 1]_c|
    logistic regression  (fac + fac (1 - fac) sum_k |z_k th_sk|) * |th_sc|     (|dfac/dm| = fac (1 - fac): the error of m = -z.th)
    Gaussian location    sum_k (|th_sk| + |x_k|) |Siginv[k, c]|
and  A[i, c] = |w_i| / S * sum_s |r_s| (Gabs[i, s, c] + mean_c Gabs[i, s, :]).
With u = 2^-53 and gamma_n ~ n u the roundings add up, to first order, as follows.  coef_s: the dot product's gamma_D (times
|dfac/dp|), a handful of u for exp, the division and the two products -- at most (D + 6) u Gabs per term.  The S-term fma chain
of V[c]: gamma_S.  So |dV[c]| <= (S + D + 6) u sum_s |r_s| Gabs[s, c].  The mean over W <= D + 1 coordinates, however it is
blocked: the dV's averaged, plus gamma_W mean_c |V[c]|, plus the division: (S + 2 D + 8) u of the mean of the same sums.  The
subtraction, the scale -(w_i / S) and its division: 3 u more.  In total |error| <= (S + 2 D + 12) u A[i, c], and
S + 2 D + 12 <= 8 (S + D) for every S, D >= 1.  Hence
    bound[i, c] = 8 (S + D) 2^-53 A[i, c]                                      (C_BOUND = 8)
The reference below is evaluated in np.longdouble (2^-64 or finer): its own error is three decimal orders below the bound."""
import os
import subprocess

import numpy as np

from oracle import models_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINREG, LOGISTIC, GAUSS = 0, 1, 2
SHAPES = ((1, 1), (7, 5), (130, 100), (40, 256))                 # (M, S)
DIMS = (1, 2, 3, 33, 64, 127, 128, 300)
MODELS = ((LINREG, 1.), (LINREG, 2.5), (LOGISTIC, 0.), (GAUSS, 0.))      # (kind, sigsq)
C_BOUND = 8.
LD_OK = np.finfo(np.longdouble).nmant >= 63


def build_harness(outdir, extra=()):
    exe = os.path.join(str(outdir), 'psvi_grad_harness')
    cmd = ['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-Wall', '-Werror', '-Wno-unknown-pragmas'] + list(extra) \
        + [os.path.join(ROOT, 'tests', 'psvi_grad_harness.cpp'), '-o', exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def make_case(kind, m, s, d, sigsq=1.):
    """Points, weights in [0, 2] with an exact 0 (m > 1), Theta, a residual.  Logistic: row 0 is scaled so that some -z.th lie
    beyond the branch at 100 (d large enough for the products to get there)."""
    rng = np.random.RandomState(100000 * kind + 1000 * d + 10 * m + s + int(10 * sigsq))
    x = rng.randn(m, d)
    th = rng.randn(s, d)
    w = rng.rand(m) * 2. + .05
    if m > 1:
        w[m // 2] = 0.
    c = {'kind': kind, 'm': m, 's': s, 'd': d, 'sigsq': float(sigsq), 'w': w, 'theta': th, 'resid': rng.randn(s) * 3.}
    if kind == LINREG:
        y = x.dot(rng.randn(d)) + rng.randn(m)
        c['pts'] = np.hstack((x, y[:, None]))
    elif kind == LOGISTIC:
        x = x * 2.
        x[0] *= 80. / np.sqrt(d)
        c['pts'] = x
    else:
        q = rng.randn(d, d)
        Si = np.linalg.inv(q.dot(q.T) / d + np.eye(d))
        c['Siginv'] = (Si + Si.T) / 2.
        c['pts'] = x * 3.
    return c


def _dots(x, th):
    """x . th^T without BLAS, in the dtype of the inputs (M x S), and the same sum of absolute values"""
    prod = x[:, np.newaxis, :] * th[np.newaxis, :, :]
    return prod.sum(axis=2), np.abs(prod).sum(axis=2)


def tensors_ld(c):
    """(Gu, Gabs) in np.longdouble, M x S x W: oracle/models_ref.py's x-gradient formulas and the same with every term's
    absolute value (module docstring)."""
    ld = np.longdouble
    pts, th = np.asarray(c['pts'], dtype=ld), np.asarray(c['theta'], dtype=ld)
    d = c['d']
    if c['kind'] == LINREG:
        x, y = pts[:, :d], pts[:, d]
        p, pabs = _dots(x, th)
        ext = np.hstack((th, np.ones((th.shape[0], 1), dtype=ld)))
        fac = 1. / ld(c['sigsq']) * (y[:, np.newaxis] - p)
        fabs = 1. / ld(c['sigsq']) * (np.abs(y)[:, np.newaxis] + pabs)
        return fac[:, :, np.newaxis] * ext[np.newaxis], fabs[:, :, np.newaxis] * np.abs(ext)[np.newaxis]
    if c['kind'] == LOGISTIC:
        p, pabs = _dots(pts, th)
        mm = -p
        small = mm < 100
        fac = np.ones_like(mm)
        fac[small] = np.exp(mm[small]) / (1. + np.exp(mm[small]))
        fabs = fac + fac * (1. - fac) * pabs
        return fac[:, :, np.newaxis] * th[np.newaxis], fabs[:, :, np.newaxis] * np.abs(th)[np.newaxis]
    Si = np.asarray(c['Siginv'], dtype=ld)
    # (np.dot of np.longdouble arrays never goes through BLAS: NumPy's own long-double loops)
    ts, xs = th.dot(Si), pts.dot(Si)
    tsa, xsa = np.abs(th).dot(np.abs(Si)), np.abs(pts).dot(np.abs(Si))
    return ts[np.newaxis] - xs[:, np.newaxis], tsa[np.newaxis] + xsa[:, np.newaxis]


def reference(c, resid=None, w=None):
    """(g_p, bound) in np.longdouble, M x W: the reference's expression -- the un-centred tensor, centred per (i, s) over the
    coordinates, times w_i r_s, summed over s, divided by -S -- and the bound of the module docstring.  `resid`, `w`: in place of
    the case's own (the GPU tests pass the residual the device has formed)."""
    ld = np.longdouble
    r = np.asarray(c['resid'] if resid is None else resid, dtype=ld)
    w = np.asarray(c['w'] if w is None else w, dtype=ld)
    S, D = c['s'], c['d']
    Gu, Gabs = tensors_ld(c)
    G = Gu - Gu.mean(axis=2)[:, :, np.newaxis]
    g = -(w[:, np.newaxis, np.newaxis] * G * r[np.newaxis, :, np.newaxis]).sum(axis=1) / S
    A = (np.abs(w)[:, np.newaxis, np.newaxis] * (Gabs + Gabs.mean(axis=2)[:, :, np.newaxis]) * np.abs(r)[np.newaxis, :, np.newaxis]).sum(axis=1) / S
    return g, ld(C_BOUND * (S + D) * 2. ** -53) * A


def numpy_expression(c, resid=None, w=None):
    """bpsvi.py:80 in NumPy doubles on oracle.coreset_ref.project_grad's tensor (what the unfused path computes on the host)"""
    r = c['resid'] if resid is None else resid
    w = c['w'] if w is None else w
    if c['kind'] == LINREG:
        g = models_ref.linreg_grad_x_loglik(c['pts'], c['theta'], c['sigsq'])
    elif c['kind'] == LOGISTIC:
        g = models_ref.logistic_grad_z_loglik(c['pts'], c['theta'])
    else:
        g = models_ref.gauss_grad_x_loglik(c['pts'], c['theta'], c['Siginv'])
    g = g - g.mean(axis=2)[:, :, np.newaxis]                       # coreset_ref.project_grad's centring
    return -(w[:, np.newaxis, np.newaxis] * g * r[np.newaxis, :, np.newaxis]).sum(axis=1) / c['s']


def staged_theta(c, dk):
    """Theta as K1's staging lays it out: rows of pitch dk, zero-padded; Gaussian: Theta' = (Siginv . Theta^T)^T"""
    th = c['theta'] if c['kind'] != GAUSS else c['theta'].dot(c['Siginv'].T)
    out = np.zeros((c['s'], dk))
    out[:, :c['d']] = th
    return out


def run_harness(exe, c, tmp):
    """g_p (M x W) of the host build of bc_psvi_point_grad on case c"""
    d = c['d']
    dk = ((d + 15) // 16) * 16
    parts = [np.array([c['kind'], c['m'], c['s'], d, dk, c['sigsq']], dtype=np.float64), c['pts'].ravel(), c['w'], staged_theta(c, dk).ravel()]
    if c['kind'] == GAUSS:
        parts.append(c['Siginv'].ravel())
    parts.append(c['resid'])
    fin, fout = os.path.join(str(tmp), 'psvi_in.bin'), os.path.join(str(tmp), 'psvi_out.bin')
    np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in parts]).tofile(fin)
    out = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stderr == '', (out.returncode, out.stderr[-2000:])
    return np.fromfile(fout).reshape(c['pts'].shape)
