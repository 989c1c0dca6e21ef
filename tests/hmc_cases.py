"""The NumPy restatement of the multi-chain logistic HMC sampler (include/beta_cores_hmc.h, csrc/bc_hmc_dev.h), the derived
bound of the multi-chain rows pass, the cases the tests share, a stand-in engine for samplers.logistic_hmc and the build of
tests/hmc_harness.cpp.  The restatement is parametrised by dtype: np.float64, or np.longdouble as the high-precision reference.
Test infrastructure only: the product never imports this module."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


# ------------------------------------------------------------------ the formulas
def lr_terms(m):
    """ll, p of model_lr.py:72-79, 98-105 in m's dtype, overflow-free, with the branch at m >= 100."""
    e = np.exp(-np.abs(m))
    small = m < 100
    ll = np.where(small, -(np.maximum(m, 0) + np.log1p(e)), -m)
    p = np.where(small, np.where(m >= 0, 1 / (1 + e), e / (1 + e)), np.ones_like(m))
    return ll, p


def rows_pass(Z, w, thetas, dtype=np.longdouble):
    """value [C], grad [C, D] of the weighted likelihood, WITHOUT the prior; also m, ll, p (n x C) for the bound."""
    Z = np.asarray(Z).astype(dtype)
    th = np.atleast_2d(thetas).astype(dtype)
    w = np.ones(Z.shape[0], dtype=dtype) if w is None else np.asarray(w).astype(dtype)
    m = -Z.dot(th.T)
    ll, p = lr_terms(m)
    return (w[:, None] * ll).sum(axis=0), (w[:, None] * p).T.dot(Z), m, ll, p


def logjoint(Z, w, thetas, dtype=np.longdouble):
    """(values [C], grads [C, D]) of model_lr.py:88-93: likelihood + N(0, I) prior."""
    th = np.atleast_2d(thetas).astype(dtype)
    d = th.shape[1]
    val, grad = rows_pass(Z, w, th, dtype)[:2]
    hdl = dtype(0.5 * d * np.log(2. * np.pi))      # (the double the library evaluates on the host)
    return val - hdl - (th * th).sum(axis=1) / 2, grad - th


def rows_pass_bound(Z, w, thetas):
    """Element-wise bound on |device - exact| of logjoint()'s two results for float64 arithmetic in ANY association, every
    term at its absolute value (u = 2^-53; second-order terms are covered by the final factor 1.01):

      m      a D-term dot product:                           dm  = (D + 2) u |z| . |theta|
      p      |dp/dm| <= 1/4, then exp, one add, one divide:   dp  = dm / 4 + 8 u            (p <= 1)
      ll     |dll/dm| <= 1, then exp, log1p, two adds:       dll = dm + 8 u (|ll| + 1)
             (the two sides of the branch at m = 100 differ by < e^-100: nothing next to u)
      value  sum_n w ll: n terms in any order, each product fused or rounded once:    sum |w| dll + (n + 2) u sum |w ll|
             - (D/2) log 2 pi - |theta|^2 / 2: a D-term sum of squares and three roundings
      grad   sum_n (w p) z: one rounding of w p, then n terms in any order:           sum |w| dp |z| + (n + 4) u sum |w p z|
             - theta: one rounding
    Returns (bound_value [C], bound_grad [C, D])."""
    ld = np.longdouble
    Zl = np.abs(np.asarray(Z).astype(ld))
    th = np.atleast_2d(thetas).astype(ld)
    n, d = Zl.shape
    wl = np.ones(n, dtype=ld) if w is None else np.abs(np.asarray(w).astype(ld))
    val, grad, _, ll, p = rows_pass(Z, w, thetas, ld)
    dm = (d + 2) * U * Zl.dot(np.abs(th).T)
    dp = dm / 4 + 8 * U
    dll = dm + 8 * U * (np.abs(ll) + 1)
    ss = (th * th).sum(axis=1) / 2
    hdl = 0.5 * d * np.log(2. * np.pi)
    bv = (wl[:, None] * dll).sum(axis=0) + (n + 2) * U * (wl[:, None] * np.abs(ll)).sum(axis=0) + (d + 2) * U * ss \
        + 4 * U * (np.abs(val) + hdl + ss)
    bg = (wl[:, None] * dp).T.dot(Zl) + (n + 4) * U * (wl[:, None] * p).T.dot(Zl) + 2 * U * (np.abs(grad) + np.abs(th))
    return (1.01 * bv).astype(np.float64), (1.01 * bg).astype(np.float64)


def hmc_run(Z, w, start, inv_mass, eps, n_leapfrog, E, logU, dtype=np.longdouble):
    """The sampler of include/beta_cores_hmc.h on given draws E [T, C, D], logU [T, C].  Returns a dict: samples [T, C, D],
    logjoint [T, C], accept [T, C] (bool), margin [T, C] = logU - (H0 - H1) (nan where H1 is not finite)."""
    th = np.array(start).astype(dtype)
    im = np.asarray(inv_mass).astype(dtype)
    eps = dtype(eps)
    T, C, D = E.shape
    lj, g = logjoint(Z, w, th, dtype)
    out = dict(samples=np.empty((T, C, D), dtype=dtype), logjoint=np.empty((T, C), dtype=dtype), accept=np.zeros((T, C), dtype=bool),
               margin=np.full((T, C), np.nan))
    for t in range(T):
        r = E[t].astype(dtype) / np.sqrt(im)
        h0 = -lj + (im * r * r).sum(axis=1) / 2
        r = r + eps / 2 * g
        thp = th + eps * (im * r)
        for l in range(1, n_leapfrog + 1):
            with np.errstate(all='ignore'):
                ljp, gp = logjoint(Z, w, thp, dtype)
                if l < n_leapfrog:
                    r = r + eps * gp
                    thp = thp + eps * (im * r)
                else:
                    r = r + eps / 2 * gp
        with np.errstate(all='ignore'):
            h1 = -ljp + (im * r * r).sum(axis=1) / 2
            fin = np.isfinite(h1)
            acc = np.logical_and(fin, logU[t].astype(dtype) < h0 - h1)
            out['margin'][t] = np.where(fin, (logU[t].astype(dtype) - (h0 - h1)), np.nan).astype(np.float64)
        th = np.where(acc[:, None], thp, th)
        g = np.where(acc[:, None], gp, g)
        lj = np.where(acc, ljp, lj)
        out['samples'][t], out['logjoint'][t], out['accept'][t] = th, lj, acc
    return out


def rel_dev(a, b):
    """max |a - b| / max |b|: the relative deviation the trace tolerances are stated in."""
    b = np.asarray(b)
    return float(np.abs(np.asarray(a).astype(b.dtype) - b).max() / np.abs(b).max())


# ------------------------------------------------------------------ cases
def make_data(n, d, seed, weighted=True, zero_frac=0.2):
    """Rows z = y * x with an intercept column of ones (the last), labels from a logistic model; weights in [0, 2) with zeros."""
    rng = np.random.RandomState(seed)
    x = rng.randn(n, d)
    x[:, -1] = 1.
    ths = rng.randn(d) / np.sqrt(d)
    y = np.where(rng.rand(n) < 1. / (1. + np.exp(-x.dot(ths))), 1., -1.)
    w = None
    if weighted:
        w = rng.rand(n) * 2.
        w[rng.rand(n) < zero_frac] = 0.
    return y[:, None] * x, w


# (name, n, D, C, L, T, eps, seed): eps chosen on the float64 restatement so that the trace holds accepted AND rejected proposals,
# all with |logU - (H0 - H1)| > 1e-6 (asserted by the tests that use them, on the restatement)
TRACE_CASES = [
    ('small', 500, 5, 3, 4, 6, 0.1, 11),
    ('wide', 300, 128, 16, 4, 6, 0.08, 12),
]


def make_trace_case(name):
    _, n, d, c, L, T, eps, seed = [t for t in TRACE_CASES if t[0] == name][0]
    Z, w = make_data(n, d, seed)
    rng = np.random.RandomState(seed + 100)
    return dict(name=name, Z=Z, w=w, start=rng.randn(c, d) * 0.1, inv_mass=0.5 + rng.rand(d), eps=eps, L=L,
                E=rng.randn(T, c, d), logU=np.log(rng.rand(T, c)))


def check_trace_condition(ref):
    """The condition on the inputs of a trace comparison: decisions of both kinds, none within 1e-6 of flipping."""
    assert ref['accept'].any() and not ref['accept'].all(), 'the case needs accepted and rejected proposals'
    assert np.all(np.isfinite(ref['margin'])) and np.abs(ref['margin']).min() > 1e-6, np.abs(ref['margin']).min()


def trace_tolerance(case):
    """Per case: 64 x the deviation of the float64 restatement from the long-double one (64: the margin for a different
    association of sums of this length), with a floor of 1e-13, relative (rel_dev).  Returns (reference, tol_samples, tol_logjoint)."""
    args = (case['Z'], case['w'], case['start'], case['inv_mass'], case['eps'], case['L'], case['E'], case['logU'])
    ref = hmc_run(*args, dtype=np.longdouble)
    f64 = hmc_run(*args, dtype=np.float64)
    assert np.array_equal(ref['accept'], f64['accept'])
    return ref, max(64. * rel_dev(f64['samples'], ref['samples']), 1e-13), max(64. * rel_dev(f64['logjoint'], ref['logjoint']), 1e-13)


# ------------------------------------------------------------------ a stand-in engine for samplers.logistic_hmc (no GPU)
class NumpyHMCEngine:
    """samplers.logistic_hmc's engine protocol (begin / auto_chunk / chunk / end) on the float64 restatement.  It records the
    step of every chunk and lets a test dictate the accept flags it reports."""

    def __init__(self, Z, wts, forced_accept=None):
        self.Z, self.w = np.asarray(Z, dtype=np.float64), wts
        self.steps, self.sizes, self.forced = [], [], forced_accept
        self.ended = False

    def begin(self, start, inv_mass, n_leapfrog, n_iter):
        self.th, self.im, self.L, self.n_iter, self.done = start.copy(), inv_mass.copy(), n_leapfrog, n_iter, 0

    def auto_chunk(self, c, d):
        return 7

    def chunk(self, normals, log_u, step):
        k = normals.shape[0]
        assert self.done + k <= self.n_iter
        self.steps.append(step)
        self.sizes.append(k)
        out = hmc_run(self.Z, self.w, self.th, self.im, step, self.L, normals, log_u, dtype=np.float64)
        self.th = out['samples'][-1].copy()
        self.done += k
        acc = out['accept'].astype(np.int32)
        if self.forced is not None:
            acc = (np.random.RandomState(len(self.steps)).rand(*acc.shape) < self.forced[len(self.steps) - 1]).astype(np.int32)
        return out['samples'], out['logjoint'], acc

    def end(self):
        self.ended = True
        return None


# ------------------------------------------------------------------ the host build of csrc/bc_hmc_dev.h
def build_harness(outdir, extra=()):
    exe = os.path.join(str(outdir), 'hmc_harness')
    cmd = ['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-Wall', '-Werror'] + list(extra) \
        + [os.path.join(ROOT, 'tests', 'hmc_harness.cpp'), '-o', exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def run_harness(exe, case, tmp):
    """The host build of the leapfrog / accept arithmetic (around a plain C++ rows pass) on a case: dict like hmc_run's."""
    Z, w = case['Z'], case['w']
    n, d = Z.shape
    T, c, _ = case['E'].shape
    w = np.ones(n) if w is None else w
    head = np.array([n, d, c, case['L'], T, case['eps']], dtype=np.float64)
    parts = [head, Z.ravel(), w, case['start'].ravel(), case['inv_mass'], case['E'].ravel(), case['logU'].ravel()]
    fin, fout = os.path.join(str(tmp), 'hmc_in.bin'), os.path.join(str(tmp), 'hmc_out.bin')
    np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in parts]).tofile(fin)
    out = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stderr == '', (out.returncode, out.stderr[-2000:])
    res = np.fromfile(fout)
    status = int(res[0])
    if status != 0:
        assert res.size == 1
        return dict(status=status)
    o = 1
    samples = res[o:o + T * c * d].reshape(T, c, d)
    o += T * c * d
    lj = res[o:o + T * c].reshape(T, c)
    o += T * c
    acc = res[o:o + T * c].reshape(T, c) != 0
    assert o + T * c == res.size
    return dict(status=0, samples=samples, logjoint=lj, accept=acc)
