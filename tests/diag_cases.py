"""Reference, derived error bounds and planted inputs for the tests of the chain summary (include/beta_cores_diag.h: posterior mean
and covariance, split-R-hat and Geyer's ESS of P x n x C x D draws); no test in here.  tests/test_diag_cases_cpu.py holds the cases
themselves, tests/test_diag_harness_cpu.py the host build of csrc/bc_diag_dev.h, tests/test_gpu_diag.py the device.

THE REFERENCE (summary) restates the header's definitions in np.longdouble, straight from the text: h = n // 2, the 2 C sequences
are every chain's first h and last h kept draws, mean and cov (ddof = 1) over all n C draws, m_s, v_s, W, Bh, varplus, rhat,
a_s(t), rho_t for t <= L = min(max_lag, h - 1), the pairs P_k, K, the monotone P'_k, tau and ess.  The sums run over the draws
less the coordinate's first draw, y = x - x_0, as the header says they are formed: that changes no quantity, is exact in long
double for the inputs here, and keeps the reference's own rounding of a coordinate of mean 1e8 below the bounds.  Run with
dtype=np.float64 it is NumPy's float64 evaluation of the same formulas (the CPU test holds it inside the bounds).

THE BOUNDS (bounds) are first order, u = 2^-53, with every input error propagated; y = fl(x - x_0) carries u |y|:
    a sum of L terms in any order, then a division             (L + 1) u sum |terms| / L       (+ the terms' own errors)
    mean = x_0 + ybar                                          min(u |mean|, |ybar| + e_ybar) + e_ybar,   e_ybar = (N + 1) u mean |y|
    m_s (of y)                                                 e_m = (h + 1) u mean_s |y|
    v_s: t_i = y_i - m_s carries u |y_i| + u |t_i| and the common e_m, which enters at second order (sum_i t_i = 0):
                                                               (2 u sum |t| |y| + (h + 4) u sum t^2 + h e_m^2) / (h - 1) + u v_s
    W                                                          (S + 1) u W + mean_s e_v
    Bh: d_s = m_s - mbar carries e_m + e_mbar + u |d_s|        (sum (2 |d| e_d + e_d^2) + (S + 2) u sum d^2) / (S - 1) + u Bh
    varplus                                                    3 u varplus + e_W + e_Bh
    a_s(t): the common e_m enters at FIRST order through the partial sums A1 = sum_{i < h - t} t_i and A2 = sum_{i >= t} t_i:
            (e_m (|A1| + |A2|) + (h - t) e_m^2 + sum (|t_i| eps_{i+t} + |t_{i+t}| eps_i) + (h - t + 2) u sum |t_i t_{i+t}|) / h + u |a_s|
    abar(t)                                                    (S + 1) u mean |a_s| + mean e_a
    rho_t = 1 - (W - abar) / varplus                           the difference, the quotient (u |q| + (e_num + |q| e_vp) / (vp - e_vp)), the difference
    cov: c_i = x_i - mean carries u |c_i|; the means' errors enter at second order
                                                               ((N + 4) u sum |c_j c_l| + N e_mean_j e_mean_l) / (N - 1) + u |cov|
The factor 1.01 covers the second order and the reference's own rounding.  Derived, not tuned.  ESS and rhat are held to the
device's OWN rho and moments (ess_from_rho and the bound of tests/test_gpu_diag.py), so the truncation index never has to agree
between two roundings.

THE PLANTED INPUTS (make_problem).  Coordinates are AR(1) chains of differing scale, offset and correlation, neighbours mixed so
that the covariance is dense.  In the first, a middle and the last coordinate of every 16-wide tile (j % 16 in 0, 7, 15) one of
five kinds is planted, cycling with the position and the problem's number so that every kind meets every place:
    const   every draw 0.1 (p + 1) + 0.2: rhat and ess NaN, cov row and column exactly 0
    big     mean 1e8, unit spread
    anti    x_i = a_c (-1)^i, a_c per chain: P_0 = 1 + rho_1 = -1 / (h (h - 1)) for the even h used here, far outside rounding;
            K = 0, ess NaN
    ar9     AR(1) with phi = 0.9
    shift   iid normal draws, chain 0 shifted by five standard deviations (rhat > 1.5 where C >= 2)
"""
import os
import subprocess

import numpy as np

from sweep_cases import LD, LONGDOUBLE_OK, LONGDOUBLE_WHY, U      # noqa: F401  (the guard is sweep_cases.py's)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTOR = 1.01
KINDS = ('const', 'big', 'anti', 'ar9', 'shift')
COV_CHUNK = 2048           # BC_DIAG_COV_CHUNK
MAX_WORK = 1 << 29         # BC_DIAG_MAX_WORK_DOUBLES
# (P, n, C, D) of the device tests: the smallest h, odd n, one chain, D on both sides of a 16-wide tile and of 128, the limits
SHAPES = [(3, 4, 1, 1), (2, 5, 2, 17), (5, 64, 16, 9), (2, 200, 16, 128), (1, 37, 3, 129), (1, 12, 64, 256)]


# ------------------------------------------------------------------ planted inputs
def planted_kinds(p, d):
    """{coordinate: kind} of problem number p"""
    pos = [j for j in range(d) if j % 16 in (0, 7, 15)]
    return {j: KINDS[(i + p) % len(KINDS)] for i, j in enumerate(pos)}


def _ar1(rng, n, c, phi):
    x = np.empty((n, c))
    x[0] = rng.randn(c)
    for i in range(1, n):
        x[i] = phi * x[i - 1] + np.sqrt(1. - phi * phi) * rng.randn(c)
    return x


def make_problem(p, n, c, d, seed=0, plant=True):
    """n x C x D draws of problem number p (float64)"""
    rng = np.random.RandomState(71000 + 1000 * seed + 37 * p + n + 3 * c + 7 * d)
    kinds = planted_kinds(p, d) if plant else {}
    x = np.empty((n, c, d))
    prev = None
    for j in range(d):
        k = kinds.get(j)
        if k == 'const':
            x[:, :, j] = 0.1 * (p + 1) + 0.2
        elif k == 'big':
            x[:, :, j] = 1e8 + _ar1(rng, n, c, 0.3)
        elif k == 'anti':
            amp = 1. + 0.5 * rng.rand(c)
            x[:, :, j] = amp[None, :] * ((-1.) ** np.arange(n))[:, None]
        elif k == 'ar9':
            x[:, :, j] = _ar1(rng, n, c, 0.9)
        elif k == 'shift':
            x[:, :, j] = rng.randn(n, c)
            x[:, 0, j] += 5.
        else:
            col = 10. ** rng.uniform(-1., 1.) * _ar1(rng, n, c, rng.uniform(0., 0.6)) + 3. * rng.randn()
            if prev is not None:
                col = col + 0.5 * prev
            x[:, :, j] = prev = col
    return x


def make_batch(shape, seed=0):
    P, n, c, d = shape
    return np.stack([make_problem(p, n, c, d, seed) for p in range(P)])


# ------------------------------------------------------------------ the restatement
def lag_of(n, max_lag=None):
    h = n // 2
    return h - 1 if max_lag is None else min(int(max_lag), h - 1)


def sequences(src, n, c):
    """[2 C, h, D]: sequence 2 c = chain c's first h draws, 2 c + 1 its last h"""
    h = n // 2
    return np.stack([src[:h, k] if half == 0 else src[n - h:, k] for k in range(c) for half in (0, 1)])


def ess_from_rho(rho, n_seq_draws, dtype=LD):
    """(ess, truncated, K, tau, sum |P'_k|) from rho_0 .. rho_L of ONE coordinate, by the header's rule; NaN entries (lags the
    device never evaluated) end the sum like any pair that is not > 0"""
    rho = np.asarray(rho, dtype=dtype)
    L = rho.shape[0] - 1
    pairs = (L + 1) // 2
    total, prev, K, full = dtype(0), dtype(0), 0, 1
    for k in range(pairs):
        pk = rho[2 * k] + rho[2 * k + 1]
        if not pk > 0:
            full = 0
            break
        prev = pk if k == 0 or pk < prev else prev
        total = total + prev
        K += 1
    tau = dtype(-1) + dtype(2) * total
    ess = dtype(n_seq_draws) / tau if K > 0 else dtype(np.nan)
    return ess, full, K, tau, total


def summary(x, max_lag=None, dtype=LD):
    """The definitions for one problem x [n, C, D]; a dict of mean [D], cov [D, D], W, varplus, rhat, ess [D], rho [L + 1, D],
    truncated, K [D] (ints)"""
    with np.errstate(invalid='ignore', divide='ignore'):
        x = np.asarray(x, dtype=dtype)
        n, c, d = x.shape
        h, N, S = n // 2, n * c, 2 * c
        flat = x.reshape(N, d)
        y = x - x[0, 0]
        mean = x[0, 0] + y.reshape(N, d).sum(axis=0) / dtype(N)
        seq = sequences(y, n, c)
        cen = flat - mean
        cov = cen.T.dot(cen) / dtype(N - 1)
        m = seq.sum(axis=1) / dtype(h)
        t = seq - m[:, None, :]
        v = (t * t).sum(axis=1) / dtype(h - 1)
        W = v.sum(axis=0) / dtype(S)
        mm = m.sum(axis=0) / dtype(S)
        Bh = ((m - mm) ** 2).sum(axis=0) / dtype(S - 1)
        vp = dtype(h - 1) / dtype(h) * W + Bh
        rhat = np.where(W == 0, dtype(np.nan), np.sqrt(vp / np.where(W == 0, dtype(1), W)))
        L = lag_of(n, max_lag)
        rho = np.ones((L + 1, d), dtype=dtype)
        for lag in range(1, L + 1):
            ab = ((t[:, :h - lag] * t[:, lag:]).sum(axis=1) / dtype(h)).sum(axis=0) / dtype(S)
            rho[lag] = dtype(1) - (W - ab) / vp
        ess, trunc, K = np.empty(d, dtype=dtype), np.zeros(d, dtype=np.int64), np.zeros(d, dtype=np.int64)
        for j in range(d):
            ess[j], trunc[j], K[j] = ess_from_rho(rho[:, j], S * h, dtype)[:3]
    return dict(mean=mean, cov=cov, W=W, varplus=vp, rhat=rhat, ess=ess, rho=rho, truncated=trunc, K=K, L=L)


# ------------------------------------------------------------------ the bounds
def bounds(x, max_lag=None):
    """First-order bounds (module docstring) on |computed - reference| for mean [D], cov [D, D], W, varplus [D] and rho [L + 1, D]
    of one problem, in np.longdouble"""
    with np.errstate(invalid='ignore', divide='ignore'):
        xl = np.asarray(x, dtype=LD)
        n, c, d = xl.shape
        h, N, S = n // 2, n * c, 2 * c
        u = LD(U)
        y = xl - xl[0, 0]
        flat = xl.reshape(N, d)
        mean = flat.sum(axis=0) / N
        e_ybar = (N + 1) * u * np.abs(y).reshape(N, d).sum(axis=0) / N
        # (the last addition x_0 + ybar errs by at most |ybar| too: x_0 is itself a float64; a constant coordinate's mean is exact)
        e_mean = np.minimum(u * np.abs(mean), np.abs(y.reshape(N, d).sum(axis=0) / N) + e_ybar) + e_ybar
        cen = flat - mean
        cov = cen.T.dot(cen) / (N - 1)
        e_cov = ((N + 4) * u * np.abs(cen).T.dot(np.abs(cen)) + N * np.outer(e_mean, e_mean)) / (N - 1) + u * np.abs(cov)
        seq = sequences(y, n, c)
        m = seq.sum(axis=1) / h
        e_m = (h + 1) * u * np.abs(seq).sum(axis=1) / h                         # [S, D]
        t = seq - m[:, None, :]
        eps = u * np.abs(seq) + u * np.abs(t)                                   # of t_i, besides the common e_m
        v = (t * t).sum(axis=1) / (h - 1)
        e_v = (2 * (np.abs(t) * eps).sum(axis=1) + (h + 4) * u * (t * t).sum(axis=1) + h * e_m * e_m) / (h - 1) + u * v
        W = v.sum(axis=0) / S
        e_W = (S + 1) * u * W + e_v.sum(axis=0) / S
        mm = m.sum(axis=0) / S
        e_mm = (S + 1) * u * np.abs(m).sum(axis=0) / S + e_m.sum(axis=0) / S
        dd = m - mm
        e_d = e_m + e_mm + u * np.abs(dd)
        Bh = (dd * dd).sum(axis=0) / (S - 1)
        e_Bh = ((2 * np.abs(dd) * e_d + e_d * e_d).sum(axis=0) + (S + 2) * u * (dd * dd).sum(axis=0)) / (S - 1) + u * Bh
        vp = LD(h - 1) / h * W + Bh
        e_vp = 3 * u * vp + e_W + e_Bh
        L = lag_of(n, max_lag)
        e_rho = np.zeros((L + 1, d), dtype=LD)
        for lag in range(1, L + 1):
            a, b = t[:, :h - lag], t[:, lag:]
            prod = a * b
            a_s = prod.sum(axis=1) / h
            e_a = (e_m * (np.abs(a.sum(axis=1)) + np.abs(b.sum(axis=1))) + (h - lag) * e_m * e_m
                   + (np.abs(a) * eps[:, lag:] + np.abs(b) * eps[:, :h - lag]).sum(axis=1)
                   + (h - lag + 2) * u * np.abs(prod).sum(axis=1)) / h + u * np.abs(a_s)
            ab = a_s.sum(axis=0) / S
            e_ab = (S + 1) * u * np.abs(a_s).sum(axis=0) / S + e_a.sum(axis=0) / S
            num = W - ab
            e_num = e_W + e_ab + u * np.abs(num)
            q = num / vp
            e_q = u * np.abs(q) + (e_num + np.abs(q) * e_vp) / (vp - e_vp)
            e_rho[lag] = e_q + u * np.abs(1 - q)
        F = LD(FACTOR)
    return dict(mean=F * e_mean, cov=F * e_cov, W=F * e_W, varplus=F * e_vp, rho=F * e_rho)


def scales(ref):
    """what a bound is compared with in the cap of the CPU test: the quantity's own size (a coordinate's spread for its mean)"""
    sd = np.sqrt(np.diag(ref['cov']))
    return dict(mean=np.maximum(np.abs(ref['mean']), sd), cov=np.outer(sd, sd), W=ref['W'], varplus=ref['varplus'],
                rho=np.ones_like(ref['rho']))


def inside(got, ref, bound):
    """every entry of got within bound of ref (a NaN reference wants a NaN)"""
    got, ref, bound = np.asarray(got, dtype=LD), np.asarray(ref, dtype=LD), np.asarray(bound, dtype=LD)
    nan = np.isnan(ref)
    return bool(np.all(np.isnan(got[nan]))) and bool(np.all(np.abs(got[~nan] - ref[~nan]) <= bound[~nan]))


def worst(got, ref, bound):
    """the largest |got - ref| / bound over the entries with a positive bound (a figure to print)"""
    got, ref, bound = np.asarray(got, dtype=LD), np.asarray(ref, dtype=LD), np.asarray(bound, dtype=LD)
    ok = ~np.isnan(ref) & (bound > 0)
    return float((np.abs(got[ok] - ref[ok]) / bound[ok]).max()) if ok.any() else 0.


# ------------------------------------------------------------------ the closed form of the work space
def _even(k):
    return (k + 1) & ~1


def work_doubles(P, n, c, d, max_lag):
    """bc_diag_work_doubles as include/beta_cores_diag.h documents it (-1 outside the limits)"""
    if P < 1 or n < 4 or not 1 <= c <= 64 or not 1 <= d <= 256 or max_lag < 1 or n * c >= 1 << 31 or P * n * c * d > MAX_WORK:
        return -1
    L = min(max_lag, n // 2 - 1)
    t = (d + 15) // 16
    T, G, pd = t * (t + 1) // 2, (n * c + COV_CHUNK - 1) // COV_CHUNK, P * d
    total = 2 * _even(P * n * c * d) + _even(256 * P * G * T) + 3 * _even(pd) + _even(pd * d) + _even(2 * pd) + _even(pd * (L + 1)) \
        + _even((pd + 1) // 2) + _even((P + 1) // 2)
    return total if total <= MAX_WORK else -1


# ------------------------------------------------------------------ the host build of csrc/bc_diag_dev.h
def build_harness(outdir, extra=()):
    exe = os.path.join(str(outdir), 'diag_harness')
    cmd = ['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-Wall', '-Werror', '-Wno-unknown-pragmas'] + list(extra) \
        + [os.path.join(ROOT, 'tests', 'diag_harness.cpp'), '-o', exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def run_harness(exe, x, max_lag, tmp, staged=True):
    """the host build on one problem x [n, C, D]: a dict shaped like summary()'s, plus status"""
    n, c, d = x.shape
    L = lag_of(n, max_lag)
    fin, fout = os.path.join(str(tmp), 'diag_in.bin'), os.path.join(str(tmp), 'diag_out.bin')
    np.concatenate([np.array([n, c, d, max_lag if max_lag is not None else n, 1. if staged else 0.]),
                    np.asarray(x, dtype=np.float64).ravel()]).tofile(fin)
    out = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stderr == '', (out.returncode, out.stderr[-2000:])
    res = np.fromfile(fout)
    r, at = {'status': int(res[0]), 'L': L}, 1
    for k, shp in [('mean', (d,)), ('cov', (d, d)), ('W', (d,)), ('varplus', (d,)), ('rhat', (d,)), ('ess', (d,)), ('truncated', (d,)),
                   ('rho', (d, L + 1))]:
        cnt = int(np.prod(shp))
        r[k] = res[at:at + cnt].reshape(shp)
        at += cnt
    assert at == res.size
    r['rho'] = r['rho'].T
    return r


# ------------------------------------------------------------------ ESS and R-hat as functions of the rho and moments that came with them
def check_own(got, n, c, what):
    """got: a dict with ess, rhat, truncated, W, varplus [D] and rho [L + 1, D] of one problem, all from ONE evaluation (the device's
    or the host build's).  K, tau and ess are re-evaluated in long double from that rho: ess must lie within
    (2 K + 4) u (1 + 2 sum |P'_k|) / |tau| relative -- the K additions, the doubling, the subtraction and the division -- and the
    truncation flag must be the one that rho gives; rhat within 4 u of sqrt(varplus / W) of the returned moments (NaN at W = 0)."""
    h, S = n // 2, 2 * c
    d = np.asarray(got['ess']).shape[0]
    for j in range(d):
        e, full, K, tau, tot = ess_from_rho(np.asarray(got['rho'])[:, j], S * h)
        assert int(got['truncated'][j]) == full, '%s coordinate %d: truncated' % (what, j)
        if K == 0:
            assert np.isnan(got['ess'][j]), '%s coordinate %d: K = 0 wants NaN, got %r' % (what, j, got['ess'][j])
        else:
            rel = (2 * K + 4) * LD(U) * (1 + 2 * tot) / abs(tau)
            assert abs(LD(got['ess'][j]) - e) <= rel * abs(e), '%s coordinate %d: ess %r, from its rho %r' % (what, j, got['ess'][j], float(e))
        W, vp = LD(got['W'][j]), LD(got['varplus'][j])
        if W == 0:
            assert np.isnan(got['rhat'][j]), '%s coordinate %d: W = 0 wants NaN' % (what, j)
        else:
            r = np.sqrt(vp / W)
            assert abs(LD(got['rhat'][j]) - r) <= 4 * LD(U) * r, '%s coordinate %d: rhat' % (what, j)


def check_against_reference(got, x, max_lag, what, printer=None):
    """mean, cov, W, varplus and every rho that was evaluated within the derived bounds of the long-double restatement; prints the
    worst ratio per quantity before it asserts"""
    ref, b = summary(x, max_lag), bounds(x, max_lag)
    rho = np.asarray(got['rho'], dtype=LD)
    seen = ~np.isnan(rho)
    rr = np.where(seen, ref['rho'], LD(0))                     # (a lag the evaluation never reached is not compared)
    figures = []
    for k, g, r in (('mean', got['mean'], ref['mean']), ('cov', got['cov'], ref['cov']), ('W', got['W'], ref['W']),
                    ('varplus', got['varplus'], ref['varplus']), ('rho', np.where(seen, rho, LD(0)), rr)):
        figures.append('%s %.3f' % (k, worst(g, r, b[k])))
    (printer or print)('%s: |got - ref| / bound at most: %s' % (what, ', '.join(figures)))
    for k, g, r in (('mean', got['mean'], ref['mean']), ('cov', got['cov'], ref['cov']), ('W', got['W'], ref['W']),
                    ('varplus', got['varplus'], ref['varplus'])):
        assert inside(g, r, b[k]), '%s: %s is %.3g bounds from the reference' % (what, k, worst(g, r, b[k]))
    nanref = np.isnan(ref['rho'])
    assert np.all(np.isnan(rho[nanref])), '%s: rho of a coordinate without one' % what
    ok = seen & ~nanref
    assert np.all(np.abs(rho[ok] - ref['rho'][ok]) <= b['rho'][ok]), '%s: rho is %.3g bounds from the reference' % (what, worst(np.where(seen, rho, LD(0)), rr, b['rho']))
    # the lags that were evaluated are those the rule asks for: 0 .. 2 K + 1 where the sum stopped at pair K, every pair otherwise
    for j in range(rho.shape[1]):
        if nanref[1, j] if rho.shape[0] > 1 else False:
            continue
        K = ess_from_rho(rho[:, j], 1)[2]
        L = rho.shape[0] - 1
        pairs = (L + 1) // 2
        upto = 2 * pairs if K == pairs else 2 * K + 2
        assert np.all(seen[:upto, j]) and not np.any(seen[upto:, j]), '%s coordinate %d: lags evaluated' % (what, j)
    return ref
