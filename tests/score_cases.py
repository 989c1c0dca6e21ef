"""The cases the tests of the held-out scorer share (k_lr_score, include/beta_cores_score.h, csrc/bc_score_dev.h): the case table,
the input condition, the long-double restatement with THE tolerance (one definition, used by the CPU and the GPU tests), and the
build of tests/score_harness.cpp.  Test infrastructure only: the product never imports this module.

THE TOLERANCE of ll[t] = sum_n ll(-s_n), s_n = z_n . theta_t, against the long-double value; u = 2^-53, gamma_k = k u / (1 - k u);
the device code is built with -ffp-contract=off.  Derived, not chosen:

  contraction   s over D' terms (D' = D padded to a multiple of 4; any association: MFMA k-steps or one fma chain):
                    bm = gamma_D' sum_i |z_i theta_i|
  one term      ll(m) = m < 100 ? -(max(m, 0) + log1p(exp(-|m|))) : -m, |d ll / d m| <= 1:
                    bt = bm + 6 u log1p(e^-|m|) + u |ll| + 3.8e-44
                the evaluation error 6 u log1p(e^-|m|) (exp to 1.5 ulp, carried through log1p, and log1p's own) and the u |ll| of
                the one addition are the constants of the K1 element-wise bound for the same function (tests/k1_cases.py,
                csrc/bc_k1_math.h); 3.8e-44 > log1p(e^-100) covers the branch, whose far side drops that term.
  row sum       Nt terms in a fixed order (any order obeys it):   sum_n bt + gamma_Nt sum_n |ll_n|
  second-order terms: one final factor 1.01, as in the K1 bound.

The counts must be EQUAL, under THE INPUT CONDITION (check_condition, asserted on the CPU inside the tests): over all
(row, theta) pairs of a case either the row is exactly zero or |z . theta| >= 1e-9 in long double, AND |z . theta| > 2 bm, the
worst-case error of the contraction of that very pair (for the unscaled thetas bm < 1e-11; for the thetas scaled by 3000 at D = 256
the worst-case count reaches 1e-8, where the margins are of the order 100 and more).  Random normal cases meet both; that was
confirmed when the table was built."""
import functools
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
LD = np.longdouble
LONGDOUBLE_OK = bool(np.finfo(np.longdouble).eps <= 2.0 ** -63)
MIN_MARGIN = 1e-9

# (name, Nt, D, T, seed, float32 rows).  X = randn(Nt, D), y = +-1, thetas = randn(T, D) * 0.7.  Where Nt >= 3 the rows 0 and 1 are
# all zero with y = +1 and y = -1 (the tie: predicted +1); where T >= 4, theta 1 is scaled by 150 and theta 2 by 3000: margins on
# both sides of +-100 and beyond +-745, where exp(-|m|) underflows (check_condition asserts that the table as a whole has both).
# Covered: Nt in {1, 15, 16, 17, 65, 300} (one row, both sides of a tile, more than one staged chunk of 32 / 64 rows), D in
# {1, 3, 4, 5, 16, 129, 256} and one D inside every other instance of the kernel (20, 40, 100: the template's 2, 4 and 8 column
# blocks), T in {1, 15, 16, 17, 33, 1025} (both sides of a wave's 16 thetas, more than a block's 128), float32 rows.
CASES = [
    ('n1_d1_t1', 1, 1, 1, 61, False),
    ('n15_d3_t15', 15, 3, 15, 62, False),
    ('n16_d4_t16', 16, 4, 16, 63, False),
    ('n17_d5_t17', 17, 5, 17, 64, False),
    ('n65_d16_t33', 65, 16, 33, 65, False),
    ('n300_d129_t1025', 300, 129, 1025, 66, False),
    ('n65_d256_t17', 65, 256, 17, 67, False),
    ('n300_d5_t33_f32', 300, 5, 33, 68, True),
    ('n33_d20_t17', 33, 20, 17, 69, False),
    ('n40_d40_t20', 40, 40, 20, 70, False),
    ('n70_d100_t130', 70, 100, 130, 71, False),
    ('n17_d129_t16_f32', 17, 129, 16, 72, True),
]
NAMES = [c[0] for c in CASES]


@functools.lru_cache(maxsize=None)
def make_case(name):
    """dict(name, X, Y, thetas, f32): X float64 (float32 for a float32 case), Y float64 in {-1, +1}, thetas float64."""
    _, nt, d, t, seed, f32 = [c for c in CASES if c[0] == name][0]
    rng = np.random.RandomState(seed)
    X = rng.randn(nt, d)
    Y = np.where(rng.rand(nt) < 0.5, 1., -1.)
    th = rng.randn(t, d) * 0.7
    if nt >= 3:
        X[0], X[1] = 0., 0.
        Y[0], Y[1] = 1., -1.
    if t >= 4:
        th[1] *= 150.
        th[2] *= 3000.
    if f32:
        X = X.astype(np.float32)
    for a in (X, Y, th):
        a.setflags(write=False)
    return dict(name=name, X=X, Y=Y, thetas=th, f32=f32)


def gamma(k):
    return k * U / (1. - k * U)


def restate(X, Y, thetas):
    """The long-double restatement: dict(correct [T] int64, ll [T] long double, tol [T] float64, margin: the smallest |z . theta| over
    the pairs whose row is not all zero (inf if there is none), s: the margins Nt x T)."""
    Z = (np.asarray(Y, dtype=LD)[:, None] * np.asarray(X).astype(LD))
    th = np.asarray(thetas).astype(LD)
    s = Z.dot(th.T)
    m = -s
    soft = np.log1p(np.exp(-np.abs(m)))
    ll = -(np.maximum(m, 0) + soft)
    yy = np.asarray(Y)[:, None]
    correct = (((yy > 0) & (s >= 0)) | ((yy < 0) & (s > 0))).sum(axis=0).astype(np.int64)
    d, nt = Z.shape[1], Z.shape[0]
    dpad = ((d + 3) // 4) * 4
    bm = gamma(dpad) * np.abs(Z).dot(np.abs(th).T)
    bt = bm + 6. * U * soft + U * np.abs(ll) + 3.8e-44
    tol = 1.01 * (bt.sum(axis=0) + gamma(nt) * np.abs(ll).sum(axis=0))
    nz = np.any(np.asarray(X) != 0, axis=1)
    margin = float(np.abs(s[nz]).min()) if nz.any() else np.inf
    sure = bool(np.all(np.abs(s[nz]) > 2. * bm[nz]))
    return dict(correct=correct, ll=ll.sum(axis=0), tol=tol.astype(np.float64), margin=margin, sure=sure, s=s)


@functools.lru_cache(maxsize=None)
def reference(name):
    """restate() of a case: computed once, shared, never modified."""
    c = make_case(name)
    return restate(c['X'], c['Y'], c['thetas'])


def check_condition(ref):
    """THE INPUT CONDITION of the module docstring, on a restatement."""
    assert ref['margin'] >= MIN_MARGIN and ref['sure'], ref['margin']


def check_table():
    """What the table as a whole must hold: every case meets the input condition; margins on both sides of the branch at +-100 and
    beyond +-745 occur with both signs; both kinds of all-zero row occur."""
    lo = hi = lon = hin = False
    for n in NAMES:
        ref = reference(n)
        check_condition(ref)
        s = ref['s'].astype(np.float64)
        lo |= bool(((s > 100) & (s < 745)).any())
        lon |= bool(((s < -100) & (s > -745)).any())
        hi |= bool((s > 745).any())
        hin |= bool((s < -745).any())
    assert lo and hi and lon and hin


def compare(correct, ll, ref, label=''):
    """Counts equal; ll within THE tolerance of the long-double value.  Prints the worst share of the tolerance."""
    assert np.array_equal(np.asarray(correct, dtype=np.int64), ref['correct']), label
    err = np.abs(np.asarray(ll).astype(LD) - ref['ll']).astype(np.float64)
    share = float((err / ref['tol']).max())
    print('%s: worst |ll - reference| / tolerance = %.3g (largest tolerance %.3g)' % (label, share, ref['tol'].max()))
    assert np.all(err <= ref['tol']), (label, share)
    return share


# ------------------------------------------------------------------ the host build of csrc/bc_score_dev.h
def build_harness(outdir, extra=()):
    exe = os.path.join(str(outdir), 'score_harness')
    cmd = ['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-Wall', '-Werror'] + list(extra) \
        + [os.path.join(ROOT, 'tests', 'score_harness.cpp'), '-o', exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def run_harness(exe, X, Y, thetas, tmp, expect=0):
    """The host build on one case: (correct [T] int64, ll [T]); expect: the exit status wanted (2: the shape is refused)."""
    Z = np.asarray(Y, dtype=np.float64)[:, None] * np.asarray(X, dtype=np.float64)
    th = np.asarray(thetas, dtype=np.float64)
    nt, d = Z.shape
    t = th.shape[0]
    fin, fout = os.path.join(str(tmp), 'score_in.bin'), os.path.join(str(tmp), 'score_out.bin')
    np.concatenate([np.array([nt, d, t], dtype=np.float64), Z.ravel(), np.asarray(Y, dtype=np.float64).ravel(), th.ravel()]).tofile(fin)
    out = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert out.returncode == expect and out.stderr == '', (out.returncode, out.stderr[-2000:])
    if expect:
        return None
    res = np.fromfile(fout)
    assert res.size == 2 * t
    return res[:t].astype(np.int64), res[t:]
