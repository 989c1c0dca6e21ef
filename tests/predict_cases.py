"""The cases the tests of the linear-regression held-out scorer share (k_linreg_predict, include/beta_cores_predict.h,
csrc/bc_predict_dev.h): the case table, the exact cases, the long-double restatement with THE tolerance (one definition, used by
the CPU and the GPU tests), and the build of tests/predict_harness.cpp.  Test infrastructure only: the product never imports this.

What is computed, per held-out row [phi, y] and posterior (mu, F, noise, scale):

    m = phi . mu     v_j = (phi F)_j     q = sum_j v_j^2     var = noise + scale q     r = y - m
    term = -1/2 ((r^2 / var + log var) + log 2 pi)            ll = sum_n term_n         sse = sum_n r_n^2

THE TOLERANCE against the long-double values; u = 2^-53, gamma_k = k u / (1 - k u); the code is built with -ffp-contract=off.
Derived from the arithmetic, not chosen:

  mean          a contraction over D' terms (D' = D padded to a multiple of 4; any association -- the eight fma chains and their
                butterfly are at most D' operations deep):      bm = gamma_D' sum_k |phi_k mu_k|
  entries of V  the same for every column j (MFMA k-steps in any association):      e_j = gamma_D' sum_k |phi_k F_kj|
  q             the computed entry is v_j + delta_j, |delta_j| <= e_j, so its square is off by 2 |v_j| e_j + e_j^2; the square is
                rounded once and the DP = 16 ceil(D / 16) squares (the padding's are exact zeros) are added in the order the
                header fixes, which like any order obeys gamma_DP:
                    bq = sum_j (2 |v_j| e_j + e_j^2) + (u + gamma_DP) sum_j (|v_j| + e_j)^2
  var           one product and one addition:      bvar = scale bq + u scale (q + bq) + u (var + scale bq)
  residual      one subtraction:      br = bm + u (|r| + bm);      its square, rounded once:
                    br2 = 2 |r| br + br^2 + u (|r| + br)^2
  per-row term  with varlo = var - bvar > 0 (asserted) and r2hi = r^2 + br2:
                    the correctly rounded division      bdiv = br2 / varlo + r2hi bvar / (var varlo) + u r2hi / varlo
                    log                                 blog = bvar / varlo + 2 u (|log var| + bvar / varlo)
                        one ulp = 2 u relative: what tests/k1_cases.py counts for a libm call (log, pow, exp, sqrt); the host's log
                        and the device library's fp64 log are both within one ulp
                    the two additions and the rounded constant log 2 pi:
                        bterm = 1/2 (bdiv + blog + u |r^2 / var + log var| + u log 2 pi + u |r^2 / var + log var + log 2 pi|
                                     + u (bdiv + blog))          (the factor -1/2 is exact)
  row sums      Nt terms in a fixed order (any order obeys it):
                    tol_ll = sum_n bterm_n + gamma_Nt sum_n |term_n|          tol_sse = sum_n br2_n + gamma_Nt sum_n r_n^2
  second-order terms: one final factor 1.01 on every bound, as in the K1 bound.
The per-row outputs are held element-wise to 1.01 bm and 1.01 bvar: far sharper than the sums."""
import functools
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
LD = np.longdouble
LONGDOUBLE_OK = bool(np.finfo(np.longdouble).eps <= 2.0 ** -63)
HEADER = os.path.join(ROOT, 'beta_cores_amd', 'csrc', 'bc_predict_dev.h')


def _define(name):
    return int(re.search(r'^#define\s+%s\s+(\d+)' % name, open(HEADER).read(), flags=re.M).group(1))


R = _define('BC_PRED_ROWS_PER_BLOCK')            # rows of one posterior per block
MAX_DIM = _define('BC_PRED_MAX_DIM')
PANEL = _define('BC_PRED_PANEL')
STAGE_NARROW, STAGE_WIDE = 64, 32                # BC_PRED_STAGE_ROWS(d) at d <= PANEL and above it (check_table reads the macro)

# (name, Nt, D, T, seed, float32 rows, factor kind).  X = randn(Nt, D); mu_t = randn(D) / 2; F_t = randn(D, D) 0.3 / sqrt(D), 'lower':
# its lower triangle (not symmetric either way); y = X . mu_0 + 0.5 randn; noise_t = 0.3 + rand; scale_0 = 1, scale_1 = 0, the others
# 2 rand.  Covered: Nt in {1, 15, 16, 17}, one row more than a staged chunk (65 at D <= 128, 33 above), R - 1, R, R + 1, 2 R + 17;
# D in {1, 3, 4, 5, 16, 17, 128, 129, 256, 257, 512} and one D inside every other instance of the kernel (40: the template's 4 column
# blocks, 100: its 8, 300: the panelled instance with a partial last panel); T in {1, 2, 17}; float32 rows; both kinds of factor.
CASES = [
    ('n1_d1_t1', 1, 1, 1, 81, False, 'full'),
    ('n15_d3_t2', 15, 3, 2, 82, False, 'lower'),
    ('n16_d4_t17', 16, 4, 17, 83, False, 'full'),
    ('n17_d5_t2', 17, 5, 2, 84, False, 'lower'),
    ('n65_d16_t17', 65, 16, 17, 85, False, 'full'),
    ('nRm1_d17_t2', R - 1, 17, 2, 86, False, 'lower'),
    ('nR_d40_t1', R, 40, 1, 87, False, 'full'),
    ('nRp1_d100_t2_f32', R + 1, 100, 2, 88, True, 'full'),
    ('n2Rp17_d128_t2', 2 * R + 17, 128, 2, 89, False, 'lower'),
    ('n33_d129_t2', 33, 129, 2, 90, False, 'full'),
    ('nRp1_d256_t1', R + 1, 256, 1, 91, False, 'lower'),
    ('n65_d257_t2_f32', 65, 257, 2, 92, True, 'full'),
    ('n17_d300_t17', 17, 300, 17, 93, False, 'full'),
    ('nRp1_d512_t2', R + 1, 512, 2, 94, False, 'full'),
]
NAMES = [c[0] for c in CASES]


@functools.lru_cache(maxsize=None)
def make_case(name):
    """dict(name, Z [Nt][D + 1] (float32 for a float32 case), mu [T][D], F [T][D][D], noise [T], scale [T], f32)."""
    _, nt, d, t, seed, f32, kind = [c for c in CASES if c[0] == name][0]
    rng = np.random.RandomState(seed)
    X = rng.randn(nt, d)
    mu = rng.randn(t, d) * 0.5
    F = rng.randn(t, d, d) * (0.3 / np.sqrt(d))
    if kind == 'lower':
        F = np.tril(F)
    y = X.dot(mu[0]) + 0.5 * rng.randn(nt)
    noise = 0.3 + rng.rand(t)
    scale = 2. * rng.rand(t)
    scale[0] = 1.
    if t >= 2:
        scale[1] = 0.
    Z = np.hstack((X, y[:, None]))
    if f32:
        Z = Z.astype(np.float32)
    for a in (Z, mu, F, noise, scale):
        a.setflags(write=False)
    return dict(name=name, Z=Z, mu=mu, F=F, noise=noise, scale=scale, f32=f32)


def gamma(k):
    return k * U / (1. - k * U)


def log_2pi():
    return np.log(LD(8) * np.arctan(LD(1)))


def restate(Z, mu, F, noise, scale):
    """The long-double restatement and THE tolerance: dict(ll, sse [T] long double; mean, var [T][Nt] long double; tol_ll, tol_sse [T],
    tol_mean, tol_var [T][Nt] float64)."""
    Z = np.asarray(Z).astype(LD)
    phi, y = Z[:, :-1], Z[:, -1]
    mu, F = np.atleast_2d(np.asarray(mu)).astype(LD), np.asarray(F).astype(LD)
    if F.ndim == 2:
        F = F[None]
    T, nt, d = mu.shape[0], phi.shape[0], phi.shape[1]
    noise = np.broadcast_to(np.asarray(noise, dtype=np.float64), (T,)).astype(LD)
    scale = np.broadcast_to(np.asarray(scale, dtype=np.float64), (T,)).astype(LD)
    dk, dp = ((d + 3) // 4) * 4, ((d + 15) // 16) * 16
    l2pi = log_2pi()
    aphi = np.abs(phi)
    out = dict((k, []) for k in ('ll', 'sse', 'mean', 'var', 'tol_ll', 'tol_sse', 'tol_mean', 'tol_var'))
    for t in range(T):
        m = phi.dot(mu[t])
        bm = gamma(dk) * aphi.dot(np.abs(mu[t]))
        v = phi.dot(F[t])
        e = gamma(dk) * aphi.dot(np.abs(F[t]))
        q = (v * v).sum(axis=1)
        av = np.abs(v)
        bq = (2. * av * e + e * e).sum(axis=1) + (U + gamma(dp)) * ((av + e) ** 2).sum(axis=1)
        var = noise[t] + scale[t] * q
        bvar = scale[t] * bq + U * scale[t] * (q + bq) + U * (var + scale[t] * bq)
        r = y - m
        br = bm + U * (np.abs(r) + bm)
        r2 = r * r
        br2 = 2. * np.abs(r) * br + br * br + U * (np.abs(r) + br) ** 2
        varlo = var - bvar
        assert np.all(varlo > 0), 'the variance is not separated from 0 by its own bound'
        r2hi = r2 + br2
        bdiv = br2 / varlo + r2hi * bvar / (var * varlo) + U * r2hi / varlo
        lv = np.log(var)
        blog = bvar / varlo + 2. * U * (np.abs(lv) + bvar / varlo)
        s1 = r2 / var + lv
        term = -0.5 * (s1 + l2pi)
        bterm = 0.5 * (bdiv + blog + U * np.abs(s1) + U * l2pi + U * np.abs(s1 + l2pi) + U * (bdiv + blog))
        out['ll'].append(term.sum())
        out['sse'].append(r2.sum())
        out['mean'].append(m)
        out['var'].append(var)
        out['tol_ll'].append(1.01 * (bterm.sum() + gamma(nt) * np.abs(term).sum()))
        out['tol_sse'].append(1.01 * (br2.sum() + gamma(nt) * r2.sum()))
        out['tol_mean'].append(1.01 * bm)
        out['tol_var'].append(1.01 * bvar)
    res = dict((k, np.array(a)) for k, a in out.items())
    for k in ('tol_ll', 'tol_sse', 'tol_mean', 'tol_var'):
        res[k] = res[k].astype(np.float64)
    return res


@functools.lru_cache(maxsize=None)
def reference(name):
    """restate() of a case: computed once, shared, never modified."""
    c = make_case(name)
    return restate(c['Z'], c['mu'], c['F'], c['noise'], c['scale'])


def check_table():
    """What the table as a whole must hold (the issue's list), read against the header's constants."""
    src = open(HEADER).read()
    assert re.search(r'#define BC_PRED_STAGE_ROWS\(d\) \(\(d\) <= BC_PRED_PANEL \? %d : %d\)' % (STAGE_NARROW, STAGE_WIDE), src)
    nts = set((c[1], c[2] > PANEL) for c in CASES)
    assert set(n for n, _ in nts) >= {1, 15, 16, 17, R - 1, R, R + 1, 2 * R + 17}
    assert (STAGE_NARROW + 1, False) in nts and (STAGE_WIDE + 1, True) in nts
    ds = set(c[2] for c in CASES)
    assert ds >= {1, 3, 4, 5, 16, 17, 128, 129, 256, 257, 512} and max(ds) == MAX_DIM
    assert any(32 < d <= 64 for d in ds) and any(64 < d < 128 for d in ds) and any(257 < d < 512 and d % 128 for d in ds)
    assert set(c[3] for c in CASES) == {1, 2, 17}
    assert any(c[5] for c in CASES) and set(c[6] for c in CASES) == {'full', 'lower'}
    for n in NAMES:
        c = make_case(n)
        assert c['scale'][0] == 1. and (len(c['scale']) < 2 or c['scale'][1] == 0.) and np.all(c['noise'] > 0)
        assert not np.allclose(c['F'][0], c['F'][0].T) or c['F'].shape[1] == 1


def compare(ll, sse, ref, label='', mean=None, var=None):
    """Sums within THE tolerance of the long-double values, the per-row outputs (when given) element-wise within theirs.  Prints
    the worst shares of the tolerance before it asserts."""
    shares = {}
    for key, got in (('ll', ll), ('sse', sse), ('mean', mean), ('var', var)):
        if got is None:
            continue
        err = np.abs(np.asarray(got).astype(LD) - ref[key]).astype(np.float64)
        tol = ref['tol_' + key]
        with np.errstate(divide='ignore', invalid='ignore'):
            sh = np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0.))
        shares[key] = (float(sh.max()), bool(np.all(err <= tol)))
    print('%s: worst |device - reference| / tolerance: %s (largest ll tolerance %.3g)'
          % (label, ', '.join('%s %.3g' % (k, s[0]) for k, s in shares.items()), ref['tol_ll'].max()))
    for k, s in shares.items():
        assert s[1], (label, k, s[0])
    return shares


# ------------------------------------------------------------------ exact cases: no tolerance
def exact_zero_factor():
    """factor = 0: var == noise bit for bit (a non-trivial mu, rows and noise).  (Z, mu, F, noise, scale)."""
    rng = np.random.RandomState(7)
    nt, d, t = 70, 37, 3
    Z = rng.randn(nt, d + 1)
    return Z, rng.randn(t, d), np.zeros((t, d, d)), 0.1 + rng.rand(t), np.array([1., 0., 3.5])


def exact_unit_rows(d):
    """Unit rows phi = e_k, k = 0 .. D - 1, a lower-triangular F with small-integer entries and scale = 1:
    var == noise + sum_j F[k][j]^2 and mean == mu_k bit for bit; a transposed F fails it.  (Z, mu, F, noise, scale, want_mean, want_var)."""
    rng = np.random.RandomState(1000 + d)
    F = np.tril(rng.randint(-3, 4, size=(d, d)).astype(np.float64))
    if d > 1:
        F[d - 1, 0] = 3.                                   # (the corner that a transposition moves is never zero)
    mu = rng.randn(1, d)
    Z = np.hstack((np.eye(d), rng.randn(d, 1)))
    noise = np.array([0.37])
    want_var = noise[0] + (F * F).sum(axis=1)
    return Z, mu, F[None], noise, np.array([1.]), mu[0].copy(), want_var


def exact_single_row():
    """One row with y = mean exactly: a unit row e_k, so that the mean is mu_k bit for bit, and row k of F a single -1 with
    noise = scale = 1/2, so that var == 1 and log var == 0 exactly: sse == 0 and ll == -1/2 log 2 pi (the header's constant) bit for
    bit.  (Z, mu, F, noise, scale, want_ll)."""
    d, k = 9, 4
    rng = np.random.RandomState(11)
    mu = rng.randn(1, d)
    F = np.tril(rng.randint(-2, 3, size=(d, d)).astype(np.float64))
    F[k] = 0.
    F[k, 2] = -1.
    Z = np.zeros((1, d + 1))
    Z[0, k], Z[0, d] = 1., mu[0, k]
    return Z, mu, F[None], np.array([0.5]), np.array([0.5]), -0.5 * 1.8378770664093453


# ------------------------------------------------------------------ the host build of csrc/bc_predict_dev.h
def build_harness(outdir, extra=()):
    exe = os.path.join(str(outdir), 'predict_harness')
    cmd = ['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-Wall', '-Werror'] + list(extra) \
        + [os.path.join(ROOT, 'tests', 'predict_harness.cpp'), '-o', exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def run_harness(exe, Z, mu, F, noise, scale, tmp, per_row=True, expect=0):
    """The host build on one problem: dict(ll, sse [T], mean, var [T][Nt] or None); expect: the exit status wanted (2: refused)."""
    Z = np.asarray(Z, dtype=np.float64)
    mu, F = np.atleast_2d(np.asarray(mu, dtype=np.float64)), np.asarray(F, dtype=np.float64)
    nt, d, t = Z.shape[0], Z.shape[1] - 1, mu.shape[0]
    noise = np.broadcast_to(np.asarray(noise, dtype=np.float64), (t,))
    scale = np.broadcast_to(np.asarray(scale, dtype=np.float64), (t,))
    fin, fout = os.path.join(str(tmp), 'predict_in.bin'), os.path.join(str(tmp), 'predict_out.bin')
    np.concatenate([np.array([nt, d, t, 1. if per_row else 0.]), Z.ravel(), mu.ravel(), F.ravel(), noise, scale]).tofile(fin)
    out = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
    assert out.returncode == expect and out.stderr == '', (out.returncode, out.stderr[-2000:])
    if expect:
        return None
    res = np.fromfile(fout)
    assert res.size == 2 * t + (2 * t * nt if per_row else 0)
    mean = res[2 * t:2 * t + t * nt].reshape(t, nt) if per_row else None
    var = res[2 * t + t * nt:].reshape(t, nt) if per_row else None
    return dict(ll=res[:t], sse=res[t:2 * t], mean=mean, var=var)
