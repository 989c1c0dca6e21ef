"""Inputs, reference, bound and shapes for the element-wise tests of K1, the projection (beta_cores_amd/csrc/bc_project_k1.h:
k_project, k_project_r; the host side in csrc/bc_project.hip); no test in here.  tests/test_k1_cases_cpu.py holds the bound
against the float64 oracle (not too tight) and against six wrong projections (not blind); tests/test_gpu_k1_bound.py runs the
lists on the device.

THE REFERENCE.  The nine model formulas (oracle/models_ref.py, likelihoods.*.beta_gradient_host, the comments of bc_model_value),
the centring f - f.mean(axis=1), the row norms and the column sums, restated in np.longdouble (64-bit mantissa, u' = 2^-64).
Contractions are summed in chunks of 64 features and column sums in chunks of 1024 rows, so the reference's own error is at
most (64 + D / 64 + 2) u' of sum |z||theta| and (1024 + n / 1024 + 2) u' of sum |phi|: of the unit u = 2^-53 of the scale the
bound uses for the same quantity, under 1/20 up to D = 2000 and under one up to a million rows.  That unit is part of the "+ 2"
of (D + 2) and (n + 2) below.

THE BOUND is element-wise and built stage by stage.  Every term is taken at its absolute value; u = 2^-53; a float64 operation
rounds its exact result by at most u relative.  The device code is built with -ffp-contract=off, so an expression of
bc_model_value costs exactly the roundings it spells; where a stage is association-free that is said.

  contraction  p = z . theta over D terms, in ANY association (MFMA k-steps of four features, k-chunks of 16 or 32, the resident
      kernel's permuted columns): each product is fused into its addition or rounded once and passes at most D - 1 additions,
          bp = (D + 2) u sum_k |z_k| |theta_k|.
      Gaussian ids: the kernel contracts x with Theta' = Siginv . theta, which plan_stage forms on the host (d products, d - 1
      additions per entry: (d + 1) u |Siginv| |theta|); contracting x with the rounded Theta' adds (d + 2) u |x| . |Theta'|:
          bp = (2 d + 3) u |x|^T |Siginv| |theta|.
      theta^T Siginv theta (plan_stage: an inner d-term sum, then a d-term sum of products) and x^T Siginv x (k_row_quadform: an
      fma chain, then a product and an addition per term) cost the same count:
          b_sa = (2 d + 3) u |theta|^T |Siginv| |theta|,      b_ra = (2 d + 3) u |x|^T |Siginv| |x|.
  model argument, in the nesting bc_model_value spells (y is data: exact)
      q = (y^2 - p (2 y)) + p^2:   bq = 2 |y| bp + 2 |p| bp + u (y^2 + 2 |p y| + |y^2 - 2 p y| + p^2 + |q|)
      q = (ra + sa) - 2 p:         bq = b_ra + b_sa + 2 bp + u (|ra + sa| + |q|)
      m = -p:                      bm = bp
      (the code below carries (value, bound) pairs through _add / _sub / _mul, which add u |result| per operation: the lines
      above are what that gives.)
  model value  f = g(argument):  |g'| (argument's bound) + the body's accuracy + the roundings of the surrounding operations and
      constants.  The constants are restated from model_constants (bc_project.hip) operation by operation through the same
      pairs; a libm call (log, pow, exp, sqrt on the host) counts one ulp = 2 u relative.  The bodies' accuracies are those a
      CPU test asserts for csrc/bc_k1_math.h compiled for the host:
        exp (bc_exp_tab_nonpos)                <= 1.5 ulp = 3 u relative            tests/test_k1_math_cpu.py
        log1p(exp(-a)) (bc_log1p_exp_neg_tab)  <= 3 ulp = 6 u relative              tests/test_k1_math_cpu.py
        bc_logistic_beta_value_pt              <= PT_BODY_ERR[beta] absolute        tests/test_k1_math_cpu.py: twice the measured
                                                  maximum over the harness's grid (the two covers device-versus-gcc evaluation)
        the two beta-gradient bodies           <= 1e-13 (1 + max|g| over the harness's grid), per beta (and sigsq): constants
                                                  included                          tests/test_betagrad_cpu.py
      exp(k2 q) of a far row underflows: its bound carries the absolute floor DBL_MIN, the smallest normal double (2.2e-308),
      which covers a flush to 0 from anywhere below it and the rounding of a subnormal result (the device clamps the argument at
      -800, where the double is 0 already).  The RAW passes (S > 256) evaluate the exp of models 1, 5 and 6 with the restated
      NumPy routine (csrc/bc_np_exp.h: np.exp's bits on AVX-512 hosts, tests/test_np_exp_cpu.py); the float64 oracle of
      tests/test_k1_cases_cpu.py, which calls np.exp itself, lying inside the bound holds that routine to the same 1.5 ulp.
        logistic log-likelihood   m < 100 ? -(max(m, 0) + log1p(exp(-|m|))) : -m;  d/dm log1p(e^m) = sigmoid(m):
                                  bf = sigmoid(m) bm + 6 u log1p(e^-|m|) + u |f|  (+ 3.8e-44 > log1p(e^-100), the step between
                                  the two sides of the branch, where |m - 100| <= bm)
        logistic beta-likelihood  f' = (b + 1) s (A^b s + s^b A),  s = sigmoid(m), A = 1 - s:   bf = |f'| bm + PT_BODY_ERR[b]
        logistic beta-gradient    g' = s (1 - (b+1) a) (e^(-b a) - e^(-(b+1) a)) + (1 - s) (1 - (b+1) c) e^(-(b+1) c),
                                  a = softplus(m), c = softplus(-m):                            bf = |g'| bm + 1e-13 (1 + G)
        linreg beta-gradient      g = (k0 + k1 q) E - k3, E = exp(k2 q):  g' = (k1 + k2 (k0 + k1 q)) E;  bf = |g'| bq + 1e-13 (1 + G)
        the other five            every operation of their case in bc_model_value through the pairs.
  centring  mean = (sum of the S computed values, in any order) / S, phi = f - mean (k1_row_stats; k_center_tiles for S > 256; a
      constant row's NumPy-ordered sum, bc_np_sum_const_*, is one such order): S - 1 additions, one division, one subtraction,
          b_mean = sum_s bf / S + (S - 1) u sum_s |f| / S + u |mean|,        b_phi = bf + b_mean + u |phi|,
      every term relative to the ROW's own sum |f| -- never to the matrix's.  A constant row (all-zero features) has phi = 0 in
      the reference and a residue of a few u |c| on the device (the reference's quirk the kernel reproduces on purpose): inside
      (S - 1) u |c| by construction.
  norm  | ||phi + e|| - ||phi|| | = |sum (2 phi e + e^2)| / (||phi + e|| + ||phi||) with |e| <= b and ||phi + e|| >= ||phi|| - ||b||:
          b_dir = min( ||b||,  (2 sum |phi| b + sum b^2) / (2 ||phi|| - ||b||) )       (the second where 2 ||phi|| > ||b||)
      which is sum |phi| b / ||phi|| to first order; the terms in b^2 and the triangle inequality ||b|| are what is left of it on
      a (nearly) constant row, where the first-order form is 0 / 0.  The sum of S squares and the square root:
          b_norm = b_dir + (S + 2) u (||phi|| + b_dir)  + 1e-300.
  column sum  over n rows in any order (per tile or per wave, then over the partials):
          b_col = sum_n b_phi + (n + 2) u sum_n |phi|  + 1e-300.
  second-order terms (products of two bounds, (1 + u)^k - 1 - k u, exp(delta) - 1 - delta) are covered by ONE final factor 1.01.

No other factor appears: derived, not tuned.  A device result outside it is a finding in K1 or an error in this derivation, and is
resolved by naming which.

INPUTS are seeded by the case.  'plain': standard normal rows; 'wide': the rows scaled over four decades, so that rows with
|f| ~ 1 sit beside rows with |f| ~ 1e4.  The logistic inputs have rows whose margins lie on both sides of the branch at 100.
Every case has two all-zero-feature rows (n // 3 and the last one; one for n = 1).  check_conditions asserts on the reference
what the derivation assumes (see there).

COVERAGE.  model id x K1 instance -> the test that holds the instance against a reference.  "bound": test_staged_case /
test_resident_case of tests/test_gpu_k1_bound.py with the cases of STAGED / RESIDENT below (every element, this bound);
"-": the instance does not exist (launch_project_r_nt: no resident NT = 7 kernel for the models with NumPy's exp, ids 1, 5, 6,
nor for the store-only ids 7, 8).  Column sums of the resident kernel: test_theta_resident_kernel_matches_staged_and_oracle.

  id  model                 staged NT=4  6+4    7      13     16     RAW    | resident NT=4  6+4    7
  0   linreg log-lik        bound        bound  bound  bound  bound  bound  | bound          bound  bound
  1   linreg beta-lik       bound        bound  bound  bound  bound  bound  | bound          bound  -
  2   logistic log-lik      bound        bound  bound  bound  bound  bound  | bound          bound  bound
  3   logistic beta-lik     bound        bound  bound  bound  bound  bound  | bound          bound  bound   (BC_K1_STAGED=-1)
  4   gauss log-lik         bound        bound  bound  bound  bound  bound  | bound          bound  bound
  5   gauss beta-lik        bound        bound  bound  bound  bound  bound  | bound          bound  -
  6   gauss beta-grad       bound        bound  bound  bound  bound  bound  | bound          bound  -
  7   linreg beta-grad      bound        bound  bound  bound  bound  bound  | bound          bound  -
  8   logistic beta-grad    bound        bound  bound  bound  bound  bound  | bound          bound  -
  The store-free forms (bc_project_colsum) produce the column partials of the same instantiation bit for bit
  (tests/test_gpu_storefree.py, test_gpu_f32.py: project_all); ids 7 and 8 have none (bc_k1_no_store_free).  float32 rows: bit
  identity with the widened rows at every staged instance (tests/test_gpu_f32.py), hence this bound.

Worst |error| / bound measured on an MI355X, per model family the largest over its cases (Phi, norms, column sums together):
                staged (STAGED)                                        resident (RESIDENT)
  linreg        0.155  (n = 300, d = 1, S = 112, 'wide': beta-lik)      0.105  (d = 37, S = 16: beta-lik)
  logistic      0.108  (n = 16, d = 31, S = 16, 'wide': beta-lik)       0.138  (d = 37, S = 16: beta-lik)
  gauss         0.094  (n = 127, d = 1, S = 16, 'wide': log-lik)        0.060  (d = 13, S = 16: log-lik)
(MEASURED_RATIOS below.)  The float64 oracle on the host uses the same share: 0.154 at its worst.  A worst-case bound over D + S
roundings that random roundings fill to a tenth is what such a count gives; the wrong projections of the CPU test leave it all the same.
"""
import functools

import numpy as np

from oracle import models_ref as M
from beta_cores_amd import likelihoods as L

U = 2.0 ** -53
LD = np.longdouble
LONGDOUBLE_OK = bool(np.finfo(np.longdouble).eps <= 2.0 ** -63)
LONGDOUBLE_WHY = ('np.longdouble has eps = %g > 2^-63 on this platform: no reference more precise than float64 to hold K1 against'
                  % float(np.finfo(np.longdouble).eps))
DBL_MIN = float(np.finfo(np.float64).tiny)

KINDS = ('plain', 'wide')
FAMILIES = ('linreg', 'logistic', 'gauss')
IDS = {'linreg': (0, 1, 7), 'logistic': (2, 3, 8), 'gauss': (4, 5, 6)}
NAMES = ['linreg log-lik', 'linreg beta-lik', 'logistic log-lik', 'logistic beta-lik', 'gauss log-lik', 'gauss beta-lik',
         'gauss beta-grad', 'linreg beta-grad', 'logistic beta-grad']
SIGSQ = 1.0                                   # on the grid of tests/betagrad_harness.c
BETA = {'linreg': 0.5, 'logistic': 0.5, 'gauss': 0.5}      # 0.5: on the grids of both harnesses

# bc_logistic_beta_value_pt against 80-bit arithmetic over the grid of tests/k1_math_harness.c (gcc -O2 -mfma -ffp-contract=off,
# two million arguments): the measured maximum of the absolute error per beta; asserted, and used in the bound, at twice that
PT_BODY_MEASURED = {0.01: 3.69e-14, 0.1: 3.90e-15, 0.5: 7.70e-16, 1.0: 4.68e-16, 8.0: 1.39e-15, 32.0: 1.35e-12}
PT_BODY_ERR = dict((b, 2. * e) for b, e in PT_BODY_MEASURED.items())
BETAGRAD_BAR = 1e-13                          # tests/test_betagrad_cpu.py: absolute error <= 1e-13 (1 + max|g| over the grid)

# worst |error| / bound measured on an MI355X (gfx950), the largest over the family's cases: (staged, resident)
MEASURED_RATIOS = {'linreg': (0.155, 0.105), 'logistic': (0.108, 0.138), 'gauss': (0.094, 0.060)}


# ------------------------------------------------------------------ (value, bound) pairs
def _t(v, e=0.):
    return (np.asarray(v, dtype=LD), np.asarray(e, dtype=LD))


def _add(a, b):
    v = a[0] + b[0]
    return v, a[1] + b[1] + U * np.abs(v)


def _sub(a, b):
    v = a[0] - b[0]
    return v, a[1] + b[1] + U * np.abs(v)


def _mul(a, b):
    v = a[0] * b[0]
    return v, np.abs(a[0]) * b[1] + np.abs(b[0]) * a[1] + U * np.abs(v)


def _div(a, b):
    v = a[0] / b[0]
    return v, a[1] / np.abs(b[0]) + np.abs(v) * b[1] / np.abs(b[0]) + U * np.abs(v)


def _scale(k, a):
    """k a for a power of two k (or -1): exact"""
    return k * a[0], abs(k) * a[1]


def _libm(v, e):
    """a host libm result: the propagated bound plus one ulp"""
    return v, e + 2 * U * np.abs(v)


def _log(a):
    return _libm(np.log(a[0]), a[1] / np.abs(a[0]))


def _sqrt(a):
    v = np.sqrt(a[0])
    return v, a[1] / (2 * v) + U * v              # correctly rounded


def _pow(a, b):
    v = a[0] ** b[0]
    return _libm(v, v * (np.abs(b[0]) * a[1] / np.abs(a[0]) + np.abs(np.log(a[0])) * b[1]))


def _exp_libm(a):
    v = np.exp(a[0])
    return _libm(v, v * a[1])


def _exp_body(a):
    """bc_exp_tab_nonpos: 1.5 ulp, and the floor for results that leave the normal range"""
    with np.errstate(under='ignore'):
        v = np.exp(a[0])
        return v, v * a[1] + 3 * U * v + DBL_MIN


ONE = _t(1.)
PI = _t(np.pi, 0.)                            # the double the sources spell; the formulas are taken at this value
# (3.141592653589793 differs from pi by 1.2e-16: the reference uses the same double, as oracle/models_ref.py's np.pi does)


# ------------------------------------------------------------------ inputs
def zero_rows(n):
    return sorted(set((n // 3, n - 1)))


def inputs(family, n, d, S, kind):
    """dict(Z [n x dz], th [S x d], Siginv, logdet) seeded by the case.  linreg: rows [x, y] with y = x . t + noise; logistic:
    rows y x with margins of a few units, a tenth of the rows scaled by 60 (margins on both sides of 100, under 700); gauss:
    rows x, a random SPD Siginv.  'wide' scales the rows by 10^[-2 .. 2] (logistic: 10^[-2 .. 0.3], next to the tenth at 60).
    Rows n // 3 and n - 1 have all-zero features."""
    assert family in FAMILIES and kind in KINDS
    rng = np.random.RandomState((1000003 * n + 10007 * d + 101 * S + 7 * FAMILIES.index(family) + KINDS.index(kind)) % (2 ** 31))
    out = dict(Siginv=None, logdet=None)
    if family == 'linreg':
        X = rng.randn(n, d)
        th = rng.randn(S, d) * (0.6 / np.sqrt(d))
        y = X.dot(rng.randn(d) * (0.6 / np.sqrt(d))) + rng.randn(n)
        Z = np.hstack((X, y[:, None]))
        lo, hi = -2., 2.
    elif family == 'logistic':
        Z = rng.randn(n, d)
        th = rng.randn(S, d) * (1.5 / np.sqrt(d))
        lo, hi = -2., 0.3
    else:
        Z = rng.randn(n, d) * 2.
        th = rng.randn(S, d)
        A = rng.randn(d, d) * (0.3 / np.sqrt(d))
        Sig = A.dot(A.T) + np.diag(rng.uniform(0.5, 2., d))
        out['Siginv'] = np.ascontiguousarray(np.linalg.inv(Sig))
        out['logdet'] = float(np.linalg.slogdet(Sig)[1])
        lo, hi = -2., 2.
    sc = 10.0 ** rng.uniform(lo, hi, size=(n, 1)) if kind == 'wide' else np.ones((n, 1))
    if family == 'logistic':
        sc[rng.permutation(n)[:(n + 9) // 10]] = 60.
    Z = Z * sc
    for r in zero_rows(n):
        Z[r, :d] = 0.
    out.update(Z=np.ascontiguousarray(Z), th=np.ascontiguousarray(th))
    return out


def model_and_ids(likelihoods, family, inp):
    """(model, [(model id, params) ...]) of the family, from the package's likelihoods module"""
    b = inp.get('beta', BETA[family])
    if family == 'linreg':
        m = likelihoods.LinearRegression(SIGSQ, beta_gradient=True)
        return m, [(m.model_id, m.params()), (m.beta_model_id, m.params(beta=b)), (m.beta_grad_model_id, m.params(beta=b))]
    if family == 'logistic':
        m = likelihoods.LogisticRegression(beta_gradient=True)
        return m, [(m.model_id, m.params()), (m.beta_model_id, m.params(beta=b)), (m.beta_grad_model_id, m.params(beta=b))]
    m = likelihoods.GaussianLocation(inp['Siginv'], inp['logdet'])
    return m, [(m.model_id, m.params()), (m.beta_model_id, m.params(beta=b)), (m.beta_grad_model_id, m.params(beta=b))]


# ------------------------------------------------------------------ the float64 oracle (what the CPU test holds the bound against)
def oracle_raw(mid, Z, th, inp, beta):
    """un-centred N x S model values in float64: oracle/models_ref.py, likelihoods.*.beta_gradient_host"""
    if mid == 0:
        return M.linreg_loglik(Z, th, SIGSQ)
    if mid == 1:
        return M.linreg_beta_lik(Z, th, beta, SIGSQ)
    if mid == 2:
        return M.logistic_loglik(Z, th)
    if mid == 3:
        return M.logistic_beta_lik(Z, th, beta)
    if mid == 4:
        return M.gauss_loglik(Z, th, inp['Siginv'], inp['logdet'])
    if mid == 5:
        return M.gauss_beta_lik(Z, th, beta, inp['Siginv'], inp['logdet'])
    if mid == 6:
        return M.gauss_beta_grad(Z, th, beta, inp['Siginv'], inp['logdet'])
    if mid == 7:
        return L.LinearRegression(SIGSQ, beta_gradient=True).beta_gradient_host(Z, th, beta)
    assert mid == 8
    return L.LogisticRegression.beta_gradient_host(Z, th, beta)


# ------------------------------------------------------------------ reference and bound
KCH, NCH = 64, 1024


def _ld_dot(A, B):
    """A . B in np.longdouble, the inner axis summed in chunks of KCH (the module docstring counts the reference's own error)"""
    A = np.asarray(A, dtype=LD)
    B = np.asarray(B, dtype=LD)
    out = np.zeros((A.shape[0], B.shape[1]), dtype=LD)
    for k in range(0, A.shape[1], KCH):
        out += A[:, k:k + KCH].dot(B[k:k + KCH])
    return out


def _ld_colsum(A):
    out = np.zeros(A.shape[1], dtype=LD)
    for i in range(0, A.shape[0], NCH):
        out += A[i:i + NCH].sum(axis=0)
    return out


def contraction(family, Z, th, Siginv):
    """(p, ra, sa) as pairs: the contraction values N x S, the per-row extra N x 1, the per-sample extra 1 x S"""
    assert LONGDOUBLE_OK, LONGDOUBLE_WHY
    Zl, tl = np.asarray(Z, dtype=LD), np.asarray(th, dtype=LD)
    d = tl.shape[1]
    zero = _t(np.zeros((1, 1)))
    if family != 'gauss':
        X = Zl[:, :d]
        p = (_ld_dot(X, tl.T), (d + 2) * U * _ld_dot(np.abs(X), np.abs(tl).T))
        ra = _t(Zl[:, d:d + 1]) if family == 'linreg' else zero
        return p, ra, zero
    Sl = np.asarray(Siginv, dtype=LD)
    k = (2 * d + 3) * U
    St, aSt = _ld_dot(Sl, tl.T), _ld_dot(np.abs(Sl), np.abs(tl).T)          # d x S
    p = (_ld_dot(Zl, St), k * _ld_dot(np.abs(Zl), aSt))
    ra = ((Zl * _ld_dot(Zl, Sl)).sum(axis=1)[:, None], k * (np.abs(Zl) * _ld_dot(np.abs(Zl), np.abs(Sl))).sum(axis=1)[:, None])
    sa = ((tl.T * St).sum(axis=0)[None, :], k * (np.abs(tl).T * aSt).sum(axis=0)[None, :])
    return p, ra, sa


def _softplus_pair(m):
    """(a, c, s, ls): softplus(m), softplus(-m), sigmoid(m), log1p(e^-|m|) in long double"""
    with np.errstate(under='ignore'):
        em = np.exp(-np.abs(m))
        ls = np.log1p(em)
        a, c = np.maximum(m, 0) + ls, np.maximum(-m, 0) + ls
        s = np.where(m > 0, 1 / (1 + em), em / (1 + em))
    return a, c, s, ls


def harness_grid(hi, two_sided, marks):
    """fill_grid of tests/betagrad_harness.c: the grid its bar's max|g| is taken over"""
    g = [(-hi if two_sided else 0.) + (2. if two_sided else 1.) * hi * i / 3000. for i in range(3001)]
    v = hi
    while v > 1e-12:
        g += [v, -v] if two_sided else [v]
        v *= 0.93
    for mk in marks:
        for i in range(-40, 41):
            v = mk * (1. + i * 2.5e-4) + i * 1e-9
            if 0. <= v <= hi:
                g += [v, -v] if two_sided else [v]
    return np.array(g + [0.], dtype=LD)


def _logistic_beta_grad(m, beta):
    a, c, s, _ = _softplus_pair(m)
    with np.errstate(under='ignore'):
        ea, ea1, ec1 = np.exp(-beta * a), np.exp(-(beta + 1) * a), np.exp(-(beta + 1) * c)
        g = ea / beta ** 2 + (beta + 1) / beta * a * ea - a * ea1 - c * ec1
        dg = s * (1 - (beta + 1) * a) * (ea - ea1) + (1 - s) * (1 - (beta + 1) * c) * ec1
    return g, dg


def _linreg_beta_grad_consts(beta, sigsq):
    beta, sigsq = LD(beta), LD(sigsq)
    Lg = np.log(2 * LD(np.pi) * sigsq)
    Cn = np.exp(-beta * Lg / 2)
    r = (beta + 1) / beta
    return (Cn * (Lg / 2 * r + 1 / beta ** 2), Cn * r / (2 * sigsq), -beta / (2 * sigsq),
            Cn * (Lg / 2 / np.sqrt(1 + beta) + (1 + beta) ** LD(-1.5) / 2))


def _linreg_beta_grad(q, beta, sigsq):
    k0, k1, k2, k3 = _linreg_beta_grad_consts(beta, sigsq)
    with np.errstate(under='ignore'):
        E = np.exp(k2 * q)
    return (k0 + k1 * q) * E - k3, (k1 + k2 * (k0 + k1 * q)) * E


@functools.lru_cache(maxsize=None)
def betagrad_scale(mid, beta, sigsq=SIGSQ):
    """1 + max|g| over the harness's grid: the unit of the beta-gradient bodies' bar"""
    if mid == 8:
        marks = [800., 709.782712893384, 745., 1499. if 800. / beta > 1500. else 800. / beta, 800. / (beta + 1.), 36.7]
        return 1 + np.abs(_logistic_beta_grad(harness_grid(1500., True, marks), LD(beta))[0]).max()
    k2 = float(_linreg_beta_grad_consts(beta, sigsq)[2])
    return 1 + np.abs(_linreg_beta_grad(harness_grid(1e4, False, [800. / -k2, 1. / -k2, 36.7 / -k2]), beta, sigsq)[0]).max()


def model_value(mid, p, ra, sa, d, beta=None, logdet=None, sigsq=SIGSQ):
    """(f, bf): the un-centred model values N x S in long double and their element-wise bound (no factor 1.01 yet).  The
    constants follow model_constants (csrc/bc_project.hip), the expressions bc_model_value (csrc/bc_project_k1.h)."""
    two_pi = _scale(2., PI)
    b = None if beta is None else _t(beta)
    if mid in (0, 1, 7):
        y = ra
        q = _add(_sub(_mul(y, y), _mul(p, _scale(2., y))), _mul(p, p))
        tps = _mul(two_pi, _t(sigsq))
        if mid == 0:                              # c0 - c1 q;  c0 = -1/2 log(2 pi sigsq), c1 = 1 / (2 sigsq)
            c0 = _scale(-.5, _log(tps))
            c1 = _div(ONE, _scale(2., _t(sigsq)))
            return _sub(c0, _mul(c1, q))
        if mid == 1:                              # k0 (k1 exp(k2 q) + k3)
            k0 = _div(ONE, _pow(tps, _scale(.5, b)))
            k1 = _scale(-1., _div(_add(b, ONE), b))
            k2 = _scale(-1., _div(b, _scale(2., _t(sigsq))))
            k3 = _div(ONE, _sqrt(_add(ONE, b)))
            return _mul(k0, _add(_mul(k1, _exp_body(_mul(k2, q))), k3))
        g, dg = _linreg_beta_grad(q[0], beta, sigsq)
        return g, np.abs(dg) * q[1] + BETAGRAD_BAR * betagrad_scale(7, beta, sigsq)
    if mid in (2, 3, 8):
        m, bm = -p[0], p[1]
        a, c, s, ls = _softplus_pair(m)
        if mid == 2:
            f = np.where(m < 100, -a, -m)
            return f, s * bm + 6 * U * ls + U * np.abs(f) + np.where(np.abs(m - 100) <= bm, LD(3.8e-44), LD(0.))
        if mid == 3:
            with np.errstate(under='ignore'):
                Ab, sb = np.exp(-beta * a), np.exp(-beta * c)      # (1 + e^m)^-beta, (1 + e^-m)^-beta
                A1, s1 = Ab * np.exp(-a), sb * np.exp(-c)
                f = -((LD(beta) + 1) / LD(beta) * Ab - (A1 + s1))
                df = (LD(beta) + 1) * s * (Ab * s + sb * np.exp(-a))
            return f, np.abs(df) * bm + PT_BODY_ERR[beta]
        g, dg = _logistic_beta_grad(m, LD(beta))
        return g, np.abs(dg) * bm + BETAGRAD_BAR * betagrad_scale(8, beta)
    q = _sub(_add(ra, sa), _scale(2., p))
    dd = _t(float(d))
    if mid == 4:                                  # c0 - 1/2 q;  c0 = -d/2 log(2 pi) - 1/2 logdet
        c0 = _sub(_mul(_scale(-.5, dd), _log(two_pi)), _scale(.5, _t(logdet)))
        return _sub(c0, _scale(.5, q))
    c0 = _div(ONE, b)
    c1 = _scale(-.5, b)
    ex = _sub(_mul(_t(-.5), dd), ONE)             # -.5 d - 1: exact in float64 (its pair's u terms are an over-count)
    c2 = _pow(_add(ONE, b), ex)
    gq = _exp_body(_mul(c1, q))
    if mid == 5:                                  # c0 exp(c1 q) - c2
        return _sub(_mul(c0, gq), c2)
    assert mid == 6                               # ((t1 - t2) - t3) - c6
    c3 = _log(_mul(_pow(two_pi, _mul(_t(-.5), dd)), _pow(_exp_libm(_t(logdet)), _t(-.5))))
    c4 = _div(ONE, _pow(b, _t(2.)))
    c5 = _div(ONE, _scale(2., b))
    c6 = _mul(c2, _log(_add(ONE, b)))
    t1 = _mul(c3, _sub(_mul(c0, gq), c2))
    t2 = _mul(c4, gq)
    t3 = _mul(_mul(c5, q), gq)
    return _sub(_sub(_sub(t1, t2), t3), c6)


def centre(f, bf):
    """(phi, b_phi, norms, b_norms, colsum, b_colsum) in long double, the bounds with their final factor 1.01"""
    n, S = f.shape
    f = np.broadcast_to(f, (n, S))
    bf = np.broadcast_to(bf, (n, S))
    mean = f.sum(axis=1) / S
    phi = f - mean[:, None]
    b_mean = bf.sum(axis=1) / S + (S - 1) * U * np.abs(f).sum(axis=1) / S + U * np.abs(mean)
    b = bf + b_mean[:, None] + U * np.abs(phi)
    nrm = np.sqrt((phi * phi).sum(axis=1))
    nb = np.sqrt((b * b).sum(axis=1))
    den = 2 * nrm - nb
    with np.errstate(divide='ignore', invalid='ignore'):
        first = np.where(den > 0, (2 * (np.abs(phi) * b).sum(axis=1) + nb * nb) / np.where(den > 0, den, 1), np.inf)
    b_dir = np.minimum(nb, first)
    b_norm = b_dir + (S + 2) * U * (nrm + b_dir) + LD(1e-300)
    cs = _ld_colsum(phi)
    b_cs = _ld_colsum(b) + (n + 2) * U * _ld_colsum(np.abs(phi)) + LD(1e-300)
    return phi, 1.01 * b, nrm, 1.01 * b_norm, cs, 1.01 * b_cs


def reference(family, mid, inp, rows=None):
    """dict(f, phi, b, norms, b_norms, colsum, b_colsum) of model `mid` on the case's inputs (`rows`: these rows only -- the column
    sums are then those of the picked rows and mean nothing)"""
    Z = inp['Z'] if rows is None else inp['Z'][rows]
    p, ra, sa = contraction(family, Z, inp['th'], inp['Siginv'])
    beta = None if mid in (0, 2, 4) else inp.get('beta', BETA[family])
    f, bf = model_value(mid, p, ra, sa, inp['th'].shape[1], beta=beta, logdet=inp['logdet'])
    phi, b, nrm, bn, cs, bcs = centre(f, bf)
    return dict(unbounded=mid in (0, 2, 4), f=np.broadcast_to(f, phi.shape), m=-p[0], phi=phi, b=b, norms=nrm, b_norms=bn, colsum=cs, b_colsum=bcs)


@functools.lru_cache(maxsize=8)
def case(family, n, d, S, kind):
    """(inputs, {model id: reference}) of a listed case: shared by the checks of one test, read-only"""
    inp = inputs(family, n, d, S, kind)
    refs = dict((mid, reference(family, mid, inp)) for mid in IDS[family])
    for ref in refs.values():
        check_conditions(family, ref, kind)
    return inp, refs


def check_conditions(family, ref, kind):
    """What the derivation assumes, asserted on the reference: NaN-free and finite; the logistic margins stay under 700 (off
    the reference's jump at np.exp's overflow) and reach both sides of the branch at 100 in a case of ten rows or more with two
    samples or more; no non-zero centred value whose square underflows; in a 'wide' case of ten rows or more at least a tenth
    of the rows have max|f| under 1e-2 of the matrix's (asserted where f is unbounded: the three log-likelihoods)."""
    f, phi = ref['f'], ref['phi']
    assert np.isfinite(f).all() and np.isfinite(phi).all() and np.isfinite(ref['b']).all()
    n, S = f.shape
    if family == 'logistic':
        m = np.abs(ref['m'])
        assert m.max() < 700.
        if n >= 10 and S >= 2:
            assert (m > 100.).any() and ((m < 100.) & (m > 50.)).any()
    nz = np.abs(phi[phi != 0])
    assert nz.size == 0 or nz.min() > 1e-150
    assert max(BETA.values()) <= 32.
    if kind == 'wide' and n >= 10 and ref['unbounded']:
        rmax = np.abs(f).max(axis=1)
        assert (rmax < 1e-2 * rmax.max()).sum() * 10 >= n, ((rmax < 1e-2 * rmax.max()).sum(), n)


def ratios(ref, phi_dev, norms_dev=None, colsum_dev=None):
    """worst |error| / bound of (Phi, norms, column sums); inf where a device value is not finite"""
    out = []
    for got, want, bound in ((phi_dev, ref['phi'], ref['b']), (norms_dev, ref['norms'], ref['b_norms']), (colsum_dev, ref['colsum'], ref['b_colsum'])):
        if got is None:
            out.append(0.)
            continue
        got = np.asarray(got)
        assert got.shape == want.shape, (got.shape, want.shape)
        if not np.isfinite(got).all():
            out.append(float('inf'))
            continue
        out.append(float((np.abs(got.astype(LD) - want) / bound).max()) if got.size else 0.)
    return tuple(out)


# ------------------------------------------------------------------ which instance a shape runs on (theta_layout, restated)
def instance(S):
    """(name, NT, padded sample count, KC) of the staged instance bc_project picks for S samples (theta_layout, bc_project.hip)"""
    if S > 256:
        return 'RAW', 16, 16 * ((S + 15) // 16), 16
    nt = (S + 15) // 16
    if 96 < S <= 100:
        return '6+4', 6, 100, 32
    NT = 4 if nt <= 4 else 7 if nt <= 7 else 13 if nt <= 13 else 16
    return str(NT), NT, 16 * NT, 32 if NT <= 7 else 16


# ------------------------------------------------------------------ the lists: (family, n, d, S, kind)
# S, one per instance and its edges: 1, 16, 64 | 97, 100 | 65, 101, 112 | 113, 208 | 209, 256 | 257, 300, 513
# D against the k-chunk: 1, 31, 32, 33 (KC = 32: NT <= 7); 15, 16, 17 (KC = 16: NT >= 13, RAW); 130 > 128
# n: 1, 15, 16, 17, 127, 128, 129, 300.  Every family (hence every model id) meets every instance and a ragged n at S = 97 .. 100.
STAGED = [
    ('linreg', 1, 1, 1, 'plain'), ('linreg', 129, 33, 64, 'wide'), ('linreg', 127, 31, 97, 'wide'), ('linreg', 17, 32, 100, 'plain'),
    ('linreg', 128, 33, 65, 'plain'), ('linreg', 300, 1, 112, 'wide'), ('linreg', 15, 15, 113, 'plain'), ('linreg', 129, 17, 208, 'wide'),
    ('linreg', 16, 16, 209, 'wide'), ('linreg', 127, 130, 256, 'plain'), ('linreg', 129, 17, 257, 'plain'), ('linreg', 300, 15, 513, 'wide'),
    ('logistic', 16, 31, 16, 'wide'), ('logistic', 1, 32, 64, 'plain'), ('logistic', 129, 33, 100, 'wide'), ('logistic', 15, 1, 97, 'plain'),
    ('logistic', 127, 32, 101, 'wide'), ('logistic', 17, 130, 112, 'plain'), ('logistic', 128, 16, 113, 'wide'), ('logistic', 300, 17, 208, 'plain'),
    ('logistic', 129, 15, 256, 'plain'), ('logistic', 17, 16, 209, 'wide'), ('logistic', 300, 16, 300, 'wide'), ('logistic', 127, 17, 257, 'plain'),
    ('gauss', 300, 33, 1, 'plain'), ('gauss', 127, 1, 16, 'wide'), ('gauss', 15, 32, 64, 'plain'), ('gauss', 129, 31, 97, 'wide'),
    ('gauss', 16, 33, 100, 'plain'), ('gauss', 17, 32, 65, 'wide'), ('gauss', 128, 31, 101, 'plain'), ('gauss', 129, 1, 112, 'wide'),
    ('gauss', 127, 16, 113, 'plain'), ('gauss', 1, 17, 208, 'plain'), ('gauss', 300, 15, 209, 'wide'), ('gauss', 129, 130, 256, 'wide'),
    ('gauss', 128, 16, 257, 'wide'), ('gauss', 17, 17, 300, 'plain'), ('gauss', 129, 15, 513, 'plain'),
]

# the resident kernel: n = 128 * 8 * n_cu + 77 rows (the smallest count project_r_grid accepts, plus a ragged group); (d, S)
RESIDENT = [(13, 16), (37, 16), (13, 100), (37, 100), (13, 112), (37, 112)]
RESIDENT_BETA = 0.1                            # another point of both harnesses' grids than the staged cases'
RESIDENT_NO_NT7 = (1, 5, 6, 7, 8)              # ids without a resident instance at S in 101 .. 112 (launch_project_r_nt)


def resident_rows(n_cu):
    return 128 * 8 * n_cu + 77


def resident_pick(n, rng):
    """>= 300 rows to reference: the group and tile edges, the ragged last group, the zero-feature rows, and random ones"""
    fixed = [0, 1, 31, 32, 127, 128, n - 33, n - 32, n - 1] + zero_rows(n)
    return np.unique(np.concatenate((fixed, rng.choice(n, 300, replace=False))))


def resident_inputs(family, n, d, S):
    """inputs() of kind 'wide' at the resident row count, with beta = RESIDENT_BETA"""
    inp = inputs(family, n, d, S, 'wide')
    inp['beta'] = RESIDENT_BETA
    return inp
