"""Shared by tests/test_psvi_many_gauss_cpu.py, tests/test_psvi_many_gauss_sanitized_cpu.py and tests/test_gpu_psvi_many_gauss.py
(no test collects from this file): the Gaussian-location kind of the batched BatchPSVI run (include/beta_cores_psvi_many.h).  A
case generator, a runner for tests/psvi_many_gauss_harness.cpp, a long-double restatement of the row aux, target, residual and g_w
of one step with the bounds both builds are held to, and a long-double restatement of a whole run of k steps.  The posterior mean
and the draw are held to tests/vi_sampler_cases.py (reference_ld, draw_bound), the point-gradient to tests/psvi_cases.py, the ADAM
stage to tests/psvi_many_cases.adam_step; nothing of theirs is changed.

The bounds, to first order with u = 2^-53.  Sg = Siginv (d x d), x a row, th a sample, and
    RA[n] = sum_ab |x_a Sg_ab x_b|,   SA[q] = sum_ab |th_a Sg_ab th_b|,   PA[n, q] = sum_ab |x_a Sg_ab th_b|,
    A[n, q] = |c0| + (RA[n] + SA[q]) / 2 + PA[n, q]                    (every term of ll with its absolute value: |ll| <= A)
  ra[n]         t_a = the d-term fma chain over b (gamma_d), one product x_a t_a, d - 1 additions:     <= (2 d + 1) u RA[n]
  sa[q]         the inner sum rounds every product and every addition (d + 1), one product, d additions: <= (2 d + 2) u SA[q]
                (the chain form; the matrix-core form's inner sum is gamma_d and its outer sum has ceil(d / 16) + 4 additions: less)
  Theta'[q, c]  a d-term sum of rounded products: (d + 1) u sum_b |Sg_cb th_b| (the matrix-core form: gamma_d); the contraction p = x . Theta'_q on the matrix
                cores adds gamma_d of its own terms:                                                      <= (2 d + 1) u PA[n, q]
  ll[n, q]      = c0 - ((ra + sa) - 2 p) / 2: two roundings in the bracket, <= u (RA + SA) + u (RA + SA + 2 PA), halved exactly,
                one rounding of the result, u A; with the three above:
                <= (2 d + 2) u (RA + SA) / 2 + (2 d + 1) u PA + u (RA + SA) + u PA + u A  <=  (2 d + 5) u A[n, q]
  c[n, q]       = ll - mean_q ll: the S-term mean adds gamma_S mean |ll| and one division, the subtraction one rounding:
                <= (S + 2 d + 7) u Ac[n, q],   Ac[n, q] = A[n, q] + mean_q A[n, .]   (and |c| <= Ac)
  target[q]     = scale sum_n c[n, q], n_sub terms in a fixed order, one product:
                <= (n_sub + S + 2 d + 8) u scale sum_n Ac[n, q]                                            =: bt[q]
  resid[q]      = target - sum_i w_i cv[i, q], an m-term fma chain and one subtraction, cv the c of the points:
                <= bt[q] + (S + 2 d + m + 9) u sum_i |w_i| Ac_p[i, q] + u scale sum_n Ac[n, q]            =: br[q]
  g_w[i]        = -(sum_q cv[i, q] resid[q]) / S:
                <= (1 / S) sum_q ((2 S + 2 d + 9) u Ac_p[i, q] |resid_q| + Ac_p[i, q] br[q])
These are tests/psvi_many_cases.py's forms with the logistic element's (D + 4) u A replaced by this model's (2 d + 5) u A: the
gamma_k sum |terms| form, k the summation lengths added up, and K_SECOND = 2 for the second-order terms; no constant is fitted.
The x-only and theta-only terms that the centring removes mathematically are part of A, as the device keeps them (K1's
expression).  The reference is the same expression evaluated in np.longdouble (the three quadratic forms from Sg itself, no
Theta'): its own error is three decimal orders below."""
import os
import subprocess

import numpy as np

import psvi_cases as pc
import psvi_many_cases as pm
import vi_sampler_cases as vc

ROOT = pm.ROOT
ld = np.longdouble
U, K_SECOND = pm.U, pm.K_SECOND
B1, B2, EPS = pm.B1, pm.B2, pm.EPS
N_TOTAL = 600.


def build_harness(outdir, extra=()):
    exe = os.path.join(str(outdir), 'psvi_many_gauss_harness')
    cmd = ['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-Wall', '-Werror', '-Wno-unknown-pragmas'] + list(extra) \
        + [os.path.join(ROOT, 'tests', 'psvi_many_gauss_harness.cpp'), '-o', exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def _spd(rng, d, lo, hi):
    """a dense symmetric positive definite d x d matrix with eigenvalues log-spaced over [lo, hi] (condition number hi / lo)"""
    q = np.linalg.qr(rng.randn(d, d))[0]
    a = (q * np.logspace(np.log10(lo), np.log10(hi), d)).dot(q.T)
    return (a + a.T) / 2.


def make_model(d, seed=0):
    """Siginv and Sig0inv dense (an isotropic matrix would hide a transposed index), condition number <= 10, mu0 non-zero."""
    rng = np.random.RandomState(52000 + 10 * d + seed)
    Siginv, Sig0inv = _spd(rng, d, 0.02, 0.2), _spd(rng, d, 0.3, 3.)
    assert np.linalg.cond(Siginv) <= 10. * (1. + 1e-9) and np.linalg.cond(Sig0inv) <= 10. * (1. + 1e-9)
    mu0 = 0.5 * rng.randn(d) + 0.25
    return {'d': d, 'Siginv': Siginv, 'Sig0inv': Sig0inv, 'mu0': mu0, 'logdet': float(-np.linalg.slogdet(Siginv)[1])}


def model_constant(mdl):
    """c0 as csrc/bc_project.hip (bc_proj_model_constants) writes it"""
    return -float(mdl['d']) / 2 * np.log(2 * 3.141592653589793) - 1. / 2. * mdl['logdet']


def make_rows(rng, n, d):
    """rows of the model's scale around a non-zero centre, values a float32 holds"""
    return (3. * rng.randn(n, d) + 1.).astype(np.float32).astype(np.float64)


def make_step(d, m, s, n_sub, seed=0, step_i=2):
    """One step's inputs: m points with weights N / m (a few perturbed), n_sub data rows, normals, moments as a few earlier steps
    would leave them, the step arrays at iteration step_i."""
    mdl = make_model(d, seed)
    rng = np.random.RandomState(91000 + 1000 * d + 10 * m + s + n_sub + seed)
    w = np.full(m, N_TOTAL / m) * (1. + 0.1 * rng.rand(m))
    st = dict(mdl, m=m, s=s, n_sub=n_sub, scale=N_TOTAL / n_sub, pts=make_rows(rng, m, d), w=w, E=rng.randn(s, d), rows=make_rows(rng, n_sub, d),
              step_i=step_i, step=1. / (1. + step_i), c1=1. - B1 ** (step_i + 1), c2=1. - B2 ** (step_i + 1),
              m1w=rng.randn(m) * 0.1, m1p=rng.randn(m, d) * 0.1, m2w=rng.rand(m) * 0.01, m2p=rng.rand(m, d) * 0.01)
    return st


def run_step(exe, st, tmp):
    d, m, s, n_sub = st['d'], st['m'], st['s'], st['n_sub']
    parts = [np.array([d, m, s, n_sub, st['scale'], st['step'], st['c1'], st['c2'], st['logdet'], 1. if st.get('chains') else 0.]), st['pts'], st['w'], st['mu0'], st['Sig0inv'],
             st['Siginv'], st['E'], st['rows'], st['m1w'], st['m1p'], st['m2w'], st['m2p']]
    fin, fout = os.path.join(str(tmp), 'pmg_in.bin'), os.path.join(str(tmp), 'pmg_out.bin')
    np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in parts]).tofile(fin)
    out = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stderr == '', (out.returncode, out.stderr[-2000:])
    res = np.fromfile(fout)
    shapes = [('mode', (d,)), ('theta', (s, d)), ('thp', (s, d)), ('sa', (s,)), ('ra_sub', (n_sub,)), ('ra_pts', (m,)), ('target', (s,)),
              ('resid', (s,)), ('gw', (m,)), ('gp', (m, d)), ('w', (m,)), ('pts', (m, d)), ('m1w', (m,)), ('m1p', (m, d)), ('m2w', (m,)), ('m2p', (m, d))]
    r, at = {'status': int(res[0])}, 1
    for k, shp in shapes:
        n = int(np.prod(shp))
        r[k] = res[at:at + n].reshape(shp)
        at += n
    assert at == res.size
    return r


# ---------------------------------------------------------------- the quadratic forms and the centred log-likelihoods in long double
def quadform_ld(X, Siginv):
    """(x^T Sg x, the same with every term's absolute value) per row, long double"""
    Xl, Sl = np.asarray(X, dtype=ld), np.asarray(Siginv, dtype=ld)
    return (Xl * Xl.dot(Sl)).sum(axis=1), (np.abs(Xl) * np.abs(Xl).dot(np.abs(Sl))).sum(axis=1)


def quadform_bounds(X, Siginv, chain):
    """(reference, bound) of the device's quadratic forms: chain = 2 d + 1 (ra) or 2 d + 2 (sa) of the module docstring"""
    ref, absum = quadform_ld(X, Siginv)
    return ref, K_SECOND * chain * U * absum


def _centred_ld(X, theta, Siginv, c0):
    """(c, Ac) of the module docstring for rows X under the draws theta, both in long double"""
    Xl, Tl, Sl = np.asarray(X, dtype=ld), np.asarray(theta, dtype=ld), np.asarray(Siginv, dtype=ld)
    ra, RA = quadform_ld(Xl, Sl)
    sa, SA = quadform_ld(Tl, Sl)
    ll = ld(c0) - ((ra[:, None] + sa[None, :]) - 2 * Xl.dot(Sl).dot(Tl.T)) / 2
    PA = np.abs(Xl).dot(np.abs(Sl)).dot(np.abs(Tl).T)
    A = np.abs(ld(c0)) + (RA[:, None] + SA[None, :]) / 2 + PA
    return ll - ll.mean(axis=1)[:, None], A + A.mean(axis=1)[:, None]


def reference_stage34(rows, scale, pts, w, theta, mdl):
    """dict of target, resid, gw (long double) and their bounds bt, br, bg for the GIVEN draws theta (the device's own)"""
    n_sub, d = rows.shape
    m, s = pts.shape[0], theta.shape[0]
    c0 = model_constant(mdl)
    c, Ac = _centred_ld(rows, theta, mdl['Siginv'], c0)
    cv, Acp = _centred_ld(pts, theta, mdl['Siginv'], c0)
    wl, sc = np.asarray(w, dtype=ld), ld(scale)
    tabs = sc * Ac.sum(axis=0)
    target = sc * c.sum(axis=0)
    resid = target - wl.dot(cv)
    gw = -cv.dot(resid) / s
    bt = (n_sub + s + 2 * d + 8) * U * tabs
    br = bt + (s + 2 * d + m + 9) * U * np.abs(wl).dot(Acp) + U * tabs
    bg = ((2 * s + 2 * d + 9) * U * Acp.dot(np.abs(resid)) + Acp.dot(br)) / s
    return dict(target=target, resid=resid, gw=gw, cv=cv, bt=K_SECOND * bt, br=K_SECOND * br, bg=K_SECOND * bg)


def _held(label, name, got, ref, bound):
    err = np.abs(np.asarray(got, dtype=ld) - ref)
    ratio = float((err / np.maximum(bound, np.finfo(np.float64).tiny)).max())
    print('%s %s: worst error %.3e, worst error / bound %.3e' % (label, name, float(err.max()), ratio))
    assert np.all(err <= bound), (label, name, ratio)
    return ratio


def check_stage34(label, rows, scale, pts, w, theta, mdl, target, resid, gw):
    """Asserts the three against reference_stage34; returns the worst error / bound ratios (target, resid, g_w)."""
    assert pc.LD_OK
    ref = reference_stage34(rows, scale, pts, w, theta, mdl)
    return [_held(label, name, got, ref[name], bound) for name, got, bound in
            (('target', target, ref['bt']), ('resid', resid, ref['br']), ('gw', gw, ref['bg']))]


def check_quadforms(label, mdl, rows=None, ra_rows=None, theta=None, sa=None):
    """the device's own d^2-term quadratic forms (the host harness hands them out; the GPU seam does not)"""
    d = mdl['d']
    if ra_rows is not None:
        _held(label, 'ra', ra_rows, *quadform_bounds(rows, mdl['Siginv'], 2 * d + 1))
    if sa is not None:
        _held(label, 'sa', sa, *quadform_bounds(theta, mdl['Siginv'], 2 * d + 2))


def sampler_case(pts, w, E, mdl):
    """the case dict of tests/vi_sampler_cases.py (GAUSS kind) for these points and weights"""
    return {'kind': vc.GAUSS, 'd': mdl['d'], 'm': pts.shape[0], 's': E.shape[0], 'w': w, 'rows': pts, 'Sig0inv': mdl['Sig0inv'], 'th0': mdl['mu0'],
            'Siginv': mdl['Siginv'], 'E': E}


def check_mean_and_draw(label, pts, w, E, mdl, mode, theta):
    """posterior mean and draw under vi_sampler_cases.reference_ld and draw_bound"""
    assert vc.LD_OK
    ref = vc.reference_ld(sampler_case(pts, w, E, mdl))
    d, kappa = mdl['d'], ref['kappa']
    err_m, bound_m = np.abs(mode - ref['mu']).max(), vc.draw_bound(d, kappa, ref['mu'])
    err_d, bound_d = np.abs(theta - ref['theta']).max(), vc.draw_bound(d, kappa, ref['theta'])
    print('%s: mean error %.3e (bound %.3e), draw error %.3e (bound %.3e), kappa %.3e' % (label, err_m, bound_m, err_d, bound_d, kappa))
    assert err_m <= bound_m, (label, err_m, bound_m)
    assert err_d <= bound_d, (label, err_d, bound_d)
    return err_m / bound_m, err_d / bound_d


def check_point_grad(label, pts, w, theta, resid, mdl, gp):
    """g_p under tests/psvi_cases.py's reference and bound (kind GAUSS) on the GIVEN resid (the device's own)."""
    c = {'kind': pc.GAUSS, 'm': pts.shape[0], 's': theta.shape[0], 'd': pts.shape[1], 'sigsq': 1., 'pts': pts, 'theta': theta, 'w': w, 'resid': resid,
         'Siginv': mdl['Siginv']}
    ref, bound = pc.reference(c)
    return _held(label, 'g_p', gp, ref, bound)


def check_adam(label, x0, g, m1, m2, step, i, m, got_x, got_m1, got_m2):
    """the state after ADAM: util/opt.py's statements (psvi_many_cases.adam_step) on the given gradient, to <= 1 ulp"""
    x, m1, m2 = pm.adam_step(x0, g, m1, m2, step, i, np.arange(m))
    for name, got, want in (('x', got_x, x), ('mom1', got_m1, m1), ('mom2', got_m2, m2)):
        worst = float(pm.ulps(got, want).max())
        print('%s ADAM %s: %.2f ulp' % (label, name, worst))
        assert worst <= 1., (label, name, worst)


# ---------------------------------------------------------------- a whole run in long double
def _posterior_ld(pts, w, mdl):
    """(mu, L) in long double: vi_sampler_cases.reference_ld's statements (A's lower triangle, explicit Cholesky, L = C^-1,
    mu = L L^T rhs), not rounded to double in between"""
    d = mdl['d']
    S0, Si, mu0 = [np.asarray(mdl[k], dtype=ld) for k in ('Sig0inv', 'Siginv', 'mu0')]
    A = S0 + w.sum() * Si
    rhs = S0.dot(mu0) + Si.dot((pts * w[:, None]).sum(axis=0))
    Cf = np.zeros((d, d), dtype=ld)
    for k in range(d):
        col = A[k:, k] - Cf[k:, :k].dot(Cf[k, :k])
        assert col[0] > 0. and np.isfinite(col[0])
        piv = np.sqrt(col[0])
        Cf[k:, k] = col / piv
        Cf[k, k] = piv
    L = np.zeros((d, d), dtype=ld)
    for i in range(d):
        e = np.zeros(d, dtype=ld)
        e[i] = 1.
        L[i] = (e - Cf[i, :i].dot(L[:i])) / Cf[i, i]
    return L.dot(L.T).dot(rhs), L


def whole_run_ld(data, pts0, w0, mdl, E, idx, steps, n_total):
    """k = len(E) steps of ONE problem in long double: posterior, draw, target, residual, both gradients (bpsvi.py:47-57 on
    gaussian.py's formulas), ADAM with the projection of the weights.  data: all rows; idx: k x n_sub row numbers; steps: k step
    sizes.  Returns (w, pts) as float64 and the smallest weight met after any step (the margin from the projection's kink)."""
    Si, c0 = np.asarray(mdl['Siginv'], dtype=ld), model_constant(mdl)
    w, pts = np.asarray(w0, dtype=ld).copy(), np.asarray(pts0, dtype=ld).copy()
    m, d = pts.shape
    S, n_sub = E.shape[1], idx.shape[1]
    x = np.concatenate((w, pts.ravel()))
    m1, m2 = np.zeros_like(x), np.zeros_like(x)
    closest = np.inf
    for i in range(E.shape[0]):
        w, pts = x[:m], x[m:].reshape(m, d)
        mu, L = _posterior_ld(pts, w, mdl)
        th = mu + np.asarray(E[i], dtype=ld).dot(L.T)

        def centred(X):
            diff = X[:, None, :] - th[None, :, :]
            ll = ld(c0) - (diff * diff.dot(Si)).sum(axis=2) / 2
            return ll - ll.mean(axis=1)[:, None]
        target = ld(n_total) / n_sub * centred(np.asarray(data[idx[i]], dtype=ld)).sum(axis=0)
        cv = centred(pts)
        resid = target - w.dot(cv)
        gw = -cv.dot(resid) / S
        G = th.dot(Si)[None, :, :] - pts.dot(Si)[:, None, :]
        G = G - G.mean(axis=2)[:, :, None]
        gp = -(w[:, None, None] * G * resid[None, :, None]).sum(axis=1) / S
        g = np.concatenate((gw, gp.ravel()))
        m1 = ld(B1) * m1 + (1 - ld(B1)) * g
        m2 = ld(B2) * m2 + (1 - ld(B2)) * g ** 2
        x = x - ld(steps[i]) * m1 / (1 - ld(B1) ** (i + 1)) / (ld(EPS) + np.sqrt(m2 / (1 - ld(B2) ** (i + 1))))
        closest = min(closest, float(np.abs(x[:m]).min()))
        x[:m] = np.maximum(x[:m], 0.)
    return x[:m].astype(np.float64), x[m:].reshape(m, d).astype(np.float64), closest
