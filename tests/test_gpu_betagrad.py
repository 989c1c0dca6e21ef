"""d/dbeta of the linear- and logistic-regression beta-likelihoods on the device (K1 models 7 and 8,
include/beta_cores_betagrad.h), the fused (w, beta) gradient (bc_vi_beta_gradient) and BetaCoreset(learn_beta=True) through it.

`check` throughout: |device - centred(host closed form)| <= 1e-11 * (1 + max|raw|) element-wise plus the column-sum and norm
checks of tests/test_gpu_project.py::check_phi -- the projections' own bar; the bodies alone keep 1e-13 (tests/betagrad_harness.c)."""
import os

import numpy as np
import pytest

from conftest import load_golden

from oracle import models_ref as M
from oracle import coreset_ref as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def bc():
    import beta_cores_amd as bc
    bc.default_context()
    return bc


def fixed(th):
    return lambda n, w, p: th


def centred(raw):
    return raw - raw.mean(axis=1)[:, None]


def check(dev_phi, raw, tol=1e-11):
    ref = centred(raw)
    got = np.asarray(dev_phi)
    scale = 1. + np.abs(raw).max()
    assert got.shape == ref.shape
    assert np.all(np.isfinite(got))
    assert np.abs(got - ref).max() <= tol * scale, np.abs(got - ref).max() / scale
    np.testing.assert_allclose(dev_phi.colsum(), got.sum(axis=0), rtol=1e-10, atol=1e-9 * scale)
    np.testing.assert_allclose(dev_phi.norms(), np.sqrt((got ** 2).sum(axis=1)), rtol=1e-12, atol=1e-300)


def lin(bc, sigsq=1.3):
    return bc.likelihoods.LinearRegression(sigsq, beta_gradient=True)


def log(bc):
    return bc.likelihoods.LogisticRegression(beta_gradient=True)


# ------------------------------------------------------------------ the formulas on the golden inputs
def test_formulas_on_golden_linreg(bc):
    g = load_golden('f2_formulas')
    Z, th = g['lin_Z'], g['lin_th']
    for sig in (1.0, 2.5):
        model = lin(bc, sig)
        prj = bc.DeviceBetaProjector(fixed(th), th.shape[0], model)
        for beta in (0.1, 0.2, 0.5):
            bl, bg = prj.project_f(Z, beta, grad=True)
            check(bl, g['lin_bl_sig%g_b%g' % (sig, beta)])           # the value: the existing golden check
            check(bg, model.beta_gradient_host(Z, th, beta))


@pytest.mark.parametrize('which', ['f2', 'f22'])
def test_formulas_on_golden_logistic_incl_overflow_margins(bc, which):
    """F2's rows hold margins 120 and 800, F22's +-700 ... +-1500, on both sides of np.exp's overflow: the value follows the
    reference's jump there (golden), the gradient is that of the mathematical function (finite, no jump)."""
    if which == 'f2':
        g = load_golden('f2_formulas')
        Z, th, key = g['log_Z'], g['log_th'], 'log_bl_b%g'
    else:
        g = load_golden('f22_logistic_beta_overflow')
        Z, th, key = g['Z'], g['th'], 'bl_b%g'
    model = log(bc)
    prj = bc.DeviceBetaProjector(fixed(th), th.shape[0], model)
    for beta in (0.01, 0.05, 0.1, 0.5, 32.):
        bl, bg = prj.project_f(Z, beta, grad=True)
        check(bl, g[key % beta] if (key % beta) in g.files else M.logistic_beta_lik(Z, th, beta))
        raw = model.beta_gradient_host(Z, th, beta)
        assert np.isfinite(raw).all()
        check(bg, raw)


# ------------------------------------------------------------------ shapes: every NT template, partial tiles / D-chunks, the wide path
_SHAPES = [(1, 1, 1), (129, 33, 100), (1000, 100, 112), (129, 64, 113), (127, 100, 256), (1000, 64, 100), (129, 33, 257)]


def _inputs(kind, rng, n, d, s):
    if kind == 'lin':
        return rng.randn(n, d + 1), rng.randn(s, d) * (0.6 / np.sqrt(d))
    return rng.randn(n, d) * 2., rng.randn(s, d) * (1.5 / np.sqrt(d))


@pytest.mark.parametrize('n,d,s', _SHAPES)
@pytest.mark.parametrize('kind', ['lin', 'log'])
def test_shapes(bc, kind, n, d, s):
    rng = np.random.RandomState(n * 1000 + d * 10 + s)
    model = lin(bc) if kind == 'lin' else log(bc)
    Z, th = _inputs(kind, rng, n, d, s)
    if n > 10:
        Z[[3, n - 1], :d] = 0.                                         # constant rows
    prj = bc.DeviceBetaProjector(fixed(th), s, model)
    for beta in (0.05, 0.7):
        bl, bg = prj.project_f(Z, beta, grad=True)
        check(bl, M.linreg_beta_lik(Z, th, beta, 1.3) if kind == 'lin' else M.logistic_beta_lik(Z, th, beta))
        check(bg, model.beta_gradient_host(Z, th, beta))
        dd = bc.DeviceData(Z)                                          # resident float64 rows: the same kernel, the same bits
        assert np.array_equal(prj.project_f(dd, beta, grad=True)[1].to_host(), bg.to_host())


@pytest.mark.parametrize('kind', ['lin', 'log'])
def test_theta_resident_kernel_and_pipelined_host_rows(bc, kind):
    """n = 262 144 + 77, d = 37, S = 100: the smallest shape of test_theta_resident_kernel_matches_staged_and_oracle -- the
    Theta-resident K1, ragged N, masked columns -- from resident rows and from a live host array (upload and K1 pipelined,
    bc_project_from_host): the same bits; against the staged kernel to rounding; against the closed form on scattered rows."""
    n, d, s, beta = 262_144 + 77, 37, 100, 0.3
    rng = np.random.RandomState(77 + (kind == 'log'))
    model = lin(bc) if kind == 'lin' else log(bc)
    Z, th = _inputs(kind, rng, n, d, s)
    pick = np.unique(np.concatenate(([0, 1, 31, 32, 127, 128, n - 33, n - 32, n - 1], rng.choice(n, 300, replace=False))))
    Z[pick[5:8], :d] = 0.
    prj = bc.DeviceBetaProjector(fixed(th), s, model)
    dd = bc.DeviceData(Z)
    os.environ.pop('BC_K1_STAGED', None)
    res = prj.project_f(dd, beta, grad=True)[1]
    rows_r, norms_r, cs_r = res.rows(pick), res.norms(), res.colsum()
    del res
    host = prj.project_f(Z, beta, grad=True)[1]
    assert np.array_equal(host.rows(pick), rows_r) and np.array_equal(host.norms(), norms_r) and np.array_equal(host.colsum(), cs_r)
    del host
    os.environ['BC_K1_STAGED'] = '1'
    try:
        old = prj.project_f(dd, beta, grad=True)[1]
        rows_s, norms_s, cs_s = old.rows(pick), old.norms(), old.colsum()
        del old
    finally:
        os.environ.pop('BC_K1_STAGED', None)
    raw = model.beta_gradient_host(Z[pick], th, beta)
    ref = centred(raw)
    scale = 1. + np.abs(raw).max()
    assert np.abs(rows_r - ref).max() <= 1e-11 * scale
    assert np.abs(rows_r - rows_s).max() <= 1e-12 * scale
    np.testing.assert_allclose(norms_r, norms_s, rtol=1e-11, atol=1e-13 * scale)
    np.testing.assert_allclose(cs_r, cs_s, rtol=1e-9, atol=1e-9 * scale)
    np.testing.assert_allclose(norms_r[pick], np.sqrt((ref ** 2).sum(axis=1)), rtol=1e-9, atol=1e-12 * scale)


@pytest.mark.parametrize('n,d,s', [(1000, 33, 100), (129, 20, 257), (5000, 64, 64)])
@pytest.mark.parametrize('kind', ['lin', 'log'])
def test_float32_rows_give_the_bits_of_the_widened_rows(bc, kind, n, d, s):
    rng = np.random.RandomState(n + d + s)
    model = lin(bc) if kind == 'lin' else log(bc)
    Z, th = _inputs(kind, rng, n, d, s)
    z32 = Z.astype(np.float32)
    prj = bc.DeviceBetaProjector(fixed(th), s, model)
    a = prj.project_f(bc.DeviceData(z32, dtype=np.float32), 0.3, grad=True)[1]
    b = prj.project_f(bc.DeviceData(z32.astype(np.float64)), 0.3, grad=True)[1]
    assert np.array_equal(a.to_host(), b.to_host()) and np.array_equal(a.norms(), b.norms()) and np.array_equal(a.colsum(), b.colsum())
    check(a, model.beta_gradient_host(z32.astype(np.float64), th, 0.3))


# ------------------------------------------------------------------ the fused (w, beta) gradient
def _grad_models(bc, rng, d):
    Sig = np.diag(rng.uniform(0.5, 2.0, d))
    return [('linreg', lin(bc), d + 1, 0.3), ('logistic', log(bc), d, 0.2),
            ('gauss', bc.likelihoods.GaussianLocation(np.linalg.inv(Sig), np.linalg.slogdet(Sig)[1]), d, 0.5)]


@pytest.mark.parametrize('m', [1, 7, 130, 300])
def test_fused_beta_gradient_matches_vi_gradient_and_host_algebra(bc, m):
    """grad and resid: the bits of bc_vi_gradient for the same inputs.  beta_dots: G.dot(resid) from the materialised
    beta-gradient of the coreset rows, with the tolerances of test_fused_gradient_matches_host_algebra."""
    rng = np.random.RandomState(m)
    n, d, s = 20000, 24, 100
    for name, model, dz, beta in _grad_models(bc, rng, d):
        Z = rng.randn(n, dz)
        th = rng.randn(s, d) * 0.3
        prj = bc.DeviceBetaProjector(fixed(th), s, model)
        dd = bc.DeviceData(Z)
        core = Z[rng.choice(n, m, replace=False)]
        w = rng.uniform(0., 3., m)
        bg = np.asarray(prj.project_f(core, beta, grad=True)[1])
        for scale in (1., 2.5):
            want_g, want_r = prj.vi_gradient(dd, core, w, scale, beta=beta, want_resid=True)
            got_g, dots, got_r = prj.vi_gradient(dd, core, w, scale, beta=beta, want_resid=True, want_beta_grad=True)
            assert np.array_equal(got_g, want_g) and np.array_equal(got_r, want_r), name
            want_d = bg.dot(got_r)
            np.testing.assert_allclose(dots, want_d, rtol=1e-11, atol=1e-12 * np.abs(want_d).max(), err_msg=name)
            g2, d2 = prj.vi_gradient(dd, core, w, scale, beta=beta, want_beta_grad=True)      # without the residual
            assert np.array_equal(g2, got_g) and np.array_equal(d2, dots)


def test_fused_beta_gradient_survives_library_calls_between_begin_and_end(bc):
    rng = np.random.RandomState(78)
    n, d, s, m = 100_000, 32, 100, 40
    Z = rng.randn(n, d + 1)
    th = rng.randn(s, d) * 0.3
    model = lin(bc)
    prj = bc.DeviceBetaProjector(fixed(th), s, model)
    other = bc.DeviceProjector(fixed(rng.randn(s, d)), s, model)
    dd = bc.DeviceData(Z)
    core = Z[rng.choice(n, m, replace=False)]
    w = rng.uniform(0., 3., m)
    want = prj.vi_gradient(dd, core, w, 1.7, beta=0.2, want_resid=True, want_beta_grad=True)
    side = {}

    def meddle():
        side['gram'] = bc.weighted_gram(core, w)
        side['phi'] = other.project(Z[:5000]).colsum()
        side['cs'] = other.colsum(dd)
        side['bg'] = prj.project_f(core, 0.4, grad=True)[1].colsum()      # re-stages Theta and the constants of model 7
    for _ in range(2):
        got = prj.vi_gradient(dd, core, w, 1.7, beta=0.2, want_resid=True, want_beta_grad=True, overlap=meddle)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
    assert np.array_equal(side['cs'], other.project(dd).colsum())


def _native_args(bc, prj, dd, core, w, beta):
    from beta_cores_amd.device import _ptr
    theta = prj.model.theta_for_device(prj.samples)
    params = np.ascontiguousarray(prj.model.params(beta=beta), dtype=np.float64)
    keep = (theta, params, core, w)
    return keep, (prj.ctx.h, dd.h, _ptr(core), core.shape[0], int(prj.model.beta_model_id), _ptr(theta), theta.shape[0], _ptr(params),
                  int(params.shape[0]), _ptr(w), 1.0, None)


def test_pending_state_is_shared_and_wrong_kind_end_is_refused(bc):
    from beta_cores_amd import _native as N
    from beta_cores_amd.device import _ptr
    rng = np.random.RandomState(9)
    n, d, s, m = 3000, 12, 64, 9
    Z = rng.randn(n, d + 1)
    prj = bc.DeviceBetaProjector(fixed(rng.randn(s, d) * 0.3), s, lin(bc))
    dd = bc.DeviceData(Z)
    core = np.ascontiguousarray(Z[:m])
    w = rng.uniform(0., 3., m)
    keep, args = _native_args(bc, prj, dd, core, w, 0.3)
    want_g, want_d, want_r = prj.vi_gradient(dd, core, w, 1., beta=0.3, want_resid=True, want_beta_grad=True)
    g, dots, r = np.empty(m), np.empty(m), np.empty(s)
    h = prj.ctx.h
    # a beta gradient is pending: a begin of either kind and the plain end are refused, the result survives
    N.call('bc_vi_beta_gradient_begin', *args)
    for name, a in (('bc_vi_gradient_begin', args), ('bc_vi_beta_gradient_begin', args), ('bc_vi_gradient_end', (h, _ptr(g), _ptr(r))),
                    ('bc_vi_beta_gradient_end', (h, _ptr(g), None, _ptr(r))), ('bc_vi_beta_gradient_end', (h, None, _ptr(dots), None))):
        with pytest.raises(ValueError):
            N.call(name, *a)
    N.call('bc_vi_beta_gradient_end', h, _ptr(g), _ptr(dots), _ptr(r))
    assert np.array_equal(g, want_g) and np.array_equal(dots, want_d) and np.array_equal(r, want_r)
    with pytest.raises(ValueError):                                   # nothing is pending any more
        N.call('bc_vi_beta_gradient_end', h, _ptr(g), _ptr(dots), _ptr(r))
    # the other way round
    N.call('bc_vi_gradient_begin', *args)
    with pytest.raises(ValueError):
        N.call('bc_vi_beta_gradient_begin', *args)
    with pytest.raises(ValueError):
        N.call('bc_vi_beta_gradient_end', h, _ptr(g), _ptr(dots), _ptr(r))
    g2, r2 = np.empty(m), np.empty(s)
    N.call('bc_vi_gradient_end', h, _ptr(g2), _ptr(r2))
    assert np.array_equal(g2, want_g) and np.array_equal(r2, want_r)
    del keep


def test_null_arguments_and_unsupported_forms_are_refused(bc):
    from beta_cores_amd import _native as N
    from beta_cores_amd.device import _ptr
    rng = np.random.RandomState(10)
    n, d, s, m = 500, 6, 32, 4
    Z = rng.randn(n, d + 1)
    th = rng.randn(s, d) * 0.3
    prj = bc.DeviceBetaProjector(fixed(th), s, lin(bc))
    dd = bc.DeviceData(Z)
    core = np.ascontiguousarray(Z[:m])
    w = rng.uniform(0., 3., m)
    keep, args = _native_args(bc, prj, dd, core, w, 0.3)
    for i in (0, 1, 2, 5, 7, 9):                                       # ctx, data, core_rows, theta, params, w
        bad = list(args)
        bad[i] = None
        with pytest.raises(ValueError):
            N.call('bc_vi_beta_gradient_begin', *bad)
    for model in (0, 2, 4, 6, 7, 8, 9):                                # not a beta-likelihood that has a beta-gradient
        bad = list(args)
        bad[4] = model
        with pytest.raises(ValueError):
            N.call('bc_vi_beta_gradient_begin', *bad)
    g, dots = np.empty(m), np.empty(m)
    with pytest.raises(ValueError):
        N.call('bc_vi_beta_gradient', *(args + (None, _ptr(dots), None)))
    with pytest.raises(ValueError):
        N.call('bc_vi_beta_gradient', *(args + (_ptr(g), None, None)))
    N.call('bc_vi_beta_gradient', *(args + (_ptr(g), _ptr(dots), None)))      # nothing was left pending by the refusals
    want = prj.vi_gradient(dd, core, w, 1., beta=0.3, want_beta_grad=True)
    assert np.array_equal(g, want[0]) and np.array_equal(dots, want[1])
    # the store-free forms of models 7 and 8 do not exist (include/beta_cores_betagrad.h): refused, not approximated
    out = np.empty(s)
    p_lin, p_log = np.array([1.3, 0.3]), np.array([0.3])
    ddl = bc.DeviceData(np.ascontiguousarray(Z[:, :d]))
    for data, model, p in ((dd, 7, p_lin), (ddl, 8, p_log)):
        with pytest.raises(ValueError, match='store-free'):
            N.call('bc_project_colsum', prj.ctx.h, data.h, model, _ptr(th), s, _ptr(p), int(p.shape[0]), None, _ptr(out))
        with pytest.raises(ValueError, match='store-free'):
            N.call('bc_vi_gradient', prj.ctx.h, data.h, _ptr(core), m, model, _ptr(th), s, _ptr(p), int(p.shape[0]), _ptr(w), 1.0, None,
                   _ptr(g), None)
    # the models the projector was not given a beta-gradient for keep the reference's error
    plain = bc.DeviceBetaProjector(fixed(th), s, bc.likelihoods.LinearRegression(1.3))
    with pytest.raises(ValueError):
        plain.vi_gradient(dd, core, w, 1., beta=0.3, want_beta_grad=True)
    with pytest.raises(ValueError):
        plain.project_f(Z, 0.3, grad=True)
    with pytest.raises(ValueError):                                    # the value model's range of beta, kept
        bc.DeviceBetaProjector(fixed(th), s, log(bc)).project_f(Z[:, :d], 33., grad=True)
    del keep


# ------------------------------------------------------------------ end to end: BetaCoreset(learn_beta=True)
def e2e_inputs(kind, n):
    """The recipe of test_fused_optimise_equals_general_path_and_oracle: D = 8, S = 64, 10 % outliers.  Returns Z, the sampler
    sampler(sz, wts, pts), the oracle's beta-likelihood (pts, th, beta) and a factory of the model from the likelihoods module."""
    rng = np.random.RandomState(5 + n)
    D, S = 8, 64
    X = rng.randn(n, D)
    out = rng.choice(n, n // 10, replace=False)
    E = rng.randn(S, D)
    if kind == 'lin':
        y = X.dot(rng.randn(D)) + rng.randn(n)
        y[out] = rng.normal(10., .5, out.shape[0])
        Z = np.hstack((X, y[:, None]))

        def sampler(sz, wts, pts):
            if pts.shape[0] == 0:
                wts, pts = np.zeros(1), np.zeros((1, Z.shape[1]))
            mu, L, _ = M.linreg_weighted_post(np.zeros(D), np.eye(D), 1.0, pts, wts)
            return mu + E.dot(L.T)
        return Z, sampler, (lambda z, t, b: M.linreg_beta_lik(z, t, b, 1.0)), (lambda L: L.LinearRegression(1.0, beta_gradient=True))
    tstar = np.full(D, 1. / np.sqrt(D))
    y = np.where(rng.rand(n) < 1. / (1. + np.exp(-X.dot(tstar))), 1., -1.)
    y[out] = -y[out]                                                   # outliers: flipped labels
    Z = y[:, None] * X
    th = tstar + 0.3 * E
    return Z, (lambda sz, wts, pts: th), M.logistic_beta_lik, (lambda L: L.LogisticRegression(beta_gradient=True))


E2E_ITS, E2E_BETA0, E2E_BUILDS = 6, 0.5, 5
e2e_sched = lambda i: 0.03 / (1. + i)


def e2e_oracle(kind, n, nsub):
    Z, sampler, beta_lik, mk = e2e_inputs(kind, n)
    from beta_cores_amd import likelihoods
    model = mk(likelihoods)
    np.random.seed(11)
    ref = C.RefGreedyVI(Z, lambda pts, th, b: C.project_f(beta_lik, pts, th, b), lambda w, p: sampler(64, w, p), E2E_ITS, e2e_sched,
                        n_subsample_select=nsub, n_subsample_opt=nsub, beta=E2E_BETA0, learn_beta=True,
                        beta_grad=lambda pts, th, b: centred(model.beta_gradient_host(pts, th, b)))
    trace = []
    for _ in range(E2E_BUILDS):
        ref.build(1)
        trace.append((ref.idcs.copy(), ref.wts.copy(), float(ref.beta)))
    return trace, np.random.rand()


@pytest.mark.parametrize('nsub', [None, 500])
@pytest.mark.parametrize('n', [3000, 9000])
@pytest.mark.parametrize('kind', ['lin', 'log'])
def test_learn_beta_fused_equals_materialising_and_oracle(bc, kind, n, nsub):
    """beta_0 = 0.5, step 0.03 / (1 + i), opt_itrs = 6, five build(1, .) calls; full data, and n_subsample_* = 500 on resident
    (pinned) rows.  Fused route and fused_gradient=False against the oracle with the centred host closed form as beta-gradient:
    same selections, weights and beta within rtol 1e-5 (F15's bars), the same RNG position; fused against materialising within
    1e-9; the fused run makes exactly 5 * opt_itrs native calls."""
    Z, sampler, _, mk = e2e_inputs(kind, n)
    want, rng_ref = e2e_oracle(kind, n, nsub)

    def run(fused):
        prj = bc.DeviceBetaProjector(sampler, 64, mk(bc.likelihoods))
        if nsub is not None:
            prj.pin(Z)                                                 # resident rows: the sub-samples are drawn on the device
        calls = {'n': 0}
        orig = prj.vi_gradient

        def counted(*a, **kw):
            calls['n'] += 1
            assert kw.get('want_beta_grad')
            return orig(*a, **kw)
        prj.vi_gradient = counted
        np.random.seed(11)
        alg = bc.BetaCoreset(Z, prj, opt_itrs=E2E_ITS, step_sched=e2e_sched, beta=E2E_BETA0, learn_beta=True, fused_gradient=fused,
                             n_subsample_select=nsub, n_subsample_opt=nsub)
        trace = []
        for k in range(E2E_BUILDS):
            alg.build(1, k + 1)
            trace.append((alg.idcs.copy(), alg.wts.copy(), float(alg.beta)))
        pos = np.random.rand()
        prj.forget()
        return trace, pos, calls['n']
    a, rng_a, calls_a = run(True)
    b, rng_b, calls_b = run(False)
    assert calls_a == E2E_BUILDS * E2E_ITS and calls_b == 0
    assert rng_a == rng_ref and rng_b == rng_ref
    for (ia, wa, ba), (ib, wb, bb), (ir, wr, br) in zip(a, b, want):
        np.testing.assert_array_equal(ia, ir)
        np.testing.assert_array_equal(ib, ir)
        np.testing.assert_allclose(wa, wr, rtol=1e-5, atol=1e-12)
        np.testing.assert_allclose(wb, wr, rtol=1e-5, atol=1e-12)
        np.testing.assert_allclose([ba, bb], [br, br], rtol=1e-5)
        np.testing.assert_allclose(wa, wb, rtol=1e-9, atol=1e-13)
        np.testing.assert_allclose(ba, bb, rtol=1e-9)
    assert 0. < a[-1][2] < E2E_BETA0                                   # beta moved, and stayed away from the projection at 0


def test_gaussian_learn_beta_takes_the_fused_route(bc):
    """The model that always had a beta-gradient: learn_beta now goes through bc_vi_beta_gradient too, and agrees with the
    materialising route (golden F15 pins both against the reference in tests/test_gpu_coresets.py)."""
    g = load_golden('f15_learn_beta')
    X, E, Si, ld = g['X'], g['E'], g['Siginv'], float(g['logdet'])
    d, S = X.shape[1], E.shape[0]

    def sampler(sz, wts, pts):
        if pts.shape[0] == 0:
            wts, pts = np.zeros(1), np.zeros((1, d))
        muw, LSigw, _ = bc.gaussian_weighted_post(np.zeros(d), np.eye(d), Si, pts, wts)
        return muw + E.dot(LSigw.T)
    res = []
    for fused in (True, False):
        prj = bc.DeviceBetaProjector(sampler, S, bc.likelihoods.GaussianLocation(Si, ld))
        calls = {'n': 0}
        orig = prj.vi_gradient

        def counted(*a, _orig=orig, _c=calls, **kw):
            _c['n'] += 1
            return _orig(*a, **kw)
        prj.vi_gradient = counted
        alg = bc.BetaCoreset(X, prj, opt_itrs=8, step_sched=lambda i: 0.1 / (1. + i), beta=.3, learn_beta=True, fused_gradient=fused)
        for k in range(3):
            alg.build(1, k + 1)
        res.append((alg.idcs.copy(), alg.wts.copy(), alg.beta, calls['n']))
    assert res[0][3] == 3 * 8 and res[1][3] == 0
    np.testing.assert_array_equal(res[0][0], res[1][0])
    np.testing.assert_allclose(res[0][1], res[1][1], rtol=1e-9, atol=1e-13)
    np.testing.assert_allclose(res[0][2], res[1][2], rtol=1e-9)


def test_without_the_flag_learn_beta_still_raises(bc):
    g = load_golden('f5_greedy_vi')
    Z, E = g['Z'], g['E']
    D = Z.shape[1] - 1

    def sampler(sz, wts, pts):
        if pts.shape[0] == 0:
            wts, pts = np.zeros(1), np.zeros((1, Z.shape[1]))
        mu, L, _ = M.linreg_weighted_post(np.zeros(D), np.eye(D), 1.0, pts, wts)
        return mu + E.dot(L.T)
    alg = bc.BetaCoreset(Z, bc.DeviceBetaProjector(sampler, E.shape[0], bc.likelihoods.LinearRegression(1.0)), opt_itrs=2, beta=0.1)
    with pytest.raises(ValueError):
        alg.build(1, 1)
