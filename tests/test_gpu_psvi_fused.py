"""BatchPSVICoreset's gradient in one native call (include/beta_cores_psvi.h; BatchPSVICoreset(fused_gradient=True)): the kernel
against the reference's expression in long double and against the unfused device path, golden F16 and whole builds through the
fused route, the cases it declines, and the C ABI.  The bound of tests 1 and 2 is tests/psvi_cases.py's, no constant changed."""
import ctypes as C

import numpy as np
import pytest

import psvi_cases as pc
from conftest import load_golden
from oracle import models_ref as M

pytestmark = pytest.mark.gpu
N_ROWS = 3000


@pytest.fixture(scope='module')
def bc():
    import beta_cores_amd as bc
    bc.default_context()
    return bc


def fixed(th):
    return lambda n, w, p: th


def model_of(bc, c):
    if c['kind'] == pc.LINREG:
        return bc.likelihoods.LinearRegression(c['sigsq'])
    if c['kind'] == pc.LOGISTIC:
        return bc.likelihoods.LogisticRegression()
    return bc.likelihoods.GaussianLocation(c['Siginv'], 0.)


_rows_cache = {}


def data_rows(bc, kind, d):
    """N_ROWS resident rows of the model's kind and width (one upload per (kind, d) for the whole module)"""
    if (kind, d) not in _rows_cache:
        rng = np.random.RandomState(31 * d + kind)
        x = rng.randn(N_ROWS, d)
        z = np.hstack((x, (x.dot(rng.randn(d)) + rng.randn(N_ROWS))[:, None])) if kind == pc.LINREG else x
        _rows_cache[kind, d] = bc.DeviceData(z)
    return _rows_cache[kind, d]


def check_kernel(bc, kind, sigsq, m, s, d):
    """tests 1 and 2 on one case; returns the worst error / bound ratios (fused against long double, fused against unfused)"""
    c = pc.make_case(kind, m, s, d, sigsq)
    dd = data_rows(bc, kind, d)
    prj = bc.DeviceProjector(fixed(c['theta']), s, model_of(bc, c))
    g_w, g_p, resid = prj.psvi_gradient(dd, c['pts'], c['w'], 1.7, want_resid=True)
    want_w, want_r = prj.vi_gradient(dd, c['pts'], c['w'], 1.7, want_resid=True)
    assert np.array_equal(g_w, want_w) and np.array_equal(resid, want_r)          # the bits of bc_vi_gradient
    again = prj.psvi_gradient(dd, c['pts'], c['w'], 1.7, want_resid=True)
    assert all(np.array_equal(a, b) for a, b in zip(again, (g_w, g_p, resid)))     # a second call: the same bits
    two = prj.psvi_gradient(dd, c['pts'], c['w'], 1.7)
    assert len(two) == 2 and np.array_equal(two[1], g_p)
    assert g_p.shape == c['pts'].shape
    if m > 1:
        assert c['w'][m // 2] == 0. and np.all(g_p[m // 2] == 0.)                  # a zero weight: an exactly zero row
    if kind == pc.LOGISTIC and d == 1:
        assert np.all(g_p == 0.)
    # 1. against the reference's expression in long double, on the residual the device has formed
    ref, bound = pc.reference(c, resid=resid)
    err = np.abs(g_p - ref)
    ratio = float((err / np.where(bound > 0, bound, 1.)).max())
    # 2. against the unfused device path: the project(grad=True) tensor contracted by bpsvi.py:80 (same Theta, same residual)
    _, pgrads = prj.project(c['pts'], grad=True)
    g_ref = -(c['w'][:, np.newaxis, np.newaxis] * pgrads * resid[np.newaxis, :, np.newaxis]).sum(axis=1) / s
    err2 = np.abs(g_p - g_ref)
    ratio2 = float((err2 / np.where(bound > 0, 2. * bound, 1.)).max())
    print('kind %d sigsq %.1f M %3d S %3d D %3d: fused - long double %.3e (ratio %.3f), fused - unfused %.3e (ratio %.3f)'
          % (kind, sigsq, m, s, d, float(err.max()), ratio, float(err2.max()), ratio2))
    assert np.all(err <= bound), (kind, sigsq, m, s, d, ratio)
    assert np.all(err2 <= bound + bound), (kind, sigsq, m, s, d, ratio2)            # bound(fused) + bound(unfused)
    return ratio, ratio2


@pytest.mark.parametrize('d', pc.DIMS)
def test_kernel_against_long_double_and_unfused(bc, d):
    assert pc.LD_OK
    worst = [0., 0.]
    for m, s in pc.SHAPES:
        for kind, sigsq in pc.MODELS:
            r = check_kernel(bc, kind, sigsq, m, s, d)
            worst = [max(worst[0], r[0]), max(worst[1], r[1])]
    print('worst ratios at D = %d: against long double %.3f, against the unfused path %.3f' % (d, worst[0], worst[1]))


@pytest.mark.parametrize('m,s,d', [(257, 64, 2), (5, 3, 513)])
def test_kernel_beyond_one_coordinate_per_thread_and_one_wave_of_points(bc, m, s, d):
    """More blocks than 256, W that is no multiple of 64, several coordinates per thread."""
    for kind, sigsq in pc.MODELS:
        check_kernel(bc, kind, sigsq, m, s, d)


# ---------------------------------------------------------------- 3. golden F16 through the fused route
def f16_problem(bc, g, tag):
    if tag == 'g':
        X, E, Si, ld = g['g_X'], g['g_E'], g['g_Siginv'], float(g['g_logdet'])
        d, S = X.shape[1], E.shape[0]

        def sampler(sz, wts, pts):
            if pts.shape[0] == 0:
                wts, pts = np.zeros(1), np.zeros((1, d))
            muw, LSigw, _ = bc.gaussian_weighted_post(np.zeros(d), np.eye(d), Si, pts, wts)
            return muw + E.dot(LSigw.T)
        return X, lambda: bc.DeviceProjector(sampler, S, bc.likelihoods.GaussianLocation(Si, ld))
    Z, E, sg = g['l_Z'], g['l_E'], float(g['l_sigsq'])
    D, S = Z.shape[1] - 1, E.shape[0]

    def sampler(sz, wts, pts):
        if pts.shape[0] == 0:
            wts, pts = np.zeros(1), np.zeros((1, D + 1))
        muw, LSigw, _ = M.linreg_weighted_post(np.zeros(D), np.eye(D), sg, pts, wts)
        return muw + E.dot(LSigw.T)
    return Z, lambda: bc.DeviceProjector(sampler, S, bc.likelihoods.LinearRegression(sg))


@pytest.mark.parametrize('tag', ['g', 'l'])
@pytest.mark.parametrize('mode,nsub', [('full', None), ('sub', 60)])
def test_f16_batch_psvi_fused(bc, tag, mode, nsub):
    g = load_golden('f16_bpsvi')
    data, mkprj = f16_problem(bc, g, tag)
    np.random.seed(160)
    alg = bc.BatchPSVICoreset(data, mkprj(), opt_itrs=6, n_subsample_opt=nsub, step_sched=lambda m: lambda i: 0.5 / (1. + i),
                              fused_gradient=True)
    done = 0
    for sz in (3, 5):
        alg.build(1, sz)
        assert alg.fused_gradient_calls - done == 6
        done = alg.fused_gradient_calls
        k = '%s_%s_%d' % (tag, mode, sz)
        np.testing.assert_array_equal(alg.idcs, g[k + '_idcs'])
        np.testing.assert_allclose(alg.wts, g[k + '_wts'], rtol=1e-7)
        np.testing.assert_allclose(alg.pts, g[k + '_pts'], rtol=1e-7, atol=1e-9)
    assert np.random.rand() == float(g['%s_%s_rng_after' % (tag, mode)])


# ---------------------------------------------------------------- 4. whole builds, fused against unfused
def build_problem(bc, model):
    """(rows (N_ROWS x dz), projector factory, the sampler's RandomState) with a posterior sampler on a stream of its own"""
    rng = np.random.RandomState({'linreg': 41, 'logistic': 42, 'gauss': 43}[model])
    S = 24
    if model == 'linreg':
        D = 6
        X = rng.randn(N_ROWS, D)
        Z = np.hstack((X, (X.dot(rng.randn(D)) + rng.randn(N_ROWS))[:, None]))
        mk = lambda r: (bc.samplers.LinregPosteriorSampler(np.zeros(D), np.eye(D), 1.5, rng=r), bc.likelihoods.LinearRegression(1.5))
    elif model == 'logistic':
        D = 5
        X = rng.randn(N_ROWS, D)
        y = np.where(rng.rand(N_ROWS) < 1. / (1. + np.exp(-X.dot(rng.randn(D)))), 1., -1.)
        Z = X * y[:, None]
        mk = lambda r: (bc.samplers.LogisticLaplaceSampler(np.zeros(D), solver='newton', rng=r), bc.likelihoods.LogisticRegression())
    else:
        D = 4
        q = rng.randn(D, D)
        Si = np.linalg.inv(q.dot(q.T) / D + np.eye(D))
        Si = (Si + Si.T) / 2.
        Z = rng.randn(N_ROWS, D) * 2. + 1.
        mk = lambda r: (bc.samplers.GaussianPosteriorSampler(np.zeros(D), np.eye(D), Si, rng=r), bc.likelihoods.GaussianLocation(Si, -np.linalg.slogdet(Si)[1]))

    def projector():
        r = np.random.RandomState(7)
        smp, lik = mk(r)
        return bc.DeviceProjector(smp, S, lik), r
    return Z, projector


def same_state(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('model', ['linreg', 'logistic', 'gauss'])
@pytest.mark.parametrize('source', ['host', 'resident', 'resident_f32'])
@pytest.mark.parametrize('nsub', [None, 200])
def test_whole_builds_fused_against_unfused(bc, model, source, nsub):
    Z, projector = build_problem(bc, model)
    if source == 'resident_f32':
        Z = Z.astype(np.float32)      # both legs read the same float32 rows
    out = []
    for fused in (False, True):
        rows = Z if source == 'host' else bc.DeviceData(Z, dtype=np.float32) if source == 'resident_f32' else bc.DeviceData(Z)
        prj, r = projector()
        np.random.seed(9)
        alg = bc.BatchPSVICoreset(rows, prj, opt_itrs=8, n_subsample_opt=nsub, step_sched=lambda m: lambda i: 0.3 / (1. + i),
                                  fused_gradient=fused)
        res = []
        for sz in (3, 7):
            alg.build(1, sz)
            res.append((alg.idcs.copy(), alg.wts.copy(), alg.pts.copy()))
        assert alg.fused_gradient_calls == (16 if fused else 0)
        out.append((res, np.random.get_state(), r.get_state()))
    for (i0, w0, p0), (i1, w1, p1) in zip(out[0][0], out[1][0]):
        np.testing.assert_array_equal(i1, i0)
        np.testing.assert_allclose(w1, w0, rtol=1e-5, atol=1e-12)
        np.testing.assert_allclose(p1, p0, rtol=1e-5, atol=1e-12)
    assert same_state(out[0][1], out[1][1])          # the global stream: choice() and the sub-samples' randint()
    assert same_state(out[0][2], out[1][2])          # the sampler's own stream (its look-ahead never runs past the last gradient)


# ---------------------------------------------------------------- 5. what the fused route declines
def counted(th):
    calls = [0]

    def sampler(n, w, p):
        calls[0] += 1
        return th
    return sampler, calls


def decline_legs(bc, rows, mkprj, sz, itrs=2):
    out = []
    for fused in (False, True):
        prj, calls = mkprj()
        np.random.seed(3)
        alg = bc.BatchPSVICoreset(rows, prj, opt_itrs=itrs, step_sched=lambda m: lambda i: 0.2 / (1. + i), fused_gradient=fused)
        alg.build(1, sz)
        assert alg.fused_gradient_calls == 0
        assert calls[0] == 1 + itrs                  # the projector's own first draw, then ONE per gradient
        out.append((alg.idcs.copy(), alg.wts.copy(), alg.pts.copy()))
    assert all(np.array_equal(a, b) for a, b in zip(*out))


def test_declines_more_than_256_samples(bc):
    rng = np.random.RandomState(1)
    Z, th = rng.randn(N_ROWS, 5), rng.randn(257, 5) * .3

    def mkprj():
        smp, calls = counted(th)
        return bc.DeviceProjector(smp, 257, bc.likelihoods.LogisticRegression()), calls
    assert mkprj()[0].psvi_gradient(Z, Z[:3], np.ones(3)) is None
    decline_legs(bc, Z, mkprj, 4)


def test_declines_points_beyond_the_staging_area(bc):
    from beta_cores_amd.coreset.projector import VI_MAX_CORE_DOUBLES
    rng = np.random.RandomState(2)
    D, sz = 599, 100
    assert (sz - 1) * (D + 2) <= VI_MAX_CORE_DOUBLES < sz * (D + 2)      # m (dz + 1) just above the limit
    X = rng.randn(N_ROWS, D)
    Z = np.hstack((X, (X.dot(rng.randn(D)) / np.sqrt(D) + rng.randn(N_ROWS))[:, None]))
    th = rng.randn(4, D) * .05

    def mkprj():
        smp, calls = counted(th)
        return bc.DeviceProjector(smp, 4, bc.likelihoods.LinearRegression(1.)), calls
    prj = mkprj()[0]
    assert prj.psvi_gradient(Z, Z[:sz], np.ones(sz)) is None and prj.psvi_gradient(Z, Z[:sz - 1], np.ones(sz - 1)) is not None
    assert prj.psvi_gradient(Z, Z[:0], np.ones(0)) is None                 # no points
    decline_legs(bc, Z, mkprj, sz)


def test_black_box_projector_ignores_the_flag(bc):
    rng = np.random.RandomState(4)
    Z, th = rng.randn(N_ROWS, 5), rng.randn(16, 5) * .3

    def mkprj():
        smp, calls = counted(th)
        return bc.BlackBoxProjector(smp, 16, M.logistic_loglik, M.logistic_grad_z_loglik), calls
    decline_legs(bc, Z, mkprj, 4)


def test_declines_an_encoder(bc):
    """There is no x-gradient through a feature encoder: psvi_gradient declines, and the existing path refuses the build exactly
    as it does with the flag off -- after ONE sampler call for the gradient that raised."""
    rng = np.random.RandomState(5)
    D = 6
    Z32 = rng.randn(N_ROWS, D + 1).astype(np.float32)
    enc = bc.encoders.MLPEncoder([(rng.randn(4, D) * 0.3, rng.randn(4) * 0.1, None, None, True)])
    th = rng.randn(8, 4) * .2
    for fused in (False, True):
        smp, calls = counted(th)
        prj = bc.DeviceProjector(smp, 8, bc.likelihoods.LinearRegression(1.), encoder=enc)
        rows = bc.DeviceData(Z32, dtype=np.float32)
        assert prj.psvi_gradient(rows, Z32[:3].astype(np.float64), np.ones(3)) is None
        np.random.seed(3)
        alg = bc.BatchPSVICoreset(rows, prj, opt_itrs=2, fused_gradient=fused)
        with pytest.raises(ValueError, match='feature encoder'):
            alg.build(1, 3)
        assert alg.fused_gradient_calls == 0 and calls[0] == 2


# ---------------------------------------------------------------- 6. the C ABI through ctypes
def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_c_abi(bc):
    from beta_cores_amd import _native as N
    lib = N.load()
    ctx = bc.default_context()
    rng = np.random.RandomState(6)
    D, S, m = 5, 12, 4
    X = rng.randn(N_ROWS, D)
    Z = np.hstack((X, (X.dot(rng.randn(D)) + rng.randn(N_ROWS))[:, None]))
    dd = bc.DeviceData(Z)
    pts, w, th, params = np.ascontiguousarray(Z[:m]), rng.rand(m) + .1, rng.randn(S, D) * .3, np.array([1.5])
    g_w, g_p, resid = np.empty(m), np.empty((m, D + 1)), np.empty(S)

    def begin(model=0, **nul):
        a = dict(ctx=ctx.h, data=dd.h, points=_p(pts), theta=_p(th), params=_p(params), w=_p(w))
        a.update(nul)
        return lib.bc_psvi_gradient_begin(a['ctx'], a['data'], a['points'], m, model, a['theta'], S, a['params'], 1, a['w'], 1.3)

    def nothing_pending():
        assert lib.bc_psvi_gradient_end(ctx.h, _p(g_w), _p(g_p), None) == N.BC_INVALID_ARGUMENT
        assert 'no gradient is pending' in N.last_error()
    nothing_pending()                                                      # _end without _begin
    for name in ('ctx', 'data', 'points', 'theta', 'params', 'w'):
        assert begin(**{name: None}) == N.BC_INVALID_ARGUMENT, name
        nothing_pending()
    for outs in ((None, _p(g_p)), (_p(g_w), None)):
        assert lib.bc_psvi_gradient(ctx.h, dd.h, _p(pts), m, 0, _p(th), S, _p(params), 1, _p(w), 1.3, outs[0], outs[1], None) == N.BC_INVALID_ARGUMENT
        nothing_pending()
    # a beta-likelihood has no x-gradient
    assert lib.bc_psvi_gradient_begin(ctx.h, dd.h, _p(pts), m, 1, _p(th), S, _p(np.array([1.5, .5])), 2, _p(w), 1.3) == N.BC_INVALID_ARGUMENT
    assert 'no x-gradient' in N.last_error()
    nothing_pending()
    # S > 256
    assert lib.bc_psvi_gradient_begin(ctx.h, dd.h, _p(pts), m, 0, _p(np.zeros((257, D))), 257, _p(params), 1, _p(w), 1.3) == N.BC_INVALID_ARGUMENT
    nothing_pending()
    # data of another context
    other = bc.Context()
    assert begin(ctx=other.h) == N.BC_INVALID_ARGUMENT and 'another context' in N.last_error()
    nothing_pending()
    # the one-call export
    want = (np.empty(m), np.empty((m, D + 1)), np.empty(S))
    assert lib.bc_psvi_gradient(ctx.h, dd.h, _p(pts), m, 0, _p(th), S, _p(params), 1, _p(w), 1.3, *[_p(a) for a in want]) == N.BC_OK, N.last_error()
    # begin; the other kinds' _end and the device weight optimisation are refused and leave it pending; then _end delivers it
    assert begin() == N.BC_OK, N.last_error()
    assert begin() == N.BC_INVALID_ARGUMENT and 'already pending' in N.last_error()
    plain = np.empty(m)
    assert lib.bc_vi_gradient_end(ctx.h, _p(plain), None) == N.BC_INVALID_ARGUMENT and 'bc_psvi_gradient_begin' in N.last_error()
    assert lib.bc_vi_beta_gradient_end(ctx.h, _p(plain), _p(np.empty(m)), None) == N.BC_INVALID_ARGUMENT
    sp = np.concatenate((np.zeros(D), np.eye(D).ravel(), [1.5]))
    step = np.ones((3, 2))
    assert lib.bc_vi_optimize_begin(ctx.h, dd.h, _p(pts), m, 0, _p(params), 1, 0, _p(sp), S, _p(w), 2, _p(step), 0, 1., 0) == N.BC_INVALID_ARGUMENT
    assert 'pending' in N.last_error()
    assert lib.bc_psvi_gradient_end(ctx.h, _p(g_w), _p(g_p), _p(resid)) == N.BC_OK, N.last_error()
    nothing_pending()
    assert all(np.array_equal(a, b) for a, b in zip((g_w, g_p, resid), want))      # bit for bit the one-call export
    # and both are what the Python layer returns
    prj = bc.DeviceProjector(fixed(th), S, bc.likelihoods.LinearRegression(1.5))
    assert all(np.array_equal(a, b) for a, b in zip(prj.psvi_gradient(dd, pts, w, 1.3, want_resid=True), want))
    # a pending plain gradient refuses this kind's _end in turn
    assert lib.bc_vi_gradient_begin(ctx.h, dd.h, _p(pts), m, 0, _p(th), S, _p(params), 1, _p(w), 1.3, None) == N.BC_OK
    assert lib.bc_psvi_gradient_end(ctx.h, _p(g_w), _p(g_p), None) == N.BC_INVALID_ARGUMENT and 'bc_vi_gradient_begin' in N.last_error()
    assert lib.bc_vi_gradient_end(ctx.h, _p(plain), None) == N.BC_OK and np.array_equal(plain, want[0])
