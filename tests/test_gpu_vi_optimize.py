"""The greedy-VI weight optimisation on the device (include/beta_cores_viopt.h; GreedyVICoreset(device_optimize=True)) against
the host loop it replaces -- the same draws, step by step -- and against the oracle and the goldens.

The device's Cholesky and E . L^T do not have LAPACK's / BLAS's bits, so the bar is the project's parity contract:
selections exact, weights within rtol = 1e-5, atol = 1e-12; the RNG position after a run exactly the host loop's.  The worst
deviations seen are recorded in profiles/vi_optimize_notes.md."""
import numpy as np
import pytest

import vi_sampler_cases as vc
from conftest import load_golden
from oracle import coreset_ref as C
from oracle import models_ref as M

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-5, 1e-12
ITRS = 8


@pytest.fixture(scope='module')
def bc():
    import beta_cores_amd as bc
    bc.default_context()
    return bc


def linreg_rows(n, D, seed):
    rng = np.random.RandomState(seed)
    X = rng.randn(n, D)
    y = X.dot(rng.randn(D) / np.sqrt(D)) + rng.randn(n)
    return np.hstack((X, y[:, None]))


def gauss_rows(n, d, seed):
    rng = np.random.RandomState(seed)
    return rng.randn(n, d) * 2. + 1.


def make_alg(bc, kind, rows, dd, S, m, seed, nsub, device, sched=None, itrs=ITRS, Sig0_sign=1., w_scale=None, th0=None, Sig0inv=None,
             sigsq=1.0, mu0=None):
    """A coreset of m given rows with weights w0, ready for _optimize().  kind: 'svi' / 'bcores' (linear regression, rows
    [x, y]) or 'gauss' (SparseVI on the Gaussian location model).  The sampler draws its normals from RandomState(seed).
    The prior: th0 (linear regression) / mu0 (Gaussian) default to 0, Sig0inv to Sig0_sign * I, sigsq to 1."""
    n, dz = rows.shape
    rng = np.random.RandomState(seed + 77)
    if kind == 'gauss':
        d = dz
        q = rng.randn(d, d)
        Siginv = np.linalg.inv(q.dot(q.T) / d + 2. * np.eye(d))
        Siginv = (Siginv + Siginv.T) / 2.
        sampler = bc.samplers.GaussianPosteriorSampler(np.zeros(d) if mu0 is None else mu0, Sig0_sign * np.eye(d) if Sig0inv is None else Sig0inv,
                                                       Siginv, rng=np.random.RandomState(seed))
        model = bc.likelihoods.GaussianLocation(Siginv, -np.linalg.slogdet(Siginv)[1])
    else:
        d = dz - 1
        sampler = bc.samplers.LinregPosteriorSampler(np.zeros(d) if th0 is None else th0, Sig0_sign * np.eye(d) if Sig0inv is None else Sig0inv,
                                                     sigsq, rng=np.random.RandomState(seed))
        model = bc.likelihoods.LinearRegression(sigsq)
    kw = dict(opt_itrs=itrs, n_subsample_opt=nsub, device_optimize=device)
    if sched is not None:
        kw['step_sched'] = sched
    if kind == 'bcores':
        alg = bc.BetaCoreset(dd, bc.DeviceBetaProjector(sampler, S, model), beta=0.5, learn_beta=False, **kw)
    else:
        alg = bc.SparseVICoreset(dd, bc.DeviceProjector(sampler, S, model), **kw)
    idcs = rng.choice(n, m, replace=False)
    alg._append(list(idcs), rows[idcs])
    w0 = rng.rand(m) * (float(n) / m if w_scale is None else w_scale)
    w0[rng.rand(m) < 0.2] = 0.
    w0[0] = (float(n) / m if w_scale is None else w_scale)
    alg.wts = w0.copy()
    return alg


def host_run(bc, *a, **kw):
    """(final weights, weights after every step, np.random.rand() afterwards) of the host loop."""
    alg = make_alg(bc, *a, device=False, **kw)
    seen, upd = [], alg.ll_projector.update

    def update(w, p):
        seen.append(np.array(w, dtype=np.float64))
        return upd(w, p)
    alg.ll_projector.update = update
    np.random.seed(a[5])
    alg._optimize()
    assert alg.device_optimize_calls == 0 and len(seen) == alg.opt_itrs
    return alg.wts.copy(), np.array(seen[1:] + [alg.wts]), np.random.rand()


def device_run(bc, *a, chunk_steps=0, **kw):
    alg = make_alg(bc, *a, device=True, **kw)
    prj, got = alg.ll_projector, {}
    run = prj.vi_optimize

    def vi_optimize(*args, **k):
        res = run(*args, want_trace=True, chunk_steps=chunk_steps, **k)
        if res is None:
            return None
        got['trace'] = res[1]
        return res[0]
    prj.vi_optimize = vi_optimize
    np.random.seed(a[5])
    alg._optimize()
    assert alg.device_optimize_calls == 1 and prj.vi_optimize_calls == 1
    return alg.wts.copy(), got['trace'], np.random.rand()


def compare(host, dev, tag):
    hw, ht, hr = host
    dw, dt, dr = dev
    with np.errstate(divide='ignore', invalid='ignore'):
        rel = np.where(ht != 0., np.abs(dt - ht) / np.abs(ht), np.abs(dt - ht))
    print('%s: worst relative deviation of the trace %.3e, of the final weights %.3e' % (tag, rel.max(), rel[-1].max()))
    # (a weight below ATOL can be far off relatively and still inside the contract; this figure is <= 1 exactly when it holds)
    print('%s: worst |device - host| / (ATOL + RTOL |host|) of the trace %.3e' % (tag, (np.abs(dt - ht) / (ATOL + RTOL * np.abs(ht))).max()))
    assert np.array_equal(dt[-1], dw)
    np.testing.assert_allclose(dt, ht, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(dw, hw, rtol=RTOL, atol=ATOL)
    assert hr == dr, 'the global stream does not stand where the host loop leaves it'


SHAPES = [(3000, 1, 5, 1), (3000, 3, 16, 7), (9000, 8, 64, 65), (9000, 33, 100, 130), (5000, 64, 100, 100), (4000, 128, 256, 100)]
_rows_cache = {}


def resident(bc, key, make, dtype=None):
    """Rows and their device copy, made once and shared (never modified) by the tests that use the same shape."""
    if key not in _rows_cache:
        rows = make()
        if dtype is not None:
            rows = rows.astype(dtype)
        _rows_cache[key] = (rows, bc.DeviceData(rows, dtype=dtype))
    return _rows_cache[key]


@pytest.mark.parametrize('nsub', [None, 50, 1000])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'n%d-D%d-S%d-m%d' % s)
def test_device_loop_equals_the_host_loop_on_the_same_draws(bc, shape, nsub):
    n, D, S, m = shape
    rows, dd = resident(bc, ('lin', n, D), lambda: linreg_rows(n, D, 10 + D))
    args = ('svi', rows, dd, S, m, 100 + D, nsub)
    compare(host_run(bc, *args), device_run(bc, *args), 'linreg ll n=%d D=%d S=%d m=%d nsub=%s' % (n, D, S, m, nsub))


@pytest.mark.parametrize('nsub', [None, 300])
def test_float32_rows(bc, nsub):
    rows, dd = resident(bc, ('lin32', 6000, 16), lambda: linreg_rows(6000, 16, 3), dtype=np.float32)
    args = ('svi', rows.astype(np.float64), dd, 64, 40, 7, nsub)
    compare(host_run(bc, *args), device_run(bc, *args), 'float32 rows nsub=%s' % nsub)


@pytest.mark.parametrize('nsub', [None, 300])
def test_gaussian_location(bc, nsub):
    rows, dd = resident(bc, ('gauss', 5000, 8), lambda: gauss_rows(5000, 8, 4))
    args = ('gauss', rows, dd, 200, 30, 11, nsub)
    compare(host_run(bc, *args), device_run(bc, *args), 'gaussian d=8 S=200 nsub=%s' % nsub)


@pytest.mark.parametrize('kind', ['bcores', 'svi'])
def test_beta_likelihood_and_plain_log_likelihood(bc, kind):
    rows, dd = resident(bc, ('lin', 9000, 8), lambda: linreg_rows(9000, 8, 18))
    args = (kind, rows, dd, 64, 20, 5, 200)
    compare(host_run(bc, *args), device_run(bc, *args), kind)


def test_chunk_boundary_does_not_change_the_bits(bc):
    rows, dd = resident(bc, ('lin', 9000, 8), lambda: linreg_rows(9000, 8, 18))
    for nsub in (None, 200):
        args = ('svi', rows, dd, 64, 20, 5, nsub)
        one = device_run(bc, *args, itrs=7)
        three = device_run(bc, *args, itrs=7, chunk_steps=3)
        assert np.array_equal(one[0], three[0]) and np.array_equal(one[1], three[1]) and one[2] == three[2]


def test_clamping_at_zero(bc):
    rows, dd = resident(bc, ('lin', 9000, 8), lambda: linreg_rows(9000, 8, 18))
    args = ('svi', rows, dd, 64, 20, 5, None)
    kw = dict(sched=lambda i: 400. / (1. + i), w_scale=100.)
    host = host_run(bc, *args, **kw)
    assert (host[0] == 0.).any() and (host[0] > 0.).any(), 'the schedule no longer drives a weight to exactly 0: the case has vanished'
    dev = device_run(bc, *args, **kw)
    compare(host, dev, 'clamping')
    assert np.array_equal(dev[0] == 0., host[0] == 0.)


# ---------------------------------------------------------------- whole builds
def _global_linreg_sampler(D):
    def sampler(w, p):
        if p.shape[0] == 0:
            w, p = np.zeros(1), np.zeros((1, D + 1))
        mu, L, _ = M.linreg_weighted_post(np.zeros(D), np.eye(D), 1.0, p, w)
        return mu + np.random.randn(64, D).dot(L.T)
    return sampler


@pytest.mark.parametrize('n,nsub', [(3000, None), (9000, 200)])
@pytest.mark.parametrize('kind', ['bcores', 'svi'])
def test_whole_builds(bc, kind, n, nsub):
    D, S, beta, itrs = 8, 64, 0.5, 7
    rows, dd = resident(bc, ('lin', n, D), lambda: linreg_rows(n, D, 10 + D))
    sched = lambda i: 1. / (1. + i)
    model = bc.likelihoods.LinearRegression(1.0)

    def make(device):
        sampler = bc.samplers.LinregPosteriorSampler(np.zeros(D), np.eye(D), 1.0)
        if kind == 'bcores':
            return bc.BetaCoreset(dd, bc.DeviceBetaProjector(sampler, S, model), beta=beta, learn_beta=False, opt_itrs=itrs,
                                  n_subsample_opt=nsub, step_sched=sched, device_optimize=device)
        return bc.SparseVICoreset(dd, bc.DeviceProjector(sampler, S, model), opt_itrs=itrs, n_subsample_opt=nsub, step_sched=sched,
                                  device_optimize=device)
    out = {}
    for device in (False, True):
        np.random.seed(31)
        alg = make(device)
        steps = []
        for m in range(5):
            alg.build(1, m + 1)
            steps.append((alg.idcs.copy(), alg.wts.copy()))
        out[device] = (steps, np.random.rand(), alg.device_optimize_calls, alg.ll_projector.vi_optimize_calls)
    assert out[False][2] == 0 and out[True][2] == 5 and out[True][3] == 5      # every _optimize() took the native call
    np.random.seed(31)
    ref_sampler = _global_linreg_sampler(D)
    ref_sampler(np.zeros(0), np.zeros((0, D + 1)))                                # the projector's constructor draw
    if kind == 'bcores':
        proj = lambda pts, th: C.project_f(lambda z, t, b: M.linreg_beta_lik(z, t, b, 1.0), pts, th, beta)
    else:
        proj = lambda pts, th: C.project(lambda z, t: M.linreg_loglik(z, t, 1.0), pts, th)
    ref = C.RefGreedyVI(rows, proj, ref_sampler, itrs, sched, n_subsample_opt=nsub, size_check_always=(kind == 'svi'))
    worst = 0.
    for m in range(5):
        ref.build(1)
        for device in (False, True):
            idcs, wts = out[device][0][m]
            np.testing.assert_array_equal(idcs, ref.idcs)
            np.testing.assert_allclose(wts, ref.wts, rtol=RTOL, atol=ATOL)
        np.testing.assert_array_equal(out[True][0][m][0], out[False][0][m][0])
        np.testing.assert_allclose(out[True][0][m][1], out[False][0][m][1], rtol=RTOL, atol=ATOL)
        hw, dw = out[False][0][m][1], out[True][0][m][1]
        worst = max(worst, float(np.max(np.abs(dw - hw) / np.maximum(np.abs(hw), 1e-300) * (hw != 0.))))
    print('%s n=%d nsub=%s: worst relative deviation device vs host build %.3e' % (kind, n, nsub, worst))
    ref_rng = np.random.rand()
    assert out[False][1] == ref_rng and out[True][1] == ref_rng


# ---------------------------------------------------------------- goldens
class _FixedNormals:
    """An `rng` stand-in whose randn returns the golden's E."""

    def __init__(self, E):
        self.E = E

    def randn(self, n, d):
        assert (n, d) == self.E.shape
        return self.E.copy()


@pytest.mark.parametrize('nm', ['bcores', 'svi'])
def test_f5_greedy_vi_goldens_with_the_device_loop(bc, nm):
    g = load_golden('f5_greedy_vi')
    Z, E = np.array(g['Z']), np.array(g['E'])
    S, D = E.shape
    beta, opt_itrs = float(g['beta']), int(g['opt_itrs'])
    sampler = bc.samplers.LinregPosteriorSampler(np.zeros(D), np.eye(D), 1.0, rng=_FixedNormals(E))
    model = bc.likelihoods.LinearRegression(1.0)
    sched = lambda i: 0.1 / (1. + i)
    if nm == 'bcores':
        prj = bc.DeviceBetaProjector(sampler, S, model)
        prj.pin(Z)
        alg = bc.BetaCoreset(Z, prj, opt_itrs=opt_itrs, step_sched=sched, beta=beta, learn_beta=False, device_optimize=True)
    else:
        prj = bc.DeviceProjector(sampler, S, model)
        prj.pin(Z)
        alg = bc.SparseVICoreset(Z, prj, opt_itrs=opt_itrs, step_sched=sched, device_optimize=True)
    for m in range(5):
        alg.build(1, m + 1)
        np.testing.assert_array_equal(alg.idcs, g['%s_allidcs_%d' % (nm, m)])
        np.testing.assert_allclose(alg.wts, g['%s_allw_%d' % (nm, m)], rtol=1e-5, atol=1e-12)
        got = alg.get()
        np.testing.assert_array_equal(got[2], g['%s_idcs_%d' % (nm, m)])
        np.testing.assert_allclose(got[0], g['%s_wts_%d' % (nm, m)], rtol=1e-5)
        assert np.array_equal(got[1], Z[got[2]])
    assert alg.device_optimize_calls == 5


def _load_example():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples', 'zellner_gaussian.py')
    spec = importlib.util.spec_from_file_location('zellner_gaussian_example_viopt', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize('nm', ['BCORES', 'SVI'])
def test_f14_example_driver_with_the_device_loop(bc, nm):
    g = load_golden('f14_zellner_gaussian_driver')
    N, d, M_, opt_itrs, n_sub_opt, n_sub_sel, proj_dim, tr = [int(v) for v in g['params']]
    res = _load_example().run(nm, tr, N=N, d=d, M=M_, opt_itrs=opt_itrs, n_subsample_opt=n_sub_opt, n_subsample_select=n_sub_sel,
                              proj_dim=proj_dim, verbose=False, device_optimize=True)
    np.testing.assert_array_equal(res['Xc'], g['Xc'])
    for m in range(M_ + 1):
        np.testing.assert_array_equal(res['idcs'][m], g['%s_idcs_%d' % (nm, m)])
        np.testing.assert_allclose(res['w'][m], g['%s_w_%d' % (nm, m)], rtol=1e-5, atol=1e-10)
    np.testing.assert_allclose(res['rkl'], g[nm + '_rkl'], rtol=1e-5)
    np.testing.assert_allclose(res['fkl'], g[nm + '_fkl'], rtol=1e-5)
    assert np.random.rand() == float(g[nm + '_rng_after'])
    assert res['device_optimize_calls'] == M_


# ---------------------------------------------------------------- not covered means unchanged
class _FixedTheta:
    """A sampler that offers device_spec() (so only the OTHER condition under test can decline the run) and returns a fixed Theta."""

    def __init__(self, th):
        self.th = th

    def __call__(self, n, w, p):
        return self.th

    def _dim(self):
        return self.th.shape[1]

    def device_spec(self):
        D = self.th.shape[1]
        return 0, np.concatenate((np.zeros(D), np.eye(D).ravel(), [1.0]))


class _KindOfAnotherModel:
    """A linear-regression sampler whose device_spec() claims the Gaussian kind (which goes with GaussianLocation only)."""

    def __init__(self, inner):
        self.inner = inner

    def __call__(self, n, w, p):
        return self.inner(n, w, p)

    def _dim(self):
        return self.inner._dim()

    def device_spec(self):
        D = self.inner._dim()
        return 1, np.concatenate((np.zeros(D), np.eye(D).ravel(), np.eye(D).ravel()))


@pytest.mark.parametrize('why', ['closure', 'encoder', 'groups', 'D129', 'S257', 'core60001', 'kind'])
def test_not_covered_means_unchanged(bc, why):
    rng = np.random.RandomState(8)
    n, D, S = 3000, (129 if why == 'D129' else 27 if why == 'core60001' else 6), (257 if why == 'S257' else 32)
    Z = linreg_rows(n, D, 50 + D)
    lin = bc.likelihoods.LinearRegression(1.0)
    kw = dict(opt_itrs=4, n_subsample_opt=100)
    enc_layers = [(rng.randn(5, D) * 0.3, rng.randn(5) * 0.1, None, None, True)]
    th5 = rng.randn(S, 5) * 0.2

    def build(device):
        np.random.seed(3)
        if why == 'encoder':
            dd = bc.DeviceData(Z.astype(np.float32), dtype=np.float32)
            prj = bc.DeviceProjector(_FixedTheta(th5), S, lin, encoder=bc.encoders.MLPEncoder(enc_layers))
        else:
            dd = bc.DeviceData(Z)
            if why == 'closure':
                inner = bc.samplers.LinregPosteriorSampler(np.zeros(D), np.eye(D), 1.0)
                sampler = lambda sz, w, p: inner(sz, w, p)
            elif why == 'kind':
                sampler = _KindOfAnotherModel(bc.samplers.LinregPosteriorSampler(np.zeros(D), np.eye(D), 1.0))
            else:
                sampler = bc.samplers.LinregPosteriorSampler(np.zeros(D), np.eye(D), 1.0)
            prj = bc.DeviceProjector(sampler, S, lin)
        if why == 'groups':
            kw2 = dict(kw, groups=[list(range(i * 10, (i + 1) * 10)) for i in range(n // 10)], n_subsample_select=20)
        else:
            kw2 = kw
        alg = bc.SparseVICoreset(dd, prj, device_optimize=device, **kw2)
        if why == 'core60001':      # m (dz + 1) = 2069 * 29 = 60001, one past the staging area: rows put in place, then one _optimize()
            idcs = np.random.RandomState(5).choice(n, 2069, replace=False)
            alg._append(list(idcs), Z[idcs])
            alg.wts = np.random.RandomState(6).rand(2069) * (float(n) / 2069)
            assert alg.pts.shape[0] * (alg.pts.shape[1] + 1) == 60001
            alg._optimize()
        else:
            for m in range(3):
                alg.build(1, 30)
        if device and why in ('closure', 'encoder', 'D129', 'S257', 'core60001', 'kind'):      # asked directly, too: the projector declines
            assert prj.vi_optimize(dd, alg.pts, alg.wts, 4, lambda i: 1. / (1. + i), n_subsample=100, n_total=n) is None
        return alg.idcs.copy(), alg.wts.copy(), np.random.rand(), alg.device_optimize_calls
    off, on = build(False), build(True)
    assert on[3] == 0 and off[3] == 0
    assert off[0].size > 0 and np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1]) and on[2] == off[2]


# ---------------------------------------------------------------- the flag
def test_precision_matrix_that_is_not_positive_definite_raises_and_leaves_the_context_usable(bc):
    rows, dd = resident(bc, ('lin', 9000, 8), lambda: linreg_rows(9000, 8, 18))
    args = ('svi', rows, dd, 64, 20, 5, 200)
    # the sampler of a coreset under construction is fed Sig0inv = -I only for _optimize: with zero weights A = -I exactly
    alg = make_alg(bc, *args, device=True)
    alg.ll_projector.sampler.Sig0inv = -np.eye(8)
    alg.wts = np.zeros_like(alg.wts)
    before = alg.wts.copy()
    held = alg.wts
    with pytest.raises(np.linalg.LinAlgError):
        alg._optimize()
    assert alg.wts is held and np.array_equal(alg.wts, before) and alg.device_optimize_calls == 0
    # the host loop refuses the same matrix the same way
    ref = make_alg(bc, *args, device=False)
    ref.ll_projector.sampler.Sig0inv = -np.eye(8)
    ref.wts = np.zeros_like(ref.wts)
    with pytest.raises(np.linalg.LinAlgError):
        ref._optimize()
    # the next valid run on the same context is right
    compare(host_run(bc, *args), device_run(bc, *args), 'after the flag')


# ---------------------------------------------------------------- the one-call export, and its index check
def _one_call_args(bc, nsub, itrs=7, seed=5, **prior):
    """Everything bc_vi_optimize takes for the problem of the chunk-boundary test, drawn the way vi_optimize draws."""
    from beta_cores_amd.util.opt import adam_step_arrays
    rows, dd = resident(bc, ('lin', 9000, 8), lambda: linreg_rows(9000, 8, 18))
    alg = make_alg(bc, 'svi', rows, dd, 64, 20, seed, nsub, device=True, itrs=itrs, **prior)
    prj, S, D, n = alg.ll_projector, 64, 8, rows.shape[0]
    np.random.seed(seed)
    E = np.empty((itrs, S, D))
    idx = np.empty((itrs, nsub), dtype=np.int64) if nsub else None
    for t in range(itrs):
        E[t] = prj.sampler._normals(S, D)
        if nsub:
            idx[t] = np.random.randint(n, size=nsub)
    kind, sp = prj.sampler.device_spec()
    return dict(alg=alg, dd=dd, core=np.ascontiguousarray(alg.pts, dtype=np.float64), w0=alg.wts.copy(), E=E, idx=idx, kind=kind,
                sp=np.ascontiguousarray(sp), steps=np.ascontiguousarray(adam_step_arrays(itrs, alg.step_sched)),
                params=np.ascontiguousarray(prj.model.params(), dtype=np.float64), model=prj.model.model_id, S=S, n=n, itrs=itrs, nsub=nsub or 0)


def _one_call(bc, a, chunk_steps, out_w, trace=None, idx=None):
    import ctypes
    from beta_cores_amd import _native as N
    p = lambda x: None if x is None else x.ctypes.data_as(ctypes.c_void_p)
    idx = a['idx'] if idx is None else idx
    return N.load().bc_vi_optimize(a['dd'].ctx.h, a['dd'].h, p(a['core']), a['core'].shape[0], int(a['model']), p(a['params']),
                                   int(a['params'].shape[0]), int(a['kind']), p(a['sp']), a['S'], p(a['w0']), a['itrs'], p(a['steps']),
                                   p(a['E']), p(idx), a['nsub'], float(a['n']) / a['nsub'] if a['nsub'] else 1., chunk_steps,
                                   p(out_w), p(trace))


@pytest.mark.parametrize('nsub', [None, 200])
def test_one_call_export_equals_the_chunked_calls(bc, nsub):
    """bc_vi_optimize (its own chunk loop and offsets into normals / sub_idx) against vi_optimize, which drives
    _begin / _chunk_begin / _chunk_end / _end from Python: the same draws, chunk_steps 0 and 3."""
    from beta_cores_amd import _native as N
    want = device_run(bc, 'svi', *resident(bc, ('lin', 9000, 8), lambda: linreg_rows(9000, 8, 18)), 64, 20, 5, nsub, itrs=7)
    a = _one_call_args(bc, nsub)
    for chunk_steps in (0, 3):
        out, trace = np.full(20, -1.), np.full((7, 20), -1.)
        assert _one_call(bc, a, chunk_steps, out, trace) == N.BC_OK, N.last_error()
        assert np.array_equal(out, want[0]) and np.array_equal(trace, want[1])
    out = np.full(20, -1.)
    assert _one_call(bc, a, 2, out) == N.BC_OK and np.array_equal(out, want[0])      # without a trace


@pytest.mark.parametrize('bad', [-1, 9000])
@pytest.mark.parametrize('where', [0, 6 * 200 + 199])
def test_an_index_out_of_range_is_refused_before_anything_runs(bc, bad, where):
    from beta_cores_amd import _native as N
    a = _one_call_args(bc, 200)
    idx = a['idx'].copy()
    idx.ravel()[where] = bad
    out = np.full(20, -1.)
    assert _one_call(bc, a, 3, out, idx=idx) == N.BC_INVALID_ARGUMENT
    msg = N.last_error()
    assert 'bc_vi_optimize' in msg and str(bad) in msg and 'step %d' % (where // 200) in msg
    assert np.all(out == -1.)                                         # out_w left alone
    # the chunked calls refuse it too, at the chunk that holds it, and the run can be closed
    prj = a['alg'].ll_projector
    lib = N.load()
    import ctypes
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    N.call('bc_vi_optimize_begin', prj.ctx.h, a['dd'].h, p(a['core']), 20, int(a['model']), p(a['params']), int(a['params'].shape[0]),
           int(a['kind']), p(a['sp']), a['S'], p(a['w0']), 7, p(a['steps']), 200, a['n'] / 200., 0)
    assert lib.bc_vi_optimize_chunk_begin(prj.ctx.h, p(a['E']), p(idx), 7) == N.BC_INVALID_ARGUMENT
    assert lib.bc_vi_optimize_chunk_end(prj.ctx.h) == N.BC_INVALID_ARGUMENT      # nothing of the chunk was enqueued
    assert lib.bc_vi_optimize_end(prj.ctx.h, None, None) == N.BC_OK
    # the context is still usable: the valid call gives the chunked calls' result
    want = device_run(bc, 'svi', *resident(bc, ('lin', 9000, 8), lambda: linreg_rows(9000, 8, 18)), 64, 20, 5, 200, itrs=7)
    assert _one_call(bc, a, 0, out) == N.BC_OK and np.array_equal(out, want[0])


def test_zero_steps_take_the_host_loop(bc):
    """nn_opt with opt_itrs = 0 returns w0; the device entry points refuse a run of no steps, so vi_optimize declines it."""
    rows, dd = resident(bc, ('lin', 9000, 8), lambda: linreg_rows(9000, 8, 18))
    alg = make_alg(bc, 'svi', rows, dd, 64, 20, 5, 200, device=True, itrs=0)
    w0 = alg.wts.copy()
    alg._optimize()
    assert alg.device_optimize_calls == 0 and np.array_equal(alg.wts, w0)


# ---------------------------------------------------------------- the draw itself, read back from the run's slab
# One-step runs of vi_optimize, then vi_last_draw(): what k_vi_sampler left for K1 from (coreset rows, w0, E[0]) against the
# formulas in long double (vi_sampler_cases.reference_ld), under the bound of tests/test_vi_sampler_cpu.py.  The data rows do not
# enter the draw, so they are 3000 resident rows per (kind, D).  Ratios seen are recorded in profiles/vi_optimize_notes.md.
DRAW_DIMS = (1, 2, 3, 16, 33, 64, 127, 128)
DRAW_SHAPES = ((1, 1), (7, 5), (130, 100), (300, 256))      # (m, S); m (dz + 1) <= 39 000


def draw_data(bc, kind, D):
    if kind == vc.GAUSS:
        return resident(bc, ('gauss', 3000, D), lambda: gauss_rows(3000, D, 4))[1]
    return resident(bc, ('lin', 3000, D), lambda: linreg_rows(3000, D, 10 + D))[1]


def draw_projector(bc, c):
    """A projector whose sampler holds case c's prior and hands out c['E'] as its next normals."""
    if c['kind'] == vc.GAUSS:
        sampler = bc.samplers.GaussianPosteriorSampler(c['th0'], c['Sig0inv'], c['Siginv'], rng=np.random.RandomState(0))
        model = bc.likelihoods.GaussianLocation(c['Siginv'], -np.linalg.slogdet(c['Siginv'])[1])
    else:
        sampler = bc.samplers.LinregPosteriorSampler(c['th0'], c['Sig0inv'], c['sigsq'], rng=np.random.RandomState(0))
        model = bc.likelihoods.LinearRegression(c['sigsq'])
    prj = bc.DeviceProjector(sampler, c['s'], model)
    prj.sampler._rng = _FixedNormals(c['E'])
    return prj


def one_step_draw(bc, c, dd):
    prj = draw_projector(bc, c)
    assert prj.vi_optimize(dd, c['rows'], c['w'], 1, lambda i: 1.) is not None and prj.vi_optimize_calls == 1
    return prj.vi_last_draw()


def check_draw(c, draw, tag):
    """The assertions on one draw; returns error / bound."""
    d = c['d']
    ref, kappa = vc.high_precision_reference(c)
    bound = vc.draw_bound(d, kappa, ref)
    got = draw['theta'] if c['kind'] == vc.LINREG else draw['raw']
    err = np.abs(got - ref).max()
    print('%s: max error %.3e, bound %.3e, ratio %.3f, kappa %.3e' % (tag, err, bound, err / bound, kappa))
    assert err <= bound, (tag, err, bound)
    assert draw['pad_max'] == 0.0, (tag, draw['pad_max'])
    if c['kind'] == vc.GAUSS:
        Si, raw = c['Siginv'], draw['raw']
        scale = np.abs(Si).sum(axis=1).max() * np.abs(raw).max()
        assert np.abs(draw['theta'] - raw.dot(Si.T)).max() <= 4. * d * 2. ** -53 * scale
        assert np.abs(draw['saux'] - (raw * raw.dot(Si)).sum(axis=1)).max() <= 4. * d * 2. ** -53 * scale * d * np.abs(raw).max()
    else:
        assert not draw['saux'].any() and not draw['raw'].any()      # the linear-regression kind never touches them
    return err / bound


def same_bits(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ('theta', 'saux', 'raw')) and a['pad_max'] == b['pad_max']


@pytest.mark.parametrize('prior', ['identity', 'general'])
@pytest.mark.parametrize('D', DRAW_DIMS)
@pytest.mark.parametrize('kind', [vc.LINREG, vc.GAUSS], ids=['linreg', 'gauss'])
def test_device_draw_matches_the_long_double_reference(bc, kind, D, prior):
    dd = draw_data(bc, kind, D)
    worst = 0.
    for i, (m, S) in enumerate(DRAW_SHAPES):
        c = vc.make_case(kind, D, m, S) if prior == 'identity' else vc.make_general_case(kind, D, m, S, variant=i + D)
        draw = one_step_draw(bc, c, dd)
        worst = max(worst, check_draw(c, draw, 'kind %d D %3d m %3d S %3d %s prior' % (kind, D, m, S, prior)))
        assert same_bits(one_step_draw(bc, c, dd), draw), 'a second identical run gave other bits'
    print('worst ratio on the device, kind %d, D = %d, %s prior: %.3f' % (kind, D, prior, worst))


@pytest.mark.parametrize('kind', ['svi', 'gauss'])
def test_last_draw_of_a_multi_step_run_is_drawn_from_the_weights_adam_just_wrote(bc, kind):
    D, S, m, itrs = 16, 64, 20, 4
    k = vc.GAUSS if kind == 'gauss' else vc.LINREG
    rows, dd = resident(bc, ('gauss', 3000, D), lambda: gauss_rows(3000, D, 4)) if kind == 'gauss' else \
        resident(bc, ('lin', 3000, D), lambda: linreg_rows(3000, D, 10 + D))
    p = vc.make_general_case(k, D, 1, 1)
    prior = dict(mu0=p['th0'], Sig0inv=p['Sig0inv']) if kind == 'gauss' else dict(th0=p['th0'], Sig0inv=p['Sig0inv'], sigsq=2.5)
    alg = make_alg(bc, kind, rows, dd, S, m, 21, 200, device=True, itrs=itrs, **prior)
    prj, E = alg.ll_projector, []
    normals = prj.sampler._normals
    prj.sampler._normals = lambda n, d: E.append(normals(n, d)) or E[-1]
    np.random.seed(21)
    w, trace = prj.vi_optimize(dd, alg.pts, alg.wts, itrs, alg.step_sched, n_subsample=200, n_total=rows.shape[0], want_trace=True)
    assert len(E) == itrs and np.array_equal(trace[-1], w)
    draw = prj.vi_last_draw()
    c = {'kind': k, 'd': D, 'm': m, 's': S, 'rows': alg.pts, 'th0': p['th0'], 'Sig0inv': p['Sig0inv'], 'E': E[3], 'w': trace[2]}
    if kind == 'gauss':
        c['Siginv'] = prj.sampler.Siginv
    else:
        c['sigsq'] = 2.5
    check_draw(c, draw, '%s, the fourth step of four' % kind)
    # ... and from no other weights: the same normals with the weights of one step earlier are far outside the bound
    ref, kappa = vc.high_precision_reference(c)
    stale = vc.high_precision_reference(dict(c, w=trace[1]))[0]
    assert np.abs(stale - ref).max() > 1e3 * vc.draw_bound(D, kappa, ref)


@pytest.mark.parametrize('prior', ['identity', 'general'])
@pytest.mark.parametrize('kind', [vc.LINREG, vc.GAUSS], ids=['linreg', 'gauss'])
def test_all_zero_weights_draw_from_the_prior(bc, kind, prior):
    """G = 0: Theta = (L L^T) Sig0inv th0 + E . L^T with L = chol(Sig0inv)^-1; with Sig0inv = I that is th0 + E, exactly."""
    for D, m, S in ((3, 7, 5), (33, 130, 100)):
        c = vc.make_case(kind, D, m, S) if prior == 'identity' else vc.make_general_case(kind, D, m, S, variant=1)
        c['w'] = np.zeros(m)
        draw = one_step_draw(bc, c, draw_data(bc, kind, D))
        check_draw(c, draw, 'kind %d D %d, zero weights, %s prior' % (kind, D, prior))
        if prior == 'identity':
            assert np.array_equal(draw['theta'] if kind == vc.LINREG else draw['raw'], c['th0'] + c['E'])


@pytest.mark.parametrize('what', ['not positive definite', 'NaN weight'])
@pytest.mark.parametrize('kind', [vc.LINREG, vc.GAUSS], ids=['linreg', 'gauss'])
def test_a_failed_first_step_leaves_the_draw_at_zero(bc, kind, what):
    D, m, S = 16, 7, 5
    dd = draw_data(bc, kind, D)
    good = vc.make_general_case(kind, D, m, S)
    first = one_step_draw(bc, good, dd)
    assert np.abs(first['theta']).min() > 0.      # the slab of this shape held a draw just before
    if what == 'NaN weight':
        bad = vc.make_general_case(kind, D, m, S)
        bad['w'][3] = np.nan
    else:
        bad = vc.make_case(kind, D, m, S, sig0_sign=-1.)
        bad['w'] = bad['w'] * (0. if kind == vc.LINREG else 1e-3)
    prj = draw_projector(bc, good)      # (the projector's constructor draws on the host: it takes the valid prior)
    prj.sampler.Sig0inv, prj.sampler._rng = bad['Sig0inv'], _FixedNormals(bad['E'])
    with pytest.raises(np.linalg.LinAlgError):
        prj.vi_optimize(dd, bad['rows'], bad['w'], 1, lambda i: 1.)
    assert prj.vi_optimize_calls == 0
    draw = prj.vi_last_draw()
    assert not draw['theta'].any() and not draw['saux'].any() and not draw['raw'].any() and draw['pad_max'] == 0.0
    assert same_bits(one_step_draw(bc, good, dd), first)      # the next valid run is right


def test_last_draw_is_refused_before_any_run_and_for_another_shape(bc):
    import ctypes
    from beta_cores_amd import _native as N
    lib, out, pad = N.load(), np.full(4, -1.), ctypes.c_double(-1.)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    fresh = bc.Context()
    assert lib.bc_vi_optimize_last_draw(fresh.h, 2, 2, p(out), None, None, ctypes.byref(pad)) == N.BC_INVALID_ARGUMENT
    assert 'no run has been begun' in N.last_error()
    c = vc.make_case(vc.LINREG, 3, 7, 5)
    prj = draw_projector(bc, c)
    prj.vi_optimize(draw_data(bc, vc.LINREG, 3), c['rows'], c['w'], 1, lambda i: 1.)
    assert lib.bc_vi_optimize_last_draw(prj.ctx.h, 2, 2, p(out), None, None, ctypes.byref(pad)) == N.BC_INVALID_ARGUMENT
    assert 'S = 5, D = 3' in N.last_error() and np.all(out == -1.) and pad.value == -1.
    th = np.empty((5, 3))      # saux and raw may be left out
    assert lib.bc_vi_optimize_last_draw(prj.ctx.h, 5, 3, p(th), None, None, ctypes.byref(pad)) == N.BC_OK
    assert np.array_equal(th, prj.vi_last_draw()['theta']) and pad.value == 0.0


# ---------------------------------------------------------------- the loop with general priors
def general_prior(kind, D, sigsq=0.37):
    p = vc.make_general_case(vc.GAUSS if kind == 'gauss' else vc.LINREG, D, 1, 1)
    if kind == 'gauss':
        return dict(mu0=p['th0'], Sig0inv=p['Sig0inv'])
    return dict(th0=p['th0'], Sig0inv=p['Sig0inv'], sigsq=sigsq)


@pytest.mark.parametrize('nsub', [None, 50])
@pytest.mark.parametrize('shape', [(3000, 3, 16, 7), (5000, 64, 100, 100)], ids=lambda s: 'n%d-D%d-S%d-m%d' % s)
@pytest.mark.parametrize('kind', ['svi', 'bcores'])
def test_general_prior_device_loop_equals_the_host_loop(bc, kind, shape, nsub):
    n, D, S, m = shape
    rows, dd = resident(bc, ('lin', n, D), lambda: linreg_rows(n, D, 10 + D))
    args = (kind, rows, dd, S, m, 100 + D, nsub)
    prior = general_prior(kind, D, sigsq=0.37 if nsub else 2.5)
    compare(host_run(bc, *args, **prior), device_run(bc, *args, **prior), 'general prior %s n=%d D=%d S=%d m=%d nsub=%s' % (kind, n, D, S, m, nsub))


@pytest.mark.parametrize('S', [64, 256])
@pytest.mark.parametrize('d', [1, 33, 128])
def test_general_prior_gaussian_location(bc, d, S):
    rows, dd = resident(bc, ('gauss', 3000, d), lambda: gauss_rows(3000, d, 4))
    args = ('gauss', rows, dd, S, 30, 11, 300)
    prior = general_prior('gauss', d)
    compare(host_run(bc, *args, **prior), device_run(bc, *args, **prior), 'general prior gaussian d=%d S=%d' % (d, S))


def test_general_prior_one_call_export(bc):
    from beta_cores_amd import _native as N
    prior = general_prior('svi', 8, sigsq=2.5)
    args = ('svi',) + resident(bc, ('lin', 9000, 8), lambda: linreg_rows(9000, 8, 18)) + (64, 20, 5, 200)
    want = device_run(bc, *args, itrs=7, **prior)
    compare(host_run(bc, *args, itrs=7, **prior), want, 'general prior, the chunked calls')
    a = _one_call_args(bc, 200, **prior)
    out, trace = np.full(20, -1.), np.full((7, 20), -1.)
    assert _one_call(bc, a, 3, out, trace) == N.BC_OK, N.last_error()
    assert np.array_equal(out, want[0]) and np.array_equal(trace, want[1])


def test_upper_triangle_of_the_prior_precision_is_read_by_its_product_with_th0_only(bc):
    """Host and device factor the LOWER triangle of Sig0inv + G / sigsq and take Sig0inv . th0 with the full matrix."""
    rows, dd = resident(bc, ('lin', 9000, 8), lambda: linreg_rows(9000, 8, 18))
    args = ('svi', rows, dd, 64, 20, 5, 200)
    prior = general_prior('svi', 8, sigsq=2.5)
    prior['Sig0inv'] = prior['Sig0inv'] + np.triu(np.random.RandomState(3).randn(8, 8) * 0.05, 1)
    host = host_run(bc, *args, **prior)
    compare(host, device_run(bc, *args, **prior), 'asymmetric Sig0inv')
    sym = dict(prior, Sig0inv=np.tril(prior['Sig0inv']) + np.tril(prior['Sig0inv'], -1).T)
    assert not np.allclose(host_run(bc, *args, **sym)[1], host[1], rtol=1e-3, atol=0.)      # (the perturbation is not lost in rounding)


# ---------------------------------------------------------------- the largest coresets the staging area takes
@pytest.mark.parametrize('shape', [(3000, 128, 64, 461), (20000, 1, 16, 20000)], ids=lambda s: 'n%d-D%d-S%d-m%d' % s)
def test_largest_accepted_coreset_runs_on_the_device(bc, shape):
    n, D, S, m = shape
    assert m * (D + 2) <= 60000 < (m + 1) * (D + 2)
    rows, dd = resident(bc, ('lin', n, D), lambda: linreg_rows(n, D, 10 + D))
    args = ('svi', rows, dd, S, m, 100 + D, 50)
    compare(host_run(bc, *args), device_run(bc, *args), 'largest coreset D=%d m=%d' % (D, m))
