"""The Gaussian-location kind of the batched BatchPSVI run on the device (include/beta_cores_psvi_many.h;
BatchPSVICoreset.build_many): every stage of the last step on the device's own inputs through the seam, against
tests/psvi_many_gauss_cases.py's long-double restatement and derived bounds, tests/vi_sampler_cases.py and tests/psvi_cases.py;
batch independence, repeatability, float32 rows; the batched route against the loop of single builds with a long-double whole run
as the reference; marking, the guards, the position of the random streams, and examples/zellner_gaussian.py with batched=True."""
import importlib.util
import os
import re

import numpy as np
import pytest

import psvi_many_gauss_cases as pg

pytestmark = pytest.mark.gpu
N_ROWS = 600
SIZES = [1, 2, 5, 17, 40]
GAUSS = 1          # BC_VI_SAMPLER_GAUSS


@pytest.fixture(scope='module')
def bc():
    import beta_cores_amd as bc
    bc.default_context()
    return bc


_rows_cache = {}


def rows_of(bc, d, f32=False):
    """(host rows as float64 values, their DeviceData): N_ROWS rows of width d, once per module; f32: float32 storage"""
    if (d, f32) not in _rows_cache:
        x = pg.make_rows(np.random.RandomState(4300 + d), N_ROWS, d)      # (values a float32 holds: both storages carry the same rows)
        dd = bc.DeviceData(x.astype(np.float32), dtype=np.float32) if f32 else bc.DeviceData(x)
        _rows_cache[d, f32] = (x, dd)
    return _rows_cache[d, f32]


def _how(bc, mdl):
    model = bc.likelihoods.GaussianLocation(mdl['Siginv'], mdl['logdet'])
    return dict(model_id=model.model_id, sampler_kind=GAUSS, model_params=model.params(),
                sampler_params=np.concatenate((mdl['mu0'], mdl['Sig0inv'].ravel(), mdl['Siginv'].ravel())))


class Run:
    """One native run on SIZES-like problems: nested initial points, weights N / m, draws of a seeded stream.  Chunks of
    opt_itrs - 1 steps and 1 step, so that the seam is read before and after the last step."""

    def __init__(self, bc, d, s, n_sub, itrs, sizes=SIZES, f32=False, w0=None, chunk=None):
        from beta_cores_amd.coreset import bpsvi
        x, dd = rows_of(bc, d, f32)
        perm = np.random.RandomState(9).permutation(N_ROWS)
        rng = np.random.RandomState(1000 + d + s)
        self.mdl = pg.make_model(d)
        self.E, self.idx = rng.randn(itrs, s, d), rng.randint(N_ROWS, size=(itrs, n_sub))
        self.x, self.d, self.s, self.n_sub, self.itrs, self.sizes = x, d, s, n_sub, itrs, list(sizes)
        self.pts0 = [x[perm[:m]] for m in sizes]
        self.w0 = [np.full(m, N_ROWS / m) for m in sizes] if w0 is None else w0
        self.steps = np.array([[1. / (1. + i) for i in range(itrs)] for _ in sizes]).reshape(len(sizes), itrs)
        self.seams, at = [], [0]

        def draw(k):
            out = self.E[at[0]:at[0] + k], self.idx[at[0]:at[0] + k]
            at[0] += k
            return out
        self.res = bpsvi.psvi_many_run(dd, self.pts0, self.w0, s, itrs, self.steps, draw, n_sub, n_total=N_ROWS,
                                       chunk_steps=chunk or max(itrs - 1, 1),
                                       on_chunk=lambda done: self.seams.append((done, bpsvi.psvi_many_last_step(dd.ctx, self.sizes, d, s))),
                                       **_how(bc, self.mdl))
        assert at[0] == itrs                                   # nothing was drawn past the last step
        self.last = self.seams[-1][1]

    def same_bits(self, other, mine=None, theirs=None):
        mine = range(len(self.sizes)) if mine is None else mine
        theirs = range(len(other.sizes)) if theirs is None else theirs
        return all(np.array_equal(self.res['w'][a], other.res['w'][b]) and np.array_equal(self.res['pts'][a], other.res['pts'][b])
                   and np.array_equal(self.res['modes'][a], other.res['modes'][b]) for a, b in zip(mine, theirs))


# ---------------------------------------------------------------- 1. each stage of the last step, on the device's own inputs
@pytest.mark.parametrize('d,s,n_sub,itrs', [(3, 7, 37, 1), (16, 100, 64, 2), (33, 200, 200, 4), (100, 200, 200, 2), (128, 100, 37, 2)])
def test_stages_of_the_last_step(bc, d, s, n_sub, itrs):
    _check_last_step(Run(bc, d, s, n_sub, itrs), d, s, n_sub, itrs)


@pytest.mark.parametrize('d,s,n_sub,itrs', [(16, 100, 64, 2), (100, 200, 200, 2)])
def test_stages_with_the_samplers_own_products(bc, monkeypatch, d, s, n_sub, itrs):
    """BC_PSVI_POST=chains (read at every begin): the posterior stage's three products by bc_vi_sampler's own per-thread chains,
    the form the matrix-core one was measured against -- the same bounds."""
    monkeypatch.setenv('BC_PSVI_POST', 'chains')
    _check_last_step(Run(bc, d, s, n_sub, itrs), d, s, n_sub, itrs)


def _check_last_step(r, d, s, n_sub, itrs):
    assert r.res['marked'] == [] and [done for done, _ in r.seams] == ([itrs] if itrs == 1 else [itrs - 1, itrs])
    L, ptr = r.last, r.last['row_ptr']
    before = r.seams[-2][1] if itrs > 1 else None              # its state AFTER step itrs - 2: the moments before the last step
    rows, i = r.x[r.idx[itrs - 1]], itrs - 1
    for p, m in enumerate(r.sizes):
        sl = slice(ptr[p], ptr[p + 1])
        label = 'D %d S %d n_sub %d steps %d m %d' % (d, s, n_sub, itrs, m)
        wb, pb = L['w_before'][sl], L['pts_before'][sl]
        if before is None:
            assert np.array_equal(wb, r.w0[p]) and np.array_equal(pb, r.pts0[p])
        else:
            assert np.array_equal(wb, before['w'][sl]) and np.array_equal(pb, before['pts'][sl])
        pg.check_mean_and_draw(label, pb, wb, r.E[i], r.mdl, L['mode'][p], L['theta'][p])
        pg.check_stage34(label, rows, N_ROWS / n_sub, pb, wb, L['theta'][p], r.mdl, L['target'][p], L['resid'][p], L['gw'][sl])
        pg.check_point_grad(label, pb, wb, L['theta'][p], L['resid'][p], r.mdl, L['gp'][sl])
        x0, g = np.concatenate((wb, pb.ravel())), np.concatenate((L['gw'][sl], L['gp'][sl].ravel()))
        m1 = np.zeros_like(x0) if before is None else np.concatenate((before['mom1_w'][sl], before['mom1_p'][sl].ravel()))
        m2 = np.zeros_like(x0) if before is None else np.concatenate((before['mom2_w'][sl], before['mom2_p'][sl].ravel()))
        pg.check_adam(label, x0, g, m1, m2, r.steps[p, i], i, m, np.concatenate((L['w'][sl], L['pts'][sl].ravel())),
                      np.concatenate((L['mom1_w'][sl], L['mom1_p'][sl].ravel())), np.concatenate((L['mom2_w'][sl], L['mom2_p'][sl].ravel())))
        assert np.array_equal(r.res['w'][p], L['w'][sl]) and np.array_equal(r.res['pts'][p], L['pts'][sl]) and \
            np.array_equal(r.res['modes'][p], L['mode'][p])    # what _end hands out is the state the seam shows
    assert not L['newton'].any() and not L['flag'].any()


# ---------------------------------------------------------------- 2. batch independence and repeatability, 3. float32 rows
@pytest.mark.parametrize('d,s,n_sub', [(33, 100, 37), (16, 7, 200)])
def test_bits_do_not_depend_on_the_batch(bc, d, s, n_sub):
    whole = Run(bc, d, s, n_sub, 3)
    assert Run(bc, d, s, n_sub, 3).same_bits(whole)                             # a repeated run: the same bits
    assert Run(bc, d, s, n_sub, 3, chunk=1).same_bits(whole)                    # however the steps are chunked
    for p, m in enumerate(SIZES):
        assert Run(bc, d, s, n_sub, 3, sizes=[m]).same_bits(whole, [0], [p]), m
    order = [3, 0, 4, 2, 1]
    assert Run(bc, d, s, n_sub, 3, sizes=[SIZES[j] for j in order]).same_bits(whole, range(5), order)


def test_float32_rows_give_the_bits_of_their_widened_copy(bc):
    assert Run(bc, 33, 100, 37, 3, f32=True).same_bits(Run(bc, 33, 100, 37, 3))
    assert Run(bc, 3, 7, 200, 2, f32=True).same_bits(Run(bc, 3, 7, 200, 2))      # (rows of 12 bytes: the narrow gather)


# ---------------------------------------------------------------- 4. against the existing single-size path
def _coreset(bc, d, s, n_sub, fused, seed, own_rng=True, itrs=6, **kw):
    _, dd = rows_of(bc, d)
    mdl = pg.make_model(d)
    smp = bc.samplers.GaussianPosteriorSampler(mdl['mu0'], mdl['Sig0inv'], mdl['Siginv'], rng=np.random.RandomState(seed) if own_rng else None)
    prj = bc.DeviceProjector(smp, s, bc.likelihoods.GaussianLocation(mdl['Siginv'], mdl['logdet']))
    return bc.BatchPSVICoreset(dd, prj, opt_itrs=itrs, n_subsample_opt=n_sub, fused_gradient=fused, **kw)


def _stream(state):
    r = np.random.RandomState()
    r.set_state(state)
    return r


def _long_double_curve(data, mdl, sizes, S, n_sub, itrs, glob, normals, sched):
    """The curve in long double on the draws a build makes from these stream states: the permutation, then per step the S x D
    normals and the row numbers.  Returns (entries as build_many gives them, the smallest |weight| met after any step)."""
    n, d = data.shape
    perm = glob.choice(n, size=max(sizes), replace=False)
    E, idx = np.empty((itrs, S, d)), np.empty((itrs, n_sub), dtype=np.int64)
    for i in range(itrs):
        E[i] = normals.randn(S, d)
        idx[i] = glob.randint(n, size=n_sub)
    entries, closest = [], np.inf
    for m in sizes:
        w, p, near = pg.whole_run_ld(data, data[perm[:m]], np.full(m, n / m), mdl, E, idx, [sched(i) for i in range(itrs)], float(n))
        keep = w > 0
        entries.append((w[keep], p[keep], perm[:m][keep]))
        closest = min(closest, near)
    return entries, closest


def _deviation(a, b):
    """the largest |a - b| / (1 + |b|) over the weights and points of two curves; the same rows must have survived"""
    worst = 0.
    for (wa, pa, ia), (wb, pb, ib) in zip(a, b):
        assert np.array_equal(ia, ib)
        worst = max(worst, float((np.abs(wa - wb) / (1. + np.abs(wb))).max()), float((np.abs(pa - pb) / (1. + np.abs(pb))).max()))
    return worst


@pytest.mark.parametrize('d,s,n_sub', [(16, 100, 64), (33, 7, 37)])
def test_batched_route_against_the_loop_of_single_builds(bc, d, s, n_sub):
    """The reference is the long-double whole run of tests/psvi_many_gauss_cases.py on the same draws (6 steps, sizes 1, 2, 5, 17,
    40, weights N / m).  The yardstick is the larger deviation of the two single-size routes the library already had
    (fused_gradient True and False) from it; the batched route's deviation from it may be 8 times that, the constant
    tests/test_gpu_psvi_many.py uses: the batched route replaces LAPACK's factorisation and BLAS's products by its own chains and
    tile order, which changes constants, while an indexing error shows at 1e-3.  deviation = max |a - b| / (1 + |b|) over weights
    and points.  The seeds are such that no weight of the long-double run comes within 1e-6 of zero (checked below; the closest
    are 14 and 13.4: weights start at N / m >= 15 and an ADAM step moves them by about its step size), so the same points survive
    on every route.

    Measured on one MI355X, deviations from the long-double run:
      D 16, S 100, n_sub 64:  fused 5.930e-12 (the yardstick), unfused 4.415e-12, batched 4.697e-12, allowed 4.744e-11;
      D 33, S 7,   n_sub 37:  fused 7.265e-12, unfused 7.935e-12 (the yardstick), batched 2.240e-12, allowed 6.348e-11
    (with BC_PSVI_POST=chains the batched figures were 1.178e-11 and 6.424e-12)."""
    x, _ = rows_of(bc, d)
    curves, ref = {}, None
    for name, fused, route in (('fused', True, 'each'), ('unfused', False, 'each'), ('batched', True, 'batched'), ('auto', True, 'auto')):
        alg = _coreset(bc, d, s, n_sub, fused, seed=5)
        np.random.seed(6)
        if ref is None:
            ref, closest = _long_double_curve(x, pg.make_model(d), SIZES, s, n_sub, 6, _stream(np.random.get_state()),
                                              _stream(alg.ll_projector.sampler._rng.get_state()), lambda i: 1. / (1. + i))
        curves[name] = alg.build_many(SIZES, route=route)
        assert alg.wts.size == 0 and alg.pts.size == 0 and alg.idcs.size == 0      # the object's own state is left alone
    assert closest > 1e-6
    assert curves['batched'].route == 'batched' == curves['auto'].route and curves['fused'].route == 'each'
    assert curves['batched'].marked == [] and curves['batched'].device_ms > 0.
    assert all(np.array_equal(x_, y_) for a, b in zip(curves['batched'], curves['auto']) for x_, y_ in zip(a, b))
    for a, b in zip(curves['batched'], curves['fused']):
        assert np.array_equal(a[2], b[2])                      # the surviving row numbers
    dev = {k: _deviation(curves[k], ref) for k in ('fused', 'unfused', 'batched')}
    yard = max(dev['fused'], dev['unfused'])
    print('D %d S %d n_sub %d: from the long-double run: fused %.3e, unfused %.3e, batched %.3e, allowed %.3e; closest weight to zero %.3g'
          % (d, s, n_sub, dev['fused'], dev['unfused'], dev['batched'], 8. * yard, closest))
    assert dev['fused'] <= 1e-9 and dev['unfused'] <= 1e-9
    assert dev['batched'] <= 8. * yard


@pytest.mark.parametrize('own_rng', [True, False])
def test_streams_stand_where_one_build_leaves_them(bc, own_rng):
    ends = []
    for route in ('batched', 'each'):
        alg = _coreset(bc, 16, 7, 37, True, seed=3, own_rng=own_rng)
        np.random.seed(8)
        assert alg.build_many([1, 5, 17], route=route).route == route
        rng = alg.ll_projector.sampler._rng
        ends.append((np.random.rand(3), rng.rand(3) if own_rng else None))
    assert np.array_equal(ends[0][0], ends[1][0]) and (not own_rng or np.array_equal(ends[0][1], ends[1][1]))
    alg = _coreset(bc, 16, 7, 37, True, seed=3, own_rng=own_rng)
    np.random.seed(8)
    alg.build(1, 5)
    rng = alg.ll_projector.sampler._rng
    assert np.array_equal(np.random.rand(3), ends[0][0]) and (not own_rng or np.array_equal(rng.rand(3), ends[0][1]))


# ---------------------------------------------------------------- 5. marking
def test_a_nan_weight_marks_its_problem_alone(bc):
    w0 = [np.full(m, N_ROWS / m) for m in SIZES]
    w0[2][3] = np.nan
    bad = Run(bc, 16, 100, 64, 3, w0=w0)
    assert bad.res['marked'] == [2] and list(bad.res['status']) == [0, 0, 1, 0, 0] and bad.res['w'][2] is None and bad.res['pts'][2] is None
    assert np.all(np.isnan(bad.res['modes'][2]))               # (the wrapper's fill: nothing was copied for it)
    assert bad.last['flag'][2] == 1 and not bad.last['flag'][[0, 1, 3, 4]].any()
    rest = Run(bc, 16, 100, 64, 3, sizes=[1, 2, 17, 40])
    assert bad.same_bits(rest, [0, 1, 3, 4], [0, 1, 2, 3])     # the others' bits: those of a batch without it


# ---------------------------------------------------------------- 6. guards
def test_uncovered_configurations_and_refused_arguments(bc):
    from beta_cores_amd.coreset import bpsvi
    x, dd = rows_of(bc, 16)
    mdl = pg.make_model(16)
    model = bc.likelihoods.GaussianLocation(mdl['Siginv'], mdl['logdet'])
    other = bc.samplers.GaussianPosteriorSampler(mdl['mu0'], mdl['Sig0inv'], mdl['Siginv'] * (1. + 2. ** -50), rng=np.random.RandomState(0))
    with pytest.raises(NotImplementedError, match="Siginv is not the model's"):
        bc.BatchPSVICoreset(dd, bc.DeviceProjector(other, 7, model), opt_itrs=2, n_subsample_opt=37).build_many([1, 2], route='batched')
    th = np.random.RandomState(2).randn(7, 16)
    closure = bc.DeviceProjector(lambda n, w, p: th, 7, model)
    with pytest.raises(NotImplementedError, match='GaussianPosteriorSampler'):
        bc.BatchPSVICoreset(dd, closure, opt_itrs=2, n_subsample_opt=37).build_many([1, 2], route='batched')
    every_row = _coreset(bc, 16, 7, None, True, 1, itrs=2, pin_data=False)
    with pytest.raises(NotImplementedError, match='n_subsample_opt'):
        every_row.build_many([1, 2], route='batched')
    assert every_row.build_many([1, 2]).route == 'each'        # 'auto' takes the loop
    alg = _coreset(bc, 16, 7, 37, True, 1)
    alg.ll_projector.encoder = object()
    with pytest.raises(NotImplementedError, match='encoder'):
        alg.build_many([1, 2], route='batched')
    alg.ll_projector.encoder = None
    alg.opt_itrs = 0
    with pytest.raises(NotImplementedError, match='opt_itrs'):
        alg.build_many([1, 2], route='batched')
    # refused by the native call, before a draw is made
    no_draw = lambda k: pytest.fail('a refused run drew random numbers')
    how = _how(bc, mdl)
    args = ([np.zeros((1, 16))], [np.ones(1)], 7, 2, np.ones((1, 2)), no_draw, 5)
    with pytest.raises(ValueError, match='diag must be 0'):
        bpsvi.psvi_many_run(dd, *args, diag=True, **how)
    with pytest.raises(ValueError, match='start must be NULL'):
        bpsvi.psvi_many_run(dd, *args, start=np.zeros((1, 16)), **how)
    with pytest.raises(ValueError, match="not the model's"):
        bpsvi.psvi_many_run(dd, *args, **dict(how, sampler_params=np.concatenate((mdl['mu0'], mdl['Sig0inv'].ravel(), 2. * mdl['Siginv'].ravel()))))
    with pytest.raises(ValueError, match='model parameters'):
        bpsvi.psvi_many_run(dd, *args, **dict(how, model_params=how['model_params'][:-1]))
    wide, m129 = bc.DeviceData(np.random.RandomState(0).randn(40, 129)), pg.make_model(129)
    with pytest.raises(ValueError, match='D = 129'):
        bpsvi.psvi_many_run(wide, [np.zeros((1, 129))], [np.ones(1)], 7, 2, np.ones((1, 2)), no_draw, 5, **_how(bc, m129))
    lin = bc.likelihoods.LinearRegression(1.)
    with pytest.raises(ValueError, match='linear-regression'):
        bpsvi.psvi_many_run(dd, *args, **dict(how, model_id=lin.model_id, sampler_kind=0))
    # the work space the run lays out is what bc_psvi_curve_work_doubles says: a run over the limit names its count
    lib = bc._native.load()
    with pytest.raises(ValueError, match='work space') as e:
        bpsvi.psvi_many_run(dd, [np.zeros((1, 16))] * 64, [np.ones(1)] * 64, 256, 2, np.ones((64, 2)), no_draw, bpsvi.PSVI_MANY_MAX_SUB, **how)
    need = int(re.search(r'needs (\d+) doubles', str(e.value)).group(1))
    assert need == lib.bc_psvi_curve_work_doubles(64, 64, 16, 256, bpsvi.PSVI_MANY_MAX_SUB, 2, GAUSS) > bpsvi.PSVI_MANY_MAX_WORK_DOUBLES
    logistic = lib.bc_psvi_many_work_doubles(64, 64, 16, 256, bpsvi.PSVI_MANY_MAX_SUB, 2)
    extra = 64 * (256 * 16 + 256) + bpsvi.PSVI_MANY_MAX_SUB + 64
    assert logistic + extra <= need <= logistic + extra + 4    # (four more pieces, each rounded up to an even count)
    assert _coreset(bc, 16, 7, 37, True, 1).build_many([1, 2]).route == 'batched'      # and the context is free again


# ---------------------------------------------------------------- 7. the example
def test_the_example_builds_its_curve_in_one_batched_run(bc):
    """examples/zellner_gaussian.py, BPSVI, batched=True against the loop, both against the long-double whole run on the same draws
    (the global stream stands at the fork state after run(), so the draws can be restated), measured as in
    test_batched_route_against_the_loop_of_single_builds; the loop's deviation is the yardstick.
    Measured on one MI355X: loop 1.129e-12, batched 2.982e-13, allowed 9.033e-12; the closest weight to zero 56.8."""
    spec = importlib.util.spec_from_file_location('zellner_gaussian', os.path.join(pg.ROOT, 'examples', 'zellner_gaussian.py'))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    kw = dict(N=300, d=5, M=6, opt_itrs=5, n_subsample_opt=37, proj_dim=7, verbose=False)
    loop = ex.run('BPSVI', 1, batched=False, **kw)
    end_loop = np.random.get_state()
    many = ex.run('BPSVI', 1, batched=True, **kw)
    end_many = np.random.get_state()
    assert many['route'] == 'batched' and loop['route'] == 'each'
    assert end_loop[0] == end_many[0] and np.array_equal(end_loop[1], end_many[1]) and tuple(end_loop[2:]) == tuple(end_many[2:])
    Sig = 500 * np.eye(5)
    mdl = {'d': 5, 'Siginv': np.linalg.inv(Sig), 'Sig0inv': np.linalg.inv(np.eye(5)), 'mu0': np.zeros(5), 'logdet': np.linalg.slogdet(Sig)[1]}
    glob = _stream(end_many)                                   # one stream: the normals and the row numbers
    ref, closest = _long_double_curve(many['Xc'], mdl, range(1, 7), 7, 37, 5, glob, glob, lambda i: 0.1 / (1. + i))
    assert closest > 1e-6
    curve = lambda r: [(r['w'][m], r['p'][m], r['idcs'][m]) for m in range(1, 7)]
    for a, b in zip(curve(many), curve(loop)):
        assert np.array_equal(a[2], b[2])
    dev_loop, dev_many = _deviation(curve(loop), ref), _deviation(curve(many), ref)
    print('the example: from the long-double run: loop %.3e (the yardstick), batched %.3e, allowed %.3e; closest weight to zero %.3g'
          % (dev_loop, dev_many, 8. * dev_loop, closest))
    assert dev_loop <= 1e-9
    assert dev_many <= 8. * dev_loop
    assert np.allclose(many['rkl'], loop['rkl'], rtol=1e-6, atol=1e-9) and np.allclose(many['fkl'], loop['fkl'], rtol=1e-6, atol=1e-9)
