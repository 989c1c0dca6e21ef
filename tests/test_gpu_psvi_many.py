"""The batched BatchPSVI run on the device (include/beta_cores_psvi_many.h; BatchPSVICoreset.build_many): every stage of the last
step on the device's own inputs through the seam, against tests/psvi_many_cases.py's long-double restatement and the bounds of
tests/vi_laplace_cases.py and tests/psvi_cases.py; batch independence, repeatability, float32 rows; the batched route against
the loop of single builds; marking, the zero-weight rows, the guards and the position of the random streams."""
import ctypes as C

import numpy as np
import pytest

import psvi_many_cases as pm

pytestmark = pytest.mark.gpu
N_ROWS = 600
SIZES = [1, 2, 5, 17, 40]


@pytest.fixture(scope='module')
def bc():
    import beta_cores_amd as bc
    bc.default_context()
    return bc


_rows_cache = {}


def rows_of(bc, d, f32=False):
    """(host rows z = y * x as float64 values, their DeviceData): N_ROWS rows of width d, once per module; f32: float32 storage"""
    if (d, f32) not in _rows_cache:
        rng = np.random.RandomState(4100 + d)
        x = rng.randn(N_ROWS, d)
        y = np.where(rng.rand(N_ROWS) < 1. / (1. + np.exp(-x.dot(rng.randn(d)) / np.sqrt(d))), 1., -1.)
        z = (y[:, None] * x).astype(np.float32).astype(np.float64)      # (values a float32 holds: both storages carry the same rows)
        dd = bc.DeviceData(z.astype(np.float32), dtype=np.float32) if f32 else bc.DeviceData(z)
        _rows_cache[d, f32] = (z, dd)
    return _rows_cache[d, f32]


class Run:
    """One native run on SIZES-like problems: nested initial points, weights N / m, draws of a seeded stream.  Chunks of
    opt_itrs - 1 steps and 1 step, so that the seam is read before and after the last step."""

    def __init__(self, bc, d, s, n_sub, itrs, diag=False, sizes=SIZES, f32=False, w0=None, steps=None, chunk=None):
        from beta_cores_amd.coreset import bpsvi
        z, dd = rows_of(bc, d, f32)
        perm = np.random.RandomState(9).permutation(N_ROWS)
        rng = np.random.RandomState(1000 + d + s)
        self.E, self.idx = rng.randn(itrs, s, d), rng.randint(N_ROWS, size=(itrs, n_sub))
        self.z, self.d, self.s, self.n_sub, self.itrs, self.diag, self.sizes = z, d, s, n_sub, itrs, diag, list(sizes)
        self.pts0 = [z[perm[:m]] for m in sizes]
        self.w0 = [np.full(m, N_ROWS / m) for m in sizes] if w0 is None else w0
        self.steps = np.array([[1. / (1. + i) for i in range(itrs)] for _ in sizes]).reshape(len(sizes), itrs) if steps is None else steps
        self.seams, at = [], [0]

        def draw(k):
            out = self.E[at[0]:at[0] + k], self.idx[at[0]:at[0] + k]
            at[0] += k
            return out
        self.res = bpsvi.psvi_many_run(dd, self.pts0, self.w0, s, itrs, self.steps, draw, n_sub, n_total=N_ROWS, diag=diag,
                                       chunk_steps=chunk or max(itrs - 1, 1),
                                       on_chunk=lambda done: self.seams.append((done, bpsvi.psvi_many_last_step(dd.ctx, self.sizes, d, s))))
        assert at[0] == itrs                                   # nothing was drawn past the last step
        self.last = self.seams[-1][1]

    def same_bits(self, other, mine=None, theirs=None):
        mine = range(len(self.sizes)) if mine is None else mine
        theirs = range(len(other.sizes)) if theirs is None else theirs
        return all(np.array_equal(self.res['w'][a], other.res['w'][b]) and np.array_equal(self.res['pts'][a], other.res['pts'][b])
                   and np.array_equal(self.res['modes'][a], other.res['modes'][b]) for a, b in zip(mine, theirs))


# ---------------------------------------------------------------- 1. each stage of the last step, on the device's own inputs
@pytest.mark.parametrize('d,s,n_sub,itrs,diag', [(3, 7, 37, 1, False), (16, 100, 64, 2, True), (33, 100, 200, 4, False),
                                                  (33, 7, 37, 4, True), (128, 100, 200, 2, False), (16, 7, 200, 1, False)])
def test_stages_of_the_last_step(bc, d, s, n_sub, itrs, diag):
    r = Run(bc, d, s, n_sub, itrs, diag)
    assert r.res['marked'] == [] and [done for done, _ in r.seams] == ([itrs] if itrs == 1 else [itrs - 1, itrs])
    L, ptr = r.last, r.last['row_ptr']
    before = r.seams[-2][1] if itrs > 1 else None              # its state AFTER step itrs - 2: the moments before the last step
    rows, i = r.z[r.idx[itrs - 1]], itrs - 1
    for p, m in enumerate(r.sizes):
        sl = slice(ptr[p], ptr[p + 1])
        label = 'D %d S %d n_sub %d steps %d m %d' % (d, s, n_sub, itrs, m)
        wb, pb = L['w_before'][sl], L['pts_before'][sl]
        if before is None:
            assert np.array_equal(wb, r.w0[p]) and np.array_equal(pb, r.pts0[p])
        else:
            assert np.array_equal(wb, before['w'][sl]) and np.array_equal(pb, before['pts'][sl])
        pm.check_mode_and_draw(label, pb, wb, r.E[i], diag, L['mode'][p], L['theta'][p])
        pm.check_stage34(label, rows, N_ROWS / n_sub, pb, wb, L['theta'][p], L['target'][p], L['resid'][p], L['gw'][sl])
        pm.check_point_grad(label, pb, wb, L['theta'][p], L['resid'][p], L['gp'][sl])
        # the state after ADAM: util/opt.py's statements on the device's gradient, to <= 1 ulp
        x0, g = np.concatenate((wb, pb.ravel())), np.concatenate((L['gw'][sl], L['gp'][sl].ravel()))
        m1 = np.zeros_like(x0) if before is None else np.concatenate((before['mom1_w'][sl], before['mom1_p'][sl].ravel()))
        m2 = np.zeros_like(x0) if before is None else np.concatenate((before['mom2_w'][sl], before['mom2_p'][sl].ravel()))
        x, m1, m2 = pm.adam_step(x0, g, m1, m2, r.steps[p, i], i, np.arange(m))
        for name, got, want in (('x', np.concatenate((L['w'][sl], L['pts'][sl].ravel())), x),
                                ('mom1', np.concatenate((L['mom1_w'][sl], L['mom1_p'][sl].ravel())), m1),
                                ('mom2', np.concatenate((L['mom2_w'][sl], L['mom2_p'][sl].ravel())), m2)):
            worst = float(pm.ulps(got, want).max())
            print('%s ADAM %s: %.2f ulp' % (label, name, worst))
            assert worst <= 1., (label, name, worst)
        assert np.array_equal(r.res['w'][p], L['w'][sl]) and np.array_equal(r.res['pts'][p], L['pts'][sl]) and \
            np.array_equal(r.res['modes'][p], L['mode'][p])    # what _end hands out is the state the seam shows
        assert L['newton'][p, 0] >= 0 and L['newton'][p, 1] >= L['newton'][p, 0] and L['flag'][p] == 0


# ---------------------------------------------------------------- 2. batch independence, 3. repeatability and float32 rows
@pytest.mark.parametrize('d,s,n_sub,diag', [(33, 100, 37, False), (16, 7, 200, True)])
def test_bits_do_not_depend_on_the_batch(bc, d, s, n_sub, diag):
    whole = Run(bc, d, s, n_sub, 3, diag)
    assert Run(bc, d, s, n_sub, 3, diag).same_bits(whole)                       # a repeated run: the same bits
    assert Run(bc, d, s, n_sub, 3, diag, chunk=1).same_bits(whole)              # however the steps are chunked
    for p, m in enumerate(SIZES):
        assert Run(bc, d, s, n_sub, 3, diag, sizes=[m]).same_bits(whole, [0], [p]), m
    order = [3, 0, 4, 2, 1]
    assert Run(bc, d, s, n_sub, 3, diag, sizes=[SIZES[j] for j in order]).same_bits(whole, range(5), order)


def test_float32_rows_give_the_bits_of_their_widened_copy(bc):
    assert Run(bc, 33, 100, 37, 3, f32=True).same_bits(Run(bc, 33, 100, 37, 3))
    assert Run(bc, 3, 7, 200, 2, f32=True).same_bits(Run(bc, 3, 7, 200, 2))      # (rows of 12 bytes: the narrow gather)


# ---------------------------------------------------------------- 4. against the existing single-size path
def _coreset(bc, d, s, n_sub, diag, fused, seed):
    _, dd = rows_of(bc, d)
    smp = bc.samplers.LogisticLaplaceSampler(np.zeros(d), diag=diag, rng=np.random.RandomState(seed), solver='newton')
    prj = bc.DeviceProjector(smp, s, bc.likelihoods.LogisticRegression())
    return bc.BatchPSVICoreset(dd, prj, opt_itrs=6, n_subsample_opt=n_sub, fused_gradient=fused)


def _deviation(a, b):
    """the largest |a - b| / (1 + |b|) over the weights and points of two curves (the same points must have survived)"""
    worst = 0.
    for (wa, pa, ia), (wb, pb, ib) in zip(a, b):
        assert np.array_equal(ia, ib)
        worst = max(worst, float((np.abs(wa - wb) / (1. + np.abs(wb))).max()), float((np.abs(pa - pb) / (1. + np.abs(pb))).max()))
    return worst


@pytest.mark.parametrize('d,s,n_sub,diag', [(16, 100, 64, False), (33, 7, 37, True)])
def test_batched_route_against_the_loop_of_single_builds(bc, d, s, n_sub, diag):
    """The yardstick is the deviation between the two single-size routes the library already had (fused_gradient True and False,
    same seeds, 6 steps); the batched route may deviate from the fused loop by 8 times that: it adds the device Cholesky's and
    draw's rounding to the gradient's (profiles/psvi_many_notes.md).

    Measured on one MI355X (deviation = the largest |a - b| / (1 + |b|) over the weights and points of the five sizes):
      D 33, S 7,   n_sub 37, diag:  yardstick 1.531e-13, batched against fused 2.395e-13, allowed 1.225e-12;
      D 16, S 100, n_sub 64, full:  yardstick 6.619e-14, batched against fused 4.439e-13, allowed 5.295e-13.
    The second case is what put the full Newton step behind the device's mode search (bc_pm_fit): without it the search ended
    7.4e-12 from the mode at step 4 of the two-point size and the case missed the allowance tenfold."""
    curves = {}
    for name, fused, route in (('fused', True, 'each'), ('unfused', False, 'each'), ('batched', True, 'batched'), ('auto', True, 'auto')):
        alg = _coreset(bc, d, s, n_sub, diag, fused, seed=5)
        mode0 = alg.ll_projector.sampler._mode.copy()
        np.random.seed(6)
        curves[name] = alg.build_many(SIZES, route=route)
        assert alg.wts.size == 0 and np.array_equal(alg.ll_projector.sampler._mode, mode0)      # the object's own state is left alone
    assert curves['batched'].route == 'batched' == curves['auto'].route and curves['fused'].route == 'each'
    assert curves['batched'].marked == [] and curves['batched'].device_ms > 0.
    assert all(np.array_equal(x, y) for a, b in zip(curves['batched'], curves['auto']) for x, y in zip(a, b))
    yard, seen = _deviation(curves['fused'], curves['unfused']), _deviation(curves['batched'], curves['fused'])
    print('D %d S %d n_sub %d diag %d: fused vs unfused %.3e (the yardstick), batched vs fused %.3e, allowed %.3e' % (d, s, n_sub, diag, yard, seen, 8. * yard))
    assert seen <= 8. * yard


# ---------------------------------------------------------------- 5. marking, 6. zero weights
def test_a_nan_weight_marks_its_problem_alone(bc):
    w0 = [np.full(m, N_ROWS / m) for m in SIZES]
    w0[2][3] = np.nan
    bad = Run(bc, 16, 100, 64, 3, w0=w0)
    assert bad.res['marked'] == [2] and list(bad.res['status']) == [0, 0, 1, 0, 0] and bad.res['w'][2] is None and bad.res['pts'][2] is None
    assert np.all(np.isnan(bad.res['modes'][2]))               # (the wrapper's fill: nothing was copied for it)
    assert bad.last['flag'][2] == 1 and not bad.last['flag'][[0, 1, 3, 4]].any()
    rest = Run(bc, 16, 100, 64, 3, sizes=[1, 2, 17, 40])
    assert bad.same_bits(rest, [0, 1, 3, 4], [0, 1, 2, 3])     # the others' bits: those of a batch without it


def test_a_weight_projected_to_zero_keeps_an_exactly_zero_point_gradient(bc):
    steps = np.array([[50., 0.5]] * len(SIZES))                # a first step long enough to push weights of 35 and less below zero
    r = Run(bc, 16, 100, 64, 2, steps=steps)
    assert r.res['marked'] == []
    L = r.last
    zero = np.where(L['w_before'] == 0.)[0]
    assert zero.size >= 3 and np.all(L['w_before'] >= 0.)
    assert np.all(L['gp'][zero] == 0.) and np.any(L['gp'][L['w_before'] > 0.] != 0.)


# ---------------------------------------------------------------- 7. guards
def test_uncovered_configurations_raise_before_a_launch(bc):
    z, dd = rows_of(bc, 16)
    lin = bc.DeviceProjector(bc.samplers.LinregPosteriorSampler(np.zeros(15), np.eye(15), 1., rng=np.random.RandomState(0)), 7,
                             bc.likelihoods.LinearRegression(1.))
    with pytest.raises(NotImplementedError, match='LogisticRegression'):
        bc.BatchPSVICoreset(dd, lin, opt_itrs=2, n_subsample_opt=37).build_many([1, 2], route='batched')
    bfgs = bc.DeviceProjector(bc.samplers.LogisticLaplaceSampler(np.zeros(16), rng=np.random.RandomState(0)), 7, bc.likelihoods.LogisticRegression())
    with pytest.raises(NotImplementedError, match='newton'):
        bc.BatchPSVICoreset(dd, bfgs, opt_itrs=2, n_subsample_opt=37).build_many([1, 2], route='batched')
    every_row = bc.BatchPSVICoreset(dd, _coreset(bc, 16, 7, 37, False, True, 1).ll_projector, opt_itrs=2, pin_data=False)
    with pytest.raises(NotImplementedError, match='n_subsample_opt'):
        every_row.build_many([1, 2], route='batched')
    assert every_row.build_many([1, 2]).route == 'each'        # 'auto' takes the loop
    alg = _coreset(bc, 16, 7, 37, False, True, 1)
    alg.ll_projector.encoder = object()
    with pytest.raises(NotImplementedError, match='encoder'):
        alg.build_many([1, 2], route='batched')
    alg.ll_projector.encoder = None
    alg.opt_itrs = 0
    with pytest.raises(NotImplementedError, match='opt_itrs'):
        alg.build_many([1, 2], route='batched')
    # the documented limits: refused by the native call, before anything is enqueued; 'auto' takes the loop instead
    from beta_cores_amd.coreset import bpsvi
    wide = bc.DeviceData(np.random.RandomState(0).randn(40, 129))
    no_draw = lambda k: pytest.fail('a refused run drew random numbers')
    with pytest.raises(ValueError, match='D = 129'):
        bpsvi.psvi_many_run(wide, [np.zeros((1, 129))], [np.ones(1)], 7, 2, np.ones((1, 2)), no_draw, 5)
    for kw, msg in ((dict(S=257), 'S = 257'), (dict(n_sub=bpsvi.PSVI_MANY_MAX_SUB + 1), 'n_sub'), (dict(itrs=0), 'opt_itrs'),
                    (dict(m=bpsvi.PSVI_MANY_MAX_POINTS + 1), 'points')):
        m, S, itrs, n_sub = kw.get('m', 2), kw.get('S', 7), kw.get('itrs', 2), kw.get('n_sub', 5)
        with pytest.raises(ValueError, match=msg):
            bpsvi.psvi_many_run(dd, [np.zeros((m, 16))], [np.ones(m)], S, itrs, np.ones((1, max(itrs, 1)))[:, :itrs], no_draw, n_sub)
    with pytest.raises(ValueError, match='work space'):
        bpsvi.psvi_many_run(dd, [np.zeros((1, 16))] * 64, [np.ones(1)] * 64, 256, 2, np.ones((64, 2)), no_draw, bpsvi.PSVI_MANY_MAX_SUB)
    ms = C.c_double(-1.)
    N = bc._native
    N.call('bc_psvi_many_device_ms', dd.ctx.h, C.byref(ms))
    assert ms.value >= 0.


def test_the_run_holds_the_context_and_a_failed_chunk_closes_with_end(bc):
    from beta_cores_amd.coreset import bpsvi
    from beta_cores_amd.device import _ptr
    N = bc._native
    lib = N.load()
    z, dd = rows_of(bc, 16)
    th = np.random.RandomState(2).randn(7, 16) * 0.2
    prj = bc.DeviceProjector(lambda n, w, p: th, 7, bc.likelihoods.LogisticRegression())
    pts, w = np.ascontiguousarray(z[:3]), np.full(3, 200.)
    row_ptr, steps, moments = np.array([0, 1, 3], dtype=np.int64), np.ones((2, 2)), np.ones((2, 2))
    begin = lambda: lib.bc_psvi_many_begin(dd.ctx.h, dd.h, int(prj.model.model_id), 2, 0, _ptr(pts), _ptr(w), _ptr(row_ptr), 2, None, 7, 2,
                                           _ptr(steps), _ptr(moments), 5, 120.)
    # a pending gradient refuses the run ...
    params = np.zeros(1)
    N.call('bc_psvi_gradient_begin', dd.ctx.h, dd.h, _ptr(pts), 3, int(prj.model.model_id), _ptr(th), 7, _ptr(params), 0, _ptr(w), 1.)
    assert begin() == N.BC_INVALID_ARGUMENT and b'gradient is pending' in lib.bc_last_error()
    gw, gp = np.empty(3), np.empty((3, 16))
    N.call('bc_psvi_gradient_end', dd.ctx.h, _ptr(gw), _ptr(gp), None)
    # ... and the open run refuses a gradient, another run of its kind and the other runs
    assert begin() == N.BC_OK
    with pytest.raises(ValueError, match='bc_psvi_many run is open'):
        prj.psvi_gradient(dd, pts, w)
    assert begin() == N.BC_INVALID_ARGUMENT and b'already open' in lib.bc_last_error()
    with pytest.raises(ValueError, match='bc_psvi_many run is open'):
        bc.samplers.logistic_laplace_many([(z[:4], np.ones(4))])
    # an index out of range: refused before anything of the chunk is enqueued; the run has failed and _end closes it
    E, idx = np.zeros((1, 7, 16)), np.array([[0, 1, 2, 3, N_ROWS]], dtype=np.int64)
    assert lib.bc_psvi_many_chunk_begin(dd.ctx.h, _ptr(E), _ptr(idx), 1) == N.BC_INVALID_ARGUMENT and b'out of range' in lib.bc_last_error()
    idx[0, 4] = 4
    assert lib.bc_psvi_many_chunk_begin(dd.ctx.h, _ptr(E), _ptr(idx), 1) == N.BC_INVALID_ARGUMENT and b'has failed' in lib.bc_last_error()
    assert lib.bc_psvi_many_chunk_end(dd.ctx.h, None) == N.BC_INVALID_ARGUMENT
    ow, op, om, ost = np.full(3, 7.), np.full((3, 16), 7.), np.full((2, 16), 7.), np.full(2, 7, dtype=np.int32)
    assert lib.bc_psvi_many_end(dd.ctx.h, _ptr(ow), _ptr(op), _ptr(om), _ptr(ost)) == N.BC_INVALID_ARGUMENT and np.all(ow == 7.) and np.all(ost == 7)
    assert lib.bc_psvi_many_end(dd.ctx.h, None, None, None, None) == N.BC_INVALID_ARGUMENT      # (that call closed it)
    assert prj.psvi_gradient(dd, pts, w) is not None and begin() == N.BC_OK
    assert lib.bc_psvi_many_end(dd.ctx.h, None, None, None, None) == N.BC_OK
    # the Python wrapper closes the run when a draw raises
    def boom(k):
        raise KeyError('draw')
    with pytest.raises(KeyError):
        bpsvi.psvi_many_run(dd, [pts[:1], pts[1:]], [w[:1], w[1:]], 7, 2, np.ones((2, 2)), boom, 5)
    assert begin() == N.BC_OK and lib.bc_psvi_many_end(dd.ctx.h, None, None, None, None) == N.BC_OK


# ---------------------------------------------------------------- 8. the position of the random streams
@pytest.mark.parametrize('own_rng', [True, False])
def test_streams_stand_where_one_build_leaves_them(bc, own_rng):
    ends = []
    for route in ('batched', 'each'):
        alg = _coreset(bc, 16, 7, 37, False, True, seed=3)
        if not own_rng:
            alg.ll_projector.sampler._rng = None               # the normals come from the global stream too
        np.random.seed(8)
        alg.build_many([1, 5, 17], route=route)
        rng = alg.ll_projector.sampler._rng
        ends.append((np.random.rand(3), rng.rand(3) if own_rng else None))
    assert np.array_equal(ends[0][0], ends[1][0]) and (not own_rng or np.array_equal(ends[0][1], ends[1][1]))
    alg = _coreset(bc, 16, 7, 37, False, True, seed=3)
    if not own_rng:
        alg.ll_projector.sampler._rng = None
    np.random.seed(8)
    alg.build(1, 5)
    rng = alg.ll_projector.sampler._rng
    assert np.array_equal(np.random.rand(3), ends[0][0]) and (not own_rng or np.array_equal(rng.rand(3), ends[0][1]))
