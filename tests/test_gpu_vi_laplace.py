"""The logistic Laplace sampler in the device weight optimisation (k_vi_laplace; include/beta_cores_vilaplace.h): the mode and
the draw of one-step runs against the formulas in long double (tests/vi_laplace_cases.py, the bounds of
tests/test_vi_laplace_cpu.py), and the device loop of SparseVICoreset / BetaCoreset with
LogisticLaplaceSampler(solver='newton') against the host loop on the same draws under the contract of
tests/test_gpu_vi_optimize.py (selections exact, weights within RTOL = 1e-5, ATOL = 1e-12, the stream where the host leaves it).

The data are 3000 resident rows z = y * x per D; they do not enter the mode search, which sees the coreset rows only."""
import ctypes

import numpy as np
import pytest

import test_gpu_vi_optimize as tvo
import vi_laplace_cases as lc

pytestmark = pytest.mark.gpu
RTOL, ATOL = tvo.RTOL, tvo.ATOL
N_ROWS = 3000


@pytest.fixture(scope='module')
def bc():
    import beta_cores_amd as bc
    bc.default_context()
    return bc


def logit_rows(n, D, seed):
    rng = np.random.RandomState(seed)
    X = rng.randn(n, D)
    y = np.where(rng.rand(n) < 1. / (1. + np.exp(-X.dot(rng.randn(D) / np.sqrt(D)))), 1., -1.)
    return y[:, None] * X


def data(bc, D, dtype=None):
    return tvo.resident(bc, ('logit', N_ROWS, D, dtype), lambda: logit_rows(N_ROWS, D, 20 + D), dtype=dtype)


class _Recording:
    """An `rng` that draws from RandomState(seed) and keeps what it handed out."""

    def __init__(self, seed):
        self.rng, self.blocks = np.random.RandomState(seed), []

    def randn(self, n, d):
        self.blocks.append(self.rng.randn(n, d))
        return self.blocks[-1].copy()


# ---------------------------------------------------------------- 7: the mode and the draw of one-step runs
def one_step(bc, c):
    """(vi_last_mode(), vi_last_draw()) after a one-step run on case c: start, weights, rows and normals are the case's."""
    sampler = bc.samplers.LogisticLaplaceSampler(np.zeros(c['d']), diag=c['diag'], rng=np.random.RandomState(0), solver='newton')
    prj = bc.DeviceProjector(sampler, c['s'], bc.likelihoods.LogisticRegression())
    sampler._rng, sampler._mode = tvo._FixedNormals(c['E']), c['start'].copy()
    assert prj.vi_optimize(data(bc, c['d'])[1], c['Z'], c['w'], 1, lambda i: 1.) is not None and prj.vi_optimize_calls == 1
    mode = prj.vi_last_mode()
    assert np.array_equal(sampler._mode, mode['mode'])           # written back for the sampler's next call
    return mode, prj.vi_last_draw()


def check_case(bc, c, label):
    mode, draw = one_step(bc, c)
    assert draw['pad_max'] == 0. and np.all(draw['saux'] == 0.) and np.all(draw['raw'] == 0.)
    assert 1 <= mode['newton'] <= 200 and mode['newton_total'] == mode['newton'] and 0 <= mode['halvings'] <= 34
    ratios = lc.check_mode_and_draw(c, mode['mode'], draw['theta'], label)
    again_mode, again_draw = one_step(bc, c)
    assert np.array_equal(again_mode['mode'], mode['mode']) and np.array_equal(again_draw['theta'], draw['theta'])      # the same bits
    assert (again_mode['newton'], again_mode['halvings']) == (mode['newton'], mode['halvings'])
    return ratios


@pytest.mark.parametrize('d', lc.DIMS)
def test_device_mode_and_draw(bc, d):
    worst = [0., 0.]
    for i, (m, s) in enumerate(lc.SHAPES):
        rm, rd = check_case(bc, lc.make_case(d, m, s, variant=i + d), 'device')
        worst = [max(worst[0], rm), max(worst[1], rd)]
    print('worst error / bound at D = %d: mode %.3g, draw %.3g' % (d, worst[0], worst[1]))


@pytest.mark.parametrize('which', ['far start', 'large margins', 'diag D3', 'diag D128'])
def test_device_mode_and_draw_of_the_other_cases(bc, which):
    c = {'far start': lc.far_start_case, 'large margins': lc.large_margin_case, 'diag D3': lambda: lc.make_case(3, 7, 5, variant=3, diag=True),
         'diag D128': lambda: lc.make_case(128, 130, 100, variant=128, diag=True)}[which]()
    check_case(bc, c, 'device, ' + which)


@pytest.mark.parametrize('d,m,s', [(1, 1, 1), (16, 7, 5), (128, 130, 100)])
def test_all_weights_zero_is_the_prior(bc, d, m, s):
    c = lc.make_case(d, m, s)
    c['w'] = np.zeros(m)
    mode, draw = one_step(bc, c)
    assert np.array_equal(draw['theta'], c['E']) and np.all(mode['mode'] == 0.) and mode['newton'] == 0 and draw['pad_max'] == 0.
    c['start'] = 50. * np.ones(d)
    mode, draw = one_step(bc, c)
    assert np.all(mode['mode'] == 0.) and mode['newton'] == 1 and np.array_equal(draw['theta'], c['E'])


# ---------------------------------------------------------------- 8: the device loop against the host loop on the same draws
ITRS = 8


def make_alg(bc, kind, rows, dd, S, m, seed, nsub, device, itrs=ITRS, diag=False, rng=None, w_scale=None):
    """A coreset of m given rows z = y * x with weights w0, ready for _optimize(): 'svi' or 'bcores' (beta = 0.1)."""
    n, D = rows.shape
    r = np.random.RandomState(seed + 77)
    sampler = bc.samplers.LogisticLaplaceSampler(np.zeros(D), diag=diag, rng=np.random.RandomState(seed) if rng is None else rng, solver='newton')
    model = bc.likelihoods.LogisticRegression()
    kw = dict(opt_itrs=itrs, n_subsample_opt=nsub, device_optimize=device)
    if kind == 'bcores':
        alg = bc.BetaCoreset(dd, bc.DeviceBetaProjector(sampler, S, model), beta=0.1, learn_beta=False, **kw)
    else:
        alg = bc.SparseVICoreset(dd, bc.DeviceProjector(sampler, S, model), **kw)
    idcs = r.choice(n, m, replace=m > n)
    alg._append(list(idcs), rows[idcs])
    w_scale = float(n) / m if w_scale is None else w_scale
    w0 = r.rand(m) * w_scale
    w0[r.rand(m) < 0.2] = 0.
    w0[0] = w_scale
    alg.wts = w0.copy()
    return alg


def host_run(bc, *a, **kw):
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


def device_run(bc, *a, chunk_steps=0, keep=None, **kw):
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
    if keep is not None:
        keep['alg'] = alg
    return alg.wts.copy(), got['trace'], np.random.rand()


LOOP_SHAPES = [(N_ROWS, 1, 5, 1), (N_ROWS, 3, 16, 7), (N_ROWS, 33, 100, 130), (N_ROWS, 128, 256, 100)]


@pytest.mark.parametrize('nsub', [None, 50])
@pytest.mark.parametrize('kind', ['svi', 'bcores'])
@pytest.mark.parametrize('shape', LOOP_SHAPES, ids=lambda s: 'n%d-D%d-S%d-m%d' % s)
def test_device_loop_equals_the_host_loop_on_the_same_draws(bc, shape, kind, nsub):
    n, D, S, m = shape
    rows, dd = data(bc, D)
    args = (kind, rows, dd, S, m, 100 + D, nsub)
    tvo.compare(host_run(bc, *args), device_run(bc, *args), 'logistic %s D=%d S=%d m=%d nsub=%s' % (kind, D, S, m, nsub))


def test_float32_rows(bc):
    rows, dd = data(bc, 16, dtype=np.float32)
    args = ('svi', rows.astype(np.float64), dd, 64, 40, 7, 50)
    tvo.compare(host_run(bc, *args), device_run(bc, *args), 'logistic, float32 rows')


def test_diagonal_covariance(bc):
    rows, dd = data(bc, 33)
    args = ('bcores', rows, dd, 100, 30, 9, 50)
    tvo.compare(host_run(bc, *args, diag=True), device_run(bc, *args, diag=True), 'logistic, diag')
    assert not np.array_equal(device_run(bc, *args)[0], device_run(bc, *args, diag=True)[0])      # (the flag reaches the kernel)


# ---------------------------------------------------------------- 9: warm start
def test_warm_start(bc):
    """The Newton count of step k is what the k-step run's last launch reports (the runs are deterministic): steps 2-6 start
    at the mode before them and take no more steps than step 1, which starts at mu0.  The 6-step run's last draw is the
    Laplace draw of the weights after step 5 (trace[-2]) with the last block of normals.

    The case is the one the warm start exists for (samplers._lr_mode_newton: "2-3 Newton steps instead of 10-20 from mu0"): few
    rows in many dimensions with the weights N / M = 1e4 of a million-row data set, so that the search from mu0 = 0 is a cold
    start in earnest -- asserted below as >= 10 steps.  A warm search is 1-3 Newton steps plus what the host's stopping rule
    spends at the rounding floor of f: there a full step is accepted only when the noise of two values of f allows it, about
    every other time, so the extra steps are geometric (k or more of them with probability about 2^-k) and a first step of 7
    -- what moderate weights give -- would be overtaken now and then by chance, not by a defect."""
    D, S, m = 64, 16, 7
    rows, dd = data(bc, D)
    counts, totals = [], []
    for k in range(1, 7):
        rec, keep = _Recording(5), {}
        w, trace, _ = device_run(bc, 'svi', rows, dd, S, m, 5, 50, itrs=k, rng=rec, keep=keep, w_scale=1e4)
        info = keep['alg'].ll_projector.vi_last_mode()
        counts.append(info['newton'])
        totals.append(info['newton_total'])
    print('Newton steps per step of the run: %s' % counts)
    assert totals == list(np.cumsum(counts))
    assert counts[0] >= 10, 'the first search is no longer a cold start: the case has vanished'
    assert all(c <= counts[0] for c in counts[1:])
    alg = keep['alg']
    draw = alg.ll_projector.vi_last_draw()
    assert draw['pad_max'] == 0.
    c = {'d': D, 'm': m, 's': S, 'Z': np.ascontiguousarray(alg.pts, dtype=np.float64), 'w': trace[-2], 'E': rec.blocks[-1], 'diag': False}
    lc.check_mode_and_draw(c, info['mode'], draw['theta'], 'device, warm start')


# ---------------------------------------------------------------- 10: chunk boundaries
def _abi_args(bc, itrs, nsub, seed=5):
    """Everything the C entry points take for a 33-dimensional run, drawn the way vi_optimize draws."""
    from beta_cores_amd.util.opt import adam_step_arrays
    D, S, m = 33, 100, 130
    rows, dd = data(bc, D)
    alg = make_alg(bc, 'svi', rows, dd, S, m, seed, nsub, device=True, itrs=itrs)
    prj = alg.ll_projector
    np.random.seed(seed)
    E, idx = np.empty((itrs, S, D)), np.empty((itrs, nsub), dtype=np.int64)
    for t in range(itrs):
        E[t] = prj.sampler._normals(S, D)
        idx[t] = np.random.randint(N_ROWS, size=nsub)
    kind, sp = prj.sampler.device_spec()
    return dict(ctx=prj.ctx, dd=dd, core=np.ascontiguousarray(alg.pts, dtype=np.float64), w0=alg.wts.copy(), E=E, idx=idx, kind=kind,
                sp=np.ascontiguousarray(sp), steps=np.ascontiguousarray(adam_step_arrays(itrs, alg.step_sched)), S=S, D=D, m=m,
                itrs=itrs, nsub=nsub, model=prj.model.model_id, prj=prj)


def _p(x):
    return None if x is None else x.ctypes.data_as(ctypes.c_void_p)


def test_chunk_boundary_does_not_change_the_bits(bc):
    from beta_cores_amd import _native as N
    lib = N.load()
    a = _abi_args(bc, 6, 50)
    h, m, S, D = a['ctx'].h, a['m'], a['S'], a['D']
    out = {}
    for chunks in ((6,), (3, 2, 1)):
        N.call('bc_vi_optimize_begin', h, a['dd'].h, _p(a['core']), m, int(a['model']), None, 0, int(a['kind']), _p(a['sp']), S, _p(a['w0']),
               6, _p(a['steps']), a['nsub'], float(N_ROWS) / a['nsub'], 1)
        done, modes = 0, []
        for k in chunks:
            N.call('bc_vi_optimize_chunk_begin', h, _p(a['E'][done:done + k]), _p(a['idx'][done:done + k]), k)
            N.call('bc_vi_optimize_chunk_end', h)
            done += k
            modes.append(a['prj'].vi_last_mode())
        w, trace = np.empty(m), np.empty((6, m))
        N.call('bc_vi_optimize_end', h, _p(w), _p(trace))
        out[chunks] = (w, trace, modes[-1], a['prj'].vi_last_draw()['theta'])
    one, three = out[(6,)], out[(3, 2, 1)]
    assert np.array_equal(one[0], three[0]) and np.array_equal(one[1], three[1]) and np.array_equal(one[3], three[3])
    assert np.array_equal(one[2]['mode'], three[2]['mode']) and one[2]['newton_total'] == three[2]['newton_total']
    assert not np.array_equal(one[1][2], one[1][3])               # (the steps behind the first boundary moved the weights)
    # the seam follows the rules of the last-draw seam: another dimension, a NULL, a run of another kind
    assert lib.bc_vi_laplace_last_mode(h, D + 1, _p(np.empty(D + 1)), _p(np.zeros(3, dtype=np.int32))) == N.BC_INVALID_ARGUMENT
    assert lib.bc_vi_laplace_last_mode(h, D, None, None) == N.BC_INVALID_ARGUMENT
    lin, dlin = tvo.resident(bc, ('lin', 9000, 8), lambda: tvo.linreg_rows(9000, 8, 18))
    tvo.device_run(bc, 'svi', lin, dlin, 64, 20, 5, 200, itrs=2)
    assert lib.bc_vi_laplace_last_mode(h, 8, _p(np.empty(8)), _p(np.zeros(3, dtype=np.int32))) == N.BC_INVALID_ARGUMENT
    assert 'kind' in N.last_error()


def test_a_model_of_another_kind_is_refused(bc):
    from beta_cores_amd import _native as N
    a = _abi_args(bc, 2, 50)
    lin = bc.likelihoods.LinearRegression(1.0)
    params = np.ascontiguousarray(lin.params(), dtype=np.float64)
    st = N.load().bc_vi_optimize_begin(a['ctx'].h, a['dd'].h, _p(a['core']), a['m'], int(lin.model_id), _p(params), int(params.shape[0]), 2,
                                       _p(a['sp']), a['S'], _p(a['w0']), 2, _p(a['steps']), a['nsub'], 60., 0)
    assert st == N.BC_INVALID_ARGUMENT and 'does not go with sampler kind 2' in N.last_error()


# ---------------------------------------------------------------- 11: whole builds
@pytest.mark.parametrize('kind', ['svi', 'bcores'])
def test_whole_builds(bc, kind):
    """Three greedy steps with the weight optimisation behind each, device against host.  (Seed 31, the first one tried.  Were the top
    two correlations of a step of the host run within 1e-9 relative, rounding alone could pick differently on the device and another
    seed would be taken here; no seed has had to be replaced.)"""
    D, S, itrs = 16, 64, 7
    rows, dd = data(bc, D)
    sched = lambda i: 1. / (1. + i)
    model = bc.likelihoods.LogisticRegression()
    out = {}
    for device in (False, True):
        np.random.seed(31)
        sampler = bc.samplers.LogisticLaplaceSampler(np.zeros(D), solver='newton')
        if kind == 'bcores':
            alg = bc.BetaCoreset(dd, bc.DeviceBetaProjector(sampler, S, model), beta=0.1, learn_beta=False, opt_itrs=itrs,
                                 n_subsample_opt=50, step_sched=sched, device_optimize=device)
        else:
            alg = bc.SparseVICoreset(dd, bc.DeviceProjector(sampler, S, model), opt_itrs=itrs, n_subsample_opt=50, step_sched=sched,
                                     device_optimize=device)
        steps = []
        for m in range(3):
            alg.build(1, m + 1)
            steps.append((alg.idcs.copy(), alg.wts.copy()))
        out[device] = (steps, alg.device_optimize_calls, sampler._mode.copy(), alg.ll_projector.vi_last_mode()['mode'] if device else None,
                       np.random.rand())
    assert out[False][1] == 0 and out[True][1] == 3
    for m in range(3):
        np.testing.assert_array_equal(out[True][0][m][0], out[False][0][m][0])
        np.testing.assert_allclose(out[True][0][m][1], out[False][0][m][1], rtol=RTOL, atol=ATOL)
    assert out[True][4] == out[False][4], 'the global stream does not stand where the host loop leaves it'
    assert np.array_equal(out[True][2], out[True][3])            # sampler._mode is the device's last mode


# ---------------------------------------------------------------- 12: declines leave the results unchanged
@pytest.mark.parametrize('why', ['bfgs', 'linreg model', 'D129'])
def test_declines_leave_the_results_unchanged(bc, why):
    D = 129 if why == 'D129' else 6
    S = 32

    class OnLinregRows(bc.samplers.LogisticLaplaceSampler):
        """This sampler on rows [x, y] of a linear-regression model: it fits z = y * x."""

        def __call__(self, n, wts, pts):
            if np.ndim(pts) == 2 and pts.shape[1] == D + 1:
                pts = pts[:, :-1] * pts[:, -1:]
            return super().__call__(n, wts, pts)

    def build(device):
        np.random.seed(3)
        if why == 'linreg model':
            rows, dd = tvo.resident(bc, ('lin', 3000, D), lambda: tvo.linreg_rows(3000, D, 10 + D))
            sampler, model = OnLinregRows(np.zeros(D), solver='newton'), bc.likelihoods.LinearRegression(1.0)
        else:
            rows, dd = data(bc, D)
            sampler = bc.samplers.LogisticLaplaceSampler(np.zeros(D), solver='bfgs' if why == 'bfgs' else 'newton')
            model = bc.likelihoods.LogisticRegression()
        prj = bc.DeviceProjector(sampler, S, model)
        alg = bc.SparseVICoreset(dd, prj, opt_itrs=4, n_subsample_opt=100, device_optimize=device)
        for m in range(3):
            alg.build(1, 30)
        if device:
            assert prj.vi_optimize(dd, alg.pts, alg.wts, 4, lambda i: 1. / (1. + i), n_subsample=100, n_total=N_ROWS) is None
        return alg.idcs.copy(), alg.wts.copy(), np.random.rand(), alg.device_optimize_calls
    off, on = build(False), build(True)
    assert on[3] == 0 and off[3] == 0
    assert off[0].size > 0 and np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1]) and on[2] == off[2]


# ---------------------------------------------------------------- 13: the failure status
def test_a_weight_that_is_not_finite_raises_and_leaves_the_context_usable(bc):
    rows, dd = data(bc, 33)
    args = ('svi', rows, dd, 100, 130, 5, 50)
    alg = make_alg(bc, *args, device=True)
    alg.wts[7] = np.nan
    before, held = alg.wts.copy(), alg.wts
    with pytest.raises(np.linalg.LinAlgError) as err:
        alg._optimize()
    assert 'not finite' in str(err.value)
    assert alg.wts is held and np.array_equal(alg.wts, before, equal_nan=True) and alg.device_optimize_calls == 0
    draw = alg.ll_projector.vi_last_draw()
    assert np.all(draw['theta'] == 0.) and draw['pad_max'] == 0.         # the first step failed: nothing was written
    mode = alg.ll_projector.vi_last_mode()
    assert np.all(mode['mode'] == 0.) and mode['newton_total'] == 0      # (the start point of the run)
    tvo.compare(host_run(bc, *args), device_run(bc, *args), 'after the failure')


# ---------------------------------------------------------------- 14: the largest accepted coresets
@pytest.mark.parametrize('D,S,m', [(128, 64, 465), (1, 16, 20000)])
def test_largest_accepted_coreset(bc, D, S, m):
    assert m * (D + 1) <= 60000 and (D != 128 or (m + 1) * (D + 1) > 60000)
    rows, dd = data(bc, D)
    args = ('svi', rows, dd, S, m, 3, 50)
    tvo.compare(host_run(bc, *args, itrs=1), device_run(bc, *args, itrs=1), 'logistic D=%d m=%d' % (D, m))
