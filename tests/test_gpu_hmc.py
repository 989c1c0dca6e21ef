"""The multi-chain logistic rows pass (k_lr_rows_mc) and the device-resident HMC run (include/beta_cores_hmc.h) on the GPU.

1. The rows pass against the formula in np.longdouble, element-wise, under the bound derived in tests/hmc_cases.py
   (rows_pass_bound): row-tile, range, k-block and chain-padding edges; weighted / unweighted / zero weights; float32 rows; rows
   on both sides of the branch at m = 100.
2. Independence and repeatability: a chain's bits alone, in a batch of 16 and in a batch of 64; a second call; C = 1 against K5.
3. The run against the restatement on the same draws (conditions on the inputs asserted on the restatement).
4. One statistical guard against gross errors.
5. Weighted-coreset use through samplers.logistic_hmc.
"""
import ctypes
import functools

import numpy as np
import pytest

import hmc_cases as hc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def bc():
    import beta_cores_amd as bc
    bc.default_context()
    return bc


def _p(x):
    return None if x is None else x.ctypes.data_as(ctypes.c_void_p)


# ------------------------------------------------------------------ 1. the rows pass under the derived bound
# (n, D, C): a list, not a product.  n: one row, the edges of the 16-row tile (15, 16, 17), of four tiles (63, 65), many
# one-tile ranges (1000, 4099: 16 rows per range on a 256-CU device) and ranges of several tiles with a short last one (70001);
# D: the k-block of 4 (1, 3, 4, 5), every kernel instance and its edge (16 | 17 | 127, 128 | 129, 256: the limit);
# C: the chain padding (1, 15, 16, 17, 64).  (33000, 256, 3): the three-wave instance of D > 128 over ranges of three tiles.
SHAPES = [(1, 1, 1), (15, 3, 15), (16, 4, 16), (17, 5, 17), (63, 16, 64), (65, 17, 1), (1000, 127, 16), (4099, 128, 17),
          (1000, 129, 15), (4099, 256, 64), (17, 256, 1), (70001, 17, 3), (33000, 33, 16), (40000, 65, 17), (33000, 256, 3)]


@functools.lru_cache(maxsize=None)
def _shape_case(n, d, c):
    Z, w = hc.make_data(n, d, 1000 * d + n % 997 + c)
    th = np.random.RandomState(n + d + c).randn(c, d) / np.sqrt(d)
    return Z, w, th


def _check(bc, Z, w, th, label, dtype=np.float64):
    from beta_cores_amd import posterior
    dz = bc.DeviceData(Z.astype(dtype), dtype=dtype) if dtype == np.float32 else bc.DeviceData(Z)
    Zx = Z.astype(dtype).astype(np.float64)            # (float32 rows are widened exactly)
    val, grad = posterior.logistic_logjoint_batch(dz, th, w)
    rv, rg = hc.logjoint(Zx, w, th, np.longdouble)
    bv, bg = hc.rows_pass_bound(Zx, w, th)
    assert np.all(np.isfinite(val)) and np.all(np.isfinite(grad))
    ev, eg = np.abs(val - rv).astype(np.float64), np.abs(grad - rg).astype(np.float64)
    print('rows pass %s: worst error / bound: value %.3f, gradient %.3f' % (label, (ev / bv).max(), (eg / bg).max()))
    assert np.all(ev <= bv), (label, (ev / bv).max())
    assert np.all(eg <= bg), (label, (eg / bg).max())
    return val, grad


@pytest.mark.parametrize('n,d,c', SHAPES)
def test_rows_pass_within_the_derived_bound(bc, n, d, c):
    Z, w, th = _shape_case(n, d, c)
    _check(bc, Z, w, th, 'n=%d D=%d C=%d weighted' % (n, d, c))


# (the last two: float32 rows over ranges of several tiles, the prefetch and the reuse of the LDS tile, at D <= 128 and D > 128)
@pytest.mark.parametrize('n,d,c', [(17, 5, 17), (1000, 127, 16), (4099, 256, 64), (33000, 33, 16), (33000, 256, 3)])
@pytest.mark.parametrize('variant', ['unweighted', 'zero', 'float32'])
def test_rows_pass_variants(bc, n, d, c, variant):
    Z, w, th = _shape_case(n, d, c)
    if variant == 'unweighted':
        _check(bc, Z, None, th, 'n=%d D=%d C=%d unweighted' % (n, d, c))
    elif variant == 'zero':
        val, grad = _check(bc, Z, np.zeros(n), th, 'n=%d D=%d C=%d zero weights' % (n, d, c))
        assert np.array_equal(grad, -th)               # the prior alone
    else:
        _check(bc, Z, w, th, 'n=%d D=%d C=%d float32' % (n, d, c), dtype=np.float32)


@pytest.mark.parametrize('d,c', [(5, 3), (128, 17)])
def test_rows_pass_on_both_sides_of_the_branch(bc, d, c):
    """Rows with |m| in {0.5, 99.9, 100, 120, 800} for every chain, both signs: no NaN, no inf, within the bound."""
    rng = np.random.RandomState(d)
    th = np.tile(rng.randn(d) / np.sqrt(d), (c, 1)) * (1. + 1e-3 * np.arange(c))[:, None]
    base = th[0] / th[0].dot(th[0])
    mags = np.array([0.5, 99.9, 100., 120., 800.])
    jitter = np.array([0., 1e-3, 1e-3, 1e-3])[:, None]               # (the first row of each group sits on the value itself)
    Z = np.concatenate([s * m * base[None, :] + jitter * rng.randn(4, d) for m in mags for s in (1., -1.)])
    w = rng.rand(Z.shape[0]) + 0.5
    m = -Z.dot(th.T)
    assert np.abs(m).max() > 790 and (m >= 100).any() and (m < 100).any() and (np.abs(np.abs(m) - 100.) < 1.).any()
    _check(bc, Z, w, th, 'branch rows D=%d C=%d' % (d, c))


# ------------------------------------------------------------------ 2. independence and repeatability
@pytest.mark.parametrize('n,d', [(4099, 128), (70001, 17), (300, 256)])
def test_a_chains_bits_do_not_depend_on_the_batch(bc, n, d):
    from beta_cores_amd import posterior
    Z, w, _ = _shape_case(n, d, 64)
    th = np.random.RandomState(3).randn(64, d) / np.sqrt(d)
    dz = bc.DeviceData(Z)
    wd = bc.DeviceData(w.reshape(n, 1))
    v64, g64 = posterior.logistic_logjoint_batch(dz, th, wd)
    v64b, g64b = posterior.logistic_logjoint_batch(dz, th, wd)
    assert np.array_equal(v64, v64b) and np.array_equal(g64, g64b)                 # a second call: the same bits
    for pick in (0, 21, 37, 63):
        v1, g1 = posterior.logistic_logjoint_batch(dz, th[pick:pick + 1], wd)      # alone
        assert np.array_equal(v1[0], v64[pick]) and np.array_equal(g1[0], g64[pick]), pick
        batch = np.roll(th[:16], 5, axis=0).copy()                                 # in a batch of 16, at another position
        batch[9] = th[pick]
        v16, g16 = posterior.logistic_logjoint_batch(dz, batch, wd)
        assert np.array_equal(v16[9], v64[pick]) and np.array_equal(g16[9], g64[pick]), pick


@pytest.mark.parametrize('n,d', [(4099, 128), (1000, 5), (300, 256)])
def test_one_chain_agrees_with_k5(bc, n, d):
    """C = 1 against logistic_newton_pass + prior under twice the bound of test 1 (the summation orders differ)."""
    from beta_cores_amd import posterior
    Z, w, th = _shape_case(n, d, 1)
    dz = bc.DeviceData(Z)
    val, grad = posterior.logistic_logjoint_batch(dz, th, w)
    v5, g5 = posterior.logistic_newton_pass(dz, th[0], w, hessian=False)[:2]
    v5 = v5 - 0.5 * d * np.log(2. * np.pi) - 0.5 * th[0].dot(th[0])
    g5 = g5 - th[0]
    bv, bg = hc.rows_pass_bound(Z, w, th)
    assert abs(val[0] - v5) <= 2. * bv[0] and np.all(np.abs(grad[0] - g5) <= 2. * bg[0])


# ------------------------------------------------------------------ 3. the run against the restatement
def _native_run(bc, dz, wd, case, chunks=None, one_call=False, eps=None):
    """(status, samples, logjoint, accept) of the run of `case` on the device: chunked as given, or through the one-call export."""
    from beta_cores_amd import _native as N
    lib = N.load()
    T, c, d = case['E'].shape
    eps = case['eps'] if eps is None else eps
    start, im = np.ascontiguousarray(case['start']), np.ascontiguousarray(case['inv_mass'])
    E, U = np.ascontiguousarray(case['E']), np.ascontiguousarray(case['logU'])
    s, lj, acc = np.full((T, c, d), 7.), np.full((T, c), 7.), np.full((T, c), 7, dtype=np.int32)
    h, wh = dz.ctx.h, (wd.h if wd is not None else None)
    if one_call:
        st = lib.bc_hmc_logistic(h, dz.h, wh, _p(start), c, _p(im), case['L'], float(eps), T, _p(E), _p(U), 0, _p(s), _p(lj), _p(acc))
        return st, s, lj, acc
    st = lib.bc_hmc_begin(h, dz.h, wh, _p(start), c, _p(im), case['L'], T)
    if st:
        return st, s, lj, acc
    i0 = 0
    for k in (chunks or [T]):
        st = lib.bc_hmc_chunk_begin(h, _p(E[i0:i0 + k]), _p(U[i0:i0 + k]), k, float(eps))
        if not st:
            st = lib.bc_hmc_chunk_end(h, _p(s[i0:i0 + k]), _p(lj[i0:i0 + k]), _p(acc[i0:i0 + k]))
        if st:
            break
        i0 += k
    assert lib.bc_hmc_end(h) == N.BC_OK
    return st, s, lj, acc


@functools.lru_cache(maxsize=None)
def _trace(name):
    case = hc.make_trace_case(name)
    return (case,) + hc.trace_tolerance(case)


def _resident(bc, case):
    n = case['Z'].shape[0]
    return bc.DeviceData(case['Z']), (bc.DeviceData(case['w'].reshape(n, 1)) if case['w'] is not None else None)


@pytest.mark.parametrize('name', ['small', 'wide'])
def test_run_follows_the_restatement(bc, name):
    case, ref, tol_s, tol_l = _trace(name)
    hc.check_trace_condition(ref)                                  # (on the restatement: rounding cannot flip a decision)
    dz, wd = _resident(bc, case)
    st, s, lj, acc = _native_run(bc, dz, wd, case)
    assert st == 0
    assert np.array_equal(acc != 0, ref['accept'])
    ds, dl = hc.rel_dev(s, ref['samples']), hc.rel_dev(lj, ref['logjoint'])
    print('run %s: deviation from the long-double restatement: samples %.3g (tol %.3g), log-joint %.3g (tol %.3g)' % (name, ds, tol_s, dl, tol_l))
    assert ds <= tol_s and dl <= tol_l
    # a rejected chain keeps its previous bits exactly
    prev_s = np.vstack((case['start'][None], s[:-1]))
    rej = acc == 0
    assert np.array_equal(s[rej], prev_s[rej])
    assert np.array_equal(lj[1:][rej[1:]], lj[:-1][rej[1:]])
    # chunked 3 + 2 + 1 against one chunk, and the one-call export
    st2, s2, lj2, acc2 = _native_run(bc, dz, wd, case, chunks=[3, 2, 1])
    assert st2 == 0 and np.array_equal(s2, s) and np.array_equal(lj2, lj) and np.array_equal(acc2, acc)
    st3, s3, lj3, acc3 = _native_run(bc, dz, wd, case, one_call=True)
    assert st3 == 0 and np.array_equal(s3, s) and np.array_equal(lj3, lj) and np.array_equal(acc3, acc)
    # the log-joint a chain carries is the one the rows pass gives at its position
    from beta_cores_amd import posterior
    v, _ = posterior.logistic_logjoint_batch(dz, s[-1], wd)
    assert np.array_equal(v, lj[-1])


def test_a_huge_step_rejects_everything(bc):
    """eps = 1e6: every proposal is rejected (H1 not finite, or astronomically large), BC_OK, every sample equals the start."""
    case = _trace('small')[0]
    dz, wd = _resident(bc, case)
    st, s, lj, acc = _native_run(bc, dz, wd, case, eps=1e6)
    assert st == 0 and not acc.any()
    assert np.array_equal(s, np.broadcast_to(case['start'], s.shape))
    assert np.array_equal(lj, np.broadcast_to(lj[0], lj.shape)) and np.all(np.isfinite(lj))


def test_a_nan_weight_marks_the_run_and_copies_nothing(bc):
    from beta_cores_amd import _native as N
    case = dict(_trace('small')[0])
    case['w'] = case['w'].copy()
    case['w'][7] = np.nan
    dz, wd = _resident(bc, case)
    for one_call in (False, True):
        st, s, lj, acc = _native_run(bc, dz, wd, case, one_call=one_call)
        assert st == N.BC_NUMERICAL_PRECISION and 'not finite' in N.last_error()
        assert np.all(s == 7.) and np.all(lj == 7.) and np.all(acc == 7)
    bad = dict(_trace('small')[0])
    bad['start'] = bad['start'].copy()
    bad['start'][1, 2] = np.inf
    dz, wd = _resident(bc, bad)
    assert _native_run(bc, dz, wd, bad)[0] == N.BC_NUMERICAL_PRECISION
    # the context serves the next run
    good = _trace('small')[0]
    dz, wd = _resident(bc, good)
    assert _native_run(bc, dz, wd, good)[0] == 0


def test_refusals(bc):
    """Out-of-range chain counts and dimensions are refused before anything runs; an HMC run and a pending gradient / an open
    weight-optimisation run exclude each other on a context."""
    from beta_cores_amd import _native as N
    lib = N.load()
    case = _trace('small')[0]
    dz, wd = _resident(bc, case)
    h = dz.ctx.h
    T, c, d = case['E'].shape
    n = case['Z'].shape[0]
    im, E, U = np.ascontiguousarray(case['inv_mass']), np.ascontiguousarray(case['E']), np.ascontiguousarray(case['logU'])
    s, lj, acc = np.empty((T, c, d)), np.empty((T, c)), np.empty((T, c), dtype=np.int32)
    for bad in (0, 65, -1):
        start = np.zeros((max(bad, 1), d))
        assert lib.bc_hmc_begin(h, dz.h, wd.h, _p(start), bad, _p(im), 4, T) == N.BC_INVALID_ARGUMENT and 'chains' in N.last_error()
        assert lib.bc_hmc_end(h) == N.BC_INVALID_ARGUMENT                        # no run was opened
        v, g = np.empty(max(bad, 1)), np.empty((max(bad, 1), d))
        assert lib.bc_logistic_logjoint_batch(h, dz.h, wd.h, _p(start), bad, _p(v), _p(g)) == N.BC_INVALID_ARGUMENT
    wide = bc.DeviceData(np.zeros((4, 257)))
    assert lib.bc_hmc_begin(h, wide.h, None, _p(np.zeros((2, 257))), 2, _p(np.ones(257)), 4, T) == N.BC_INVALID_ARGUMENT and '256' in N.last_error()
    start = np.ascontiguousarray(case['start'])
    assert lib.bc_hmc_begin(h, dz.h, wd.h, _p(start), c, _p(im * 0.), 4, T) == N.BC_INVALID_ARGUMENT
    assert lib.bc_hmc_begin(h, dz.h, wd.h, _p(start), c, _p(im), 0, T) == N.BC_INVALID_ARGUMENT
    assert lib.bc_hmc_begin(h, dz.h, dz.h, _p(start), c, _p(im), 4, T) == N.BC_INVALID_ARGUMENT       # weights that are not n x 1
    assert lib.bc_hmc_chunk_begin(h, _p(E), _p(U), T, 0.1) == N.BC_INVALID_ARGUMENT                   # no run is open
    # a run is open: a second run, the batch pass, a gradient and a weight-optimisation run are refused
    m, S = 6, 8
    core, w0, th = np.ascontiguousarray(case['Z'][:m]), np.ones(m), np.zeros((S, d))
    sp, steps = np.zeros(d + 1), np.ones((3, 2))
    grad_args = (h, dz.h, _p(core), m, 2, _p(th), S, None, 0, _p(w0), 1., None)
    opt_args = (h, dz.h, _p(core), m, 2, None, 0, 2, _p(sp), S, _p(w0), 2, _p(steps), 0, 1., 0)
    assert lib.bc_hmc_begin(h, dz.h, wd.h, _p(start), c, _p(im), 4, T) == N.BC_OK
    assert lib.bc_hmc_begin(h, dz.h, wd.h, _p(start), c, _p(im), 4, T) == N.BC_INVALID_ARGUMENT and 'already open' in N.last_error()
    assert lib.bc_logistic_logjoint_batch(h, dz.h, wd.h, _p(start), c, _p(np.empty(c)), _p(np.empty((c, d)))) == N.BC_INVALID_ARGUMENT
    assert lib.bc_vi_gradient_begin(*grad_args) == N.BC_INVALID_ARGUMENT and 'bc_hmc' in N.last_error()
    assert lib.bc_vi_optimize_begin(*opt_args) == N.BC_INVALID_ARGUMENT and 'bc_hmc' in N.last_error()
    assert lib.bc_hmc_chunk_begin(h, _p(E), _p(U), T + 1, 0.1) == N.BC_INVALID_ARGUMENT                # more than the run's iterations
    assert lib.bc_hmc_chunk_begin(h, _p(E), _p(U), T, -0.1) == N.BC_INVALID_ARGUMENT
    assert lib.bc_hmc_chunk_end(h, _p(s), _p(lj), _p(acc)) == N.BC_INVALID_ARGUMENT                    # nothing was enqueued
    assert lib.bc_hmc_chunk_begin(h, _p(E), _p(U), T, case['eps']) == N.BC_OK
    assert lib.bc_hmc_chunk_begin(h, _p(E), _p(U), T, case['eps']) == N.BC_INVALID_ARGUMENT            # a chunk is pending
    assert lib.bc_hmc_chunk_end(h, None, _p(lj), _p(acc)) == N.BC_INVALID_ARGUMENT                     # an output is missing: the chunk stays pending
    assert lib.bc_hmc_chunk_end(h, _p(s), _p(lj), _p(acc)) == N.BC_OK
    assert lib.bc_hmc_end(h) == N.BC_OK
    ref = _native_run(bc, dz, wd, case)
    assert np.array_equal(s, ref[1]) and np.array_equal(acc, ref[3])                                   # the refusals left the run alone
    # the reverse: a pending gradient, then an open weight-optimisation run, refuse an HMC run
    assert lib.bc_vi_gradient_begin(*grad_args) == N.BC_OK
    assert lib.bc_hmc_begin(h, dz.h, wd.h, _p(start), c, _p(im), 4, T) == N.BC_INVALID_ARGUMENT and 'pending' in N.last_error()
    assert lib.bc_vi_gradient_end(h, _p(np.empty(m)), _p(np.empty(S))) == N.BC_OK
    assert lib.bc_vi_optimize_begin(*opt_args) == N.BC_OK
    assert lib.bc_hmc_begin(h, dz.h, wd.h, _p(start), c, _p(im), 4, T) == N.BC_INVALID_ARGUMENT and 'bc_vi_optimize' in N.last_error()
    assert lib.bc_vi_optimize_end(h, None, None) == N.BC_OK
    ms = ctypes.c_double(-1.)
    assert lib.bc_hmc_device_ms(h, ctypes.byref(ms)) == N.BC_OK and ms.value > 0.
    assert lib.bc_hmc_auto_chunk(16, 128) == (32 << 20) // (8 * (16 * 128 + 16)) and lib.bc_hmc_auto_chunk(64, 256) >= 1


# ------------------------------------------------------------------ 4. one statistical guard
def test_statistical_guard(bc):
    """n = 20 000, D = 4, unit weights, C = 16, L = 8, mass from the Laplace diagonal, 300 iterations with the first 100 dropped.
    The pooled mean within 0.25 Laplace standard deviations of the Newton mode per coordinate, the pooled variance within
    [0.8, 1.25] of the Laplace variance: bars 5 x outside what the NumPy restatement does (0.001-0.05 sd, 0.97-1.05 at steps
    0.15 .. 0.6) -- they catch a wrong sign of the prior or a factor in the step, not subtleties."""
    from beta_cores_amd import samplers
    rng = np.random.RandomState(0)
    n, ths = 20000, np.array([1., -0.5, 0.25, 0.3])
    x = rng.randn(n, 4)
    x[:, -1] = 1.
    y = np.where(rng.rand(n) < 1. / (1. + np.exp(-x.dot(ths))), 1., -1.)
    dz = bc.DeviceData(y[:, None] * x)
    res = samplers.logistic_hmc(dz, None, n_samples=300, n_chains=16, step_size=0.3, n_leapfrog=8, inv_mass='laplace',
                                rng=np.random.RandomState(1))
    mode, LSig, _ = samplers.logistic_laplace(None, dz, np.zeros(4), solver='newton')
    var = np.diag(LSig.dot(LSig.T))
    kept = res.samples[100:].reshape(-1, 4)
    shift, ratio = (kept.mean(axis=0) - mode) / np.sqrt(var), kept.var(axis=0) / var
    print('guard: mean shift %s sd, variance ratio %s, acceptance %.3f' % (np.round(shift, 4), np.round(ratio, 3), res.accept_rate.mean()))
    assert np.all(np.abs(shift) <= 0.25) and np.all(ratio >= 0.8) and np.all(ratio <= 1.25)


# ------------------------------------------------------------------ 5. weighted-coreset use
def test_weighted_coreset_through_logistic_hmc(bc):
    """An ndarray of 40 rows with weights: the same samples as the same rows uploaded by hand; zero-weight rows contribute
    nothing: the run with those rows deleted agrees under the trace tolerance (the reduction tree differs, the bits may)."""
    from beta_cores_amd import samplers
    Z, w = hc.make_data(40, 6, 21)
    w = w * 12.
    assert (w == 0.).sum() >= 3 and (w > 0.).sum() >= 20
    rng = np.random.RandomState(2)
    start, im = rng.randn(5, 6) * 0.1, 0.5 + rng.rand(6)
    kw = dict(n_samples=8, n_chains=5, step_size=0.05, n_leapfrog=4, inv_mass=im, start=start, warmup=6, adapt_every=3)
    a = samplers.logistic_hmc(Z, w, rng=np.random.RandomState(3), **kw)
    b = samplers.logistic_hmc(bc.DeviceData(Z), w, rng=np.random.RandomState(3), **kw)
    assert np.array_equal(a.samples, b.samples) and np.array_equal(a.logjoint, b.logjoint) and a.step_size == b.step_size
    assert a.accept.any() and a.device_ms > 0. and a.warmup_steps.shape == (2,)
    keep = w > 0.
    c = samplers.logistic_hmc(Z[keep], w[keep], rng=np.random.RandomState(3), **kw)
    # the tolerance of test 3 for this problem, from the restatement on the draws the kept iterations used
    r = np.random.RandomState(3)
    for k in (3, 3):
        r.randn(k, 5, 6), r.rand(k, 5)
    case = dict(Z=Z, w=w, start=start, inv_mass=im, eps=a.step_size, L=4, E=r.randn(8, 5, 6), logU=np.log(r.rand(8, 5)))
    _, tol_s, tol_l = hc.trace_tolerance(case)
    assert np.array_equal(c.accept, a.accept) and c.step_size == a.step_size
    assert hc.rel_dev(c.samples, a.samples) <= tol_s and hc.rel_dev(c.logjoint, a.logjoint) <= tol_l
    # defaults: the start drawn from the device Laplace fit
    d = samplers.logistic_hmc(Z, w, n_samples=4, n_chains=3, step_size=0.05, n_leapfrog=2, rng=np.random.RandomState(4))
    assert d.samples.shape == (4, 3, 6) and np.all(np.isfinite(d.samples)) and d.start.shape == (3, 6)
