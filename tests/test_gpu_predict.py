"""The held-out scorer of the linear-regression family (k_linreg_predict, include/beta_cores_predict.h) on the GPU.

1. samplers.linreg_predictive against the long-double restatement of tests/predict_cases.py on every case of its table: the sums and
   the per-row outputs element-wise within the derived tolerance; float32 rows give the bits of the same values stored as float64;
   the exact cases bit for bit.
2. The reference's figures (tests/golden/predict_f24.npz).
3. Batch independence and repeatability, bit for bit.
4. Every refusal of the C ABI; a refused call writes nothing and the call after it works.
5. RegressionHeldOut with an encoder: the cache follows encoder.version.
"""
import ctypes
import os

import numpy as np
import pytest

import predict_cases as pc

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(pc.ROOT, 'tests', 'golden', 'predict_f24.npz')
needs_longdouble = pytest.mark.skipif(not pc.LONGDOUBLE_OK, reason='np.longdouble is no wider than float64 on this platform')


@pytest.fixture(scope='module')
def bc():
    import beta_cores_amd as bc
    bc.default_context()
    return bc


def _p(x):
    return None if x is None else x.ctypes.data_as(ctypes.c_void_p)


def _held_of(bc, case):
    return bc.RegressionHeldOut(case['Z'], dtype=np.float32 if case['f32'] else None)


def _score(bc, held, c, per_row=True):
    return bc.linreg_predictive(held, c['mu'], c['F'], c['noise'], c['scale'], per_row=per_row)


# ------------------------------------------------------------------ 1. against the restatement, and the exact cases
@needs_longdouble
@pytest.mark.parametrize('name', pc.NAMES)
def test_predictive_follows_the_restatement(bc, name):
    case, ref = pc.make_case(name), pc.reference(name)
    held = _held_of(bc, case)
    assert held.shape == case['Z'].shape
    got = _score(bc, held, case)
    t, nt = case['mu'].shape[0], case['Z'].shape[0]
    assert got.ll.shape == got.sse.shape == (t,) and got.mean.shape == got.var.shape == (t, nt) and got.n == nt
    pc.compare(got.ll, got.sse, ref, 'device ' + name, mean=got.mean, var=got.var)
    lean = _score(bc, held, case, per_row=False)
    assert lean.mean is None and lean.var is None and np.array_equal(lean.ll, got.ll) and np.array_equal(lean.sse, got.sse)
    if case['f32']:
        wide = _score(bc, bc.RegressionHeldOut(case['Z'].astype(np.float64)), case)
        for a, b in ((wide.ll, got.ll), (wide.sse, got.sse), (wide.mean, got.mean), (wide.var, got.var)):
            assert np.array_equal(a, b)


def test_exact_zero_factor(bc):
    Z, mu, F, noise, scale = pc.exact_zero_factor()
    got = bc.linreg_predictive(bc.RegressionHeldOut(Z), mu, F, noise, scale, per_row=True)
    assert np.array_equal(got.var, np.repeat(noise[:, None], Z.shape[0], axis=1))


@pytest.mark.parametrize('d', [1, 5, 16, 17, 128, 129, 300])
def test_exact_unit_rows(bc, d):
    Z, mu, F, noise, scale, want_mean, want_var = pc.exact_unit_rows(d)
    held = bc.RegressionHeldOut(Z)
    got = bc.linreg_predictive(held, mu, F, noise, scale, per_row=True)
    assert np.array_equal(got.mean[0], want_mean) and np.array_equal(got.var[0], want_var)
    if d > 1:
        wrong = bc.linreg_predictive(held, mu, np.ascontiguousarray(F.transpose(0, 2, 1)), noise, scale, per_row=True)
        assert not np.array_equal(wrong.var[0], want_var)


def test_exact_single_row(bc):
    Z, mu, F, noise, scale, want_ll = pc.exact_single_row()
    got = bc.linreg_predictive(bc.RegressionHeldOut(Z), mu, F, noise, scale, per_row=True)
    assert got.sse[0] == 0. and got.var[0, 0] == 1. and got.mean[0, 0] == Z[0, -1] and got.ll[0] == want_ll


def test_a_non_finite_feature_gives_non_finite_sums(bc):
    case = pc.make_case('n65_d16_t17')
    Z = case['Z'].copy()
    Z[40, 3] = np.inf
    got = bc.linreg_predictive(bc.RegressionHeldOut(Z), case['mu'], case['F'], case['noise'], case['scale'])
    assert not np.any(np.isfinite(got.ll)) and not np.any(np.isfinite(got.sse))
    again = _score(bc, _held_of(bc, case), case, per_row=False)            # (and the next call is served)
    assert np.all(np.isfinite(again.ll))


# ------------------------------------------------------------------ 2. the reference's figures
@needs_longdouble
def test_predictive_against_the_reference_fixture(bc):
    g = np.load(GOLDEN)
    Z = np.hstack((g['Xt'], g['yt'][:, None]))
    nt, host_gap, std = Z.shape[0], float(g['host_gap']), float(g['output_std'])
    assert host_gap <= 1e-12
    held = bc.RegressionHeldOut(Z)
    F = np.array([np.linalg.cholesky(c) for c in g['theta_cov']])
    got = bc.linreg_predictive(held, g['theta_mean'], F, g['sigmasq'], 1., per_row=True)
    ref = pc.restate(Z, g['theta_mean'], F, g['sigmasq'], 1.)
    pc.compare(got.ll, got.sse, ref, 'device predict_f24', mean=got.mean, var=got.var)
    # the golden tolerance: the derived bound plus 8 host_gap (|golden| + 1) (a different LAPACK Cholesky on this host)
    assert np.all(np.abs(got.mean - g['pred_mean']) <= ref['tol_mean'] + 8. * host_gap * (np.abs(g['pred_mean']) + 1.))
    assert np.all(np.abs(got.var - g['pred_var']) <= ref['tol_var'] + 8. * host_gap * (np.abs(g['pred_var']) + 1.))
    nll_tol = ref['tol_ll'] / nt + 8. * host_gap * (np.abs(g['nll']) + 1.)
    print('nll', got.nll(), g['nll'], 'rmse', got.rmse(std), g['rmse'])
    assert np.all(np.abs(got.nll() - g['nll']) <= nll_tol)
    # d sqrt(x) = dx / (2 sqrt(x)): the sse tolerance carried through output_std sqrt(sse / Nt), plus the host gap
    rmse_tol = std * ref['tol_sse'] / nt / (2. * g['rmse'] / std) * 1.01 + 8. * host_gap * (g['rmse'] + 1.)
    assert np.all(np.abs(got.rmse(std) - g['rmse']) <= rmse_tol)


# ------------------------------------------------------------------ 3. batch independence, repeatability
@pytest.mark.parametrize('name', ['n65_d16_t17', 'n17_d300_t17'])
def test_a_posteriors_bits_do_not_depend_on_its_batch(bc, name):
    case = pc.make_case(name)
    held = _held_of(bc, case)
    full = _score(bc, held, case)

    def sub(sel, per_row):
        return bc.linreg_predictive(held, case['mu'][sel], case['F'][sel], case['noise'][sel], case['scale'][sel], per_row=per_row)
    for t in range(17):
        for sel in ([t], [t, (t + 5) % 17]):
            one = sub(sel, True)
            assert one.ll[0] == full.ll[t] and one.sse[0] == full.sse[t], (t, sel)
            assert np.array_equal(one.mean[0], full.mean[t]) and np.array_equal(one.var[0], full.var[t])
    rev = sub(list(range(16, -1, -1)), False)
    assert np.array_equal(rev.ll[::-1], full.ll) and np.array_equal(rev.sse[::-1], full.sse)
    again = _score(bc, held, case)
    for a, b in ((again.ll, full.ll), (again.sse, full.sse), (again.mean, full.mean), (again.var, full.var)):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------ 4. refusals
def test_refusals(bc):
    from beta_cores_amd import _native as N
    case = pc.make_case('n17_d5_t2')
    held = _held_of(bc, case)
    lib, h, z = N.load(), bc.default_context().h, held.rows().h
    nt, d, t = 17, 5, 2
    mu, F = np.ascontiguousarray(case['mu']), np.ascontiguousarray(case['F'])
    noise, scale = np.ascontiguousarray(case['noise']), np.ascontiguousarray(case['scale'])
    outs = [np.full(t, 7.), np.full(t, 7.), np.full((t, nt), 7.), np.full((t, nt), 7.)]

    def call(ctx=h, zt=z, mu=mu, F=F, noise=noise, scale=scale, t=t, ll=outs[0], sse=outs[1], mean=outs[2], var=outs[3]):
        return lib.bc_linreg_predict(ctx, zt, _p(mu), _p(F), _p(noise), _p(scale), t, _p(ll), _p(sse), _p(mean), _p(var))

    def bad(arr, at, value):
        arr = arr.copy()
        arr[at] = value
        return arr
    other_ctx = bc.Context()
    wide = bc.DeviceData(np.zeros((3, pc.MAX_DIM + 2)))
    narrow = bc.DeviceData(np.zeros((3, 1)))
    refused = [
        (dict(ctx=None), 'ctx'), (dict(zt=None), 'zt'), (dict(mu=None), 'mu'), (dict(F=None), 'factor'), (dict(noise=None), 'noise'),
        (dict(scale=None), 'scale'), (dict(ll=None), 'out_ll'), (dict(sse=None), 'out_sse'),
        (dict(mean=None), 'out_mean'), (dict(var=None), 'out_var'),
        (dict(zt=wide.h), 'columns'), (dict(zt=narrow.h), 'columns'), (dict(t=0), 't must be'),
        (dict(mu=bad(mu, (1, 3), np.nan)), 'mu of posterior 1, entry 3'), (dict(F=bad(F, (1, 2, 4), np.inf)), 'factor of posterior 1, entry 14'),
        (dict(noise=bad(noise, 1, np.nan)), 'noise[1]'), (dict(scale=bad(scale, 0, -np.inf)), 'scale[0]'),
        (dict(noise=bad(noise, 0, 0.)), 'noise[0]'), (dict(noise=bad(noise, 1, -1.)), 'noise[1]'), (dict(scale=bad(scale, 1, -1e-300)), 'scale[1]'),
        (dict(ctx=other_ctx.h), 'this context'),
    ]
    for kw, word in refused:
        assert call(**kw) == N.BC_INVALID_ARGUMENT, kw.keys()
        assert 'bc_linreg_predict' in N.last_error() and word in N.last_error(), (word, N.last_error())
        assert all(np.all(o == 7.) for o in outs), word              # a refused call writes to no output
    empty = bc.DeviceData.slot(d + 1)                                # a slot that holds no rows yet: Nt = 0
    assert call(zt=empty.h) == N.BC_INVALID_ARGUMENT and 'at least one row' in N.last_error()
    assert all(np.all(o == 7.) for o in outs)
    assert call() == N.BC_OK                                         # the call after a refusal works
    want = _score(bc, held, case)
    assert np.array_equal(outs[0], want.ll) and np.array_equal(outs[1], want.sse) and np.array_equal(outs[2], want.mean)
    assert np.array_equal(outs[3], want.var)
    with pytest.raises(ValueError, match='mu must be'):
        bc.linreg_predictive(held, mu[:, :4], F, noise, scale)
    with pytest.raises(ValueError, match='factor must be'):
        bc.linreg_predictive(held, mu, F[:1], noise, scale)
    with pytest.raises(ValueError, match='noise must be'):
        bc.linreg_predictive(held, mu, F, np.ones(3), scale)


def test_refused_while_a_sampler_run_is_open(bc):
    from beta_cores_amd import _native as N
    import hmc_many_cases as mc
    lib, h = N.load(), bc.default_context().h
    batch = mc.make_batch_case('ragged5')
    rows, w, row_ptr, start, im, eps = mc.pack(batch['problems'])
    P, c, d = start.shape
    case = pc.make_case('n17_d5_t2')
    held = _held_of(bc, case)
    ll, sse = np.full(2, 7.), np.full(2, 7.)
    args = (h, held.rows().h, _p(np.ascontiguousarray(case['mu'])), _p(np.ascontiguousarray(case['F'])), _p(np.ascontiguousarray(case['noise'])),
            _p(np.ascontiguousarray(case['scale'])), 2, _p(ll), _p(sse), None, None)
    assert lib.bc_hmc_small_begin(h, _p(rows), _p(w), _p(row_ptr), P, d, _p(start), c, _p(im), batch['L'], batch['T']) == 0
    try:
        assert lib.bc_linreg_predict(*args) == N.BC_INVALID_ARGUMENT and 'bc_hmc_small' in N.last_error()
        assert np.all(ll == 7.) and np.all(sse == 7.)
    finally:
        assert lib.bc_hmc_small_end(h) == 0
    assert lib.bc_linreg_predict(*args) == N.BC_OK and np.all(ll != 7.)


# ------------------------------------------------------------------ 5. with an encoder
def test_held_out_rows_behind_an_encoder(bc):
    rng = np.random.RandomState(3)
    nt, d0, d1 = 300, 7, 12
    raw = np.hstack((rng.randn(nt, d0), rng.randn(nt, 1))).astype(np.float32)

    def layers():
        return [(rng.randn(d1, d0) * 0.4, rng.randn(d1) * 0.1, None, None, True)]
    enc = bc.encoders.MLPEncoder(layers())
    held = bc.RegressionHeldOut(raw, encoder=enc, dtype=np.float32)
    assert held.shape == (nt, d1 + 1)
    mu, F = rng.randn(2, d1), rng.randn(2, d1, d1) * 0.2
    before = enc.launches
    a = bc.linreg_predictive(held, mu, F, 0.5, per_row=True)
    assert enc.launches == before + 1
    b = bc.linreg_predictive(held, mu, F, 0.5, per_row=True)
    assert enc.launches == before + 1                                # an unchanged version: no re-encode
    direct = bc.RegressionHeldOut(bc.DeviceData(raw, dtype=np.float32).encode(enc))      # float32 features, as DeviceProjector keeps them
    c = bc.linreg_predictive(direct, mu, F, 0.5, per_row=True)
    for x in (b, c):
        assert np.array_equal(x.ll, a.ll) and np.array_equal(x.sse, a.sse) and np.array_equal(x.mean, a.mean) and np.array_equal(x.var, a.var)
    assert held.rows().dtype == np.float32 == bc.DeviceProjector(lambda n, w, p: mu, 2, bc.likelihoods.LinearRegression(1.0), encoder=enc).encoded_dtype
    enc.update(layers())
    count = enc.launches
    e = bc.linreg_predictive(held, mu, F, 0.5, per_row=True)
    assert enc.launches == count + 1                                 # exactly one more encode launch
    assert not np.array_equal(e.ll, a.ll) and not np.array_equal(e.mean, a.mean)
    f = bc.linreg_predictive(bc.RegressionHeldOut(bc.DeviceData(raw, dtype=np.float32).encode(enc)), mu, F, 0.5, per_row=True)
    assert np.array_equal(f.ll, e.ll) and np.array_equal(f.var, e.var)
