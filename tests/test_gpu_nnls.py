"""GPU: the device NNLS refit (include/beta_cores_nnls.h) -- the refit itself against scipy.optimize.nnls, OrthoPursuit in the
fused loop (bc.snnls.DeviceOrthoPursuit) against the CPU oracle and the goldens generated from the reference, and
optimize(device=True).  Bars: identical supports, weights within 1e-5 relative, error within rtol 1e-7."""
import ctypes as C

import numpy as np
import pytest
from scipy.optimize import nnls

from conftest import load_golden
from nnls_cases import refit_cases

pytestmark = pytest.mark.gpu

WTOL = 1e-5


@pytest.fixture(scope='module')
def bc():
    import beta_cores_amd as bc
    bc.default_context()
    return bc


def seeded_phi():
    rng = np.random.RandomState(11)
    n, s_ = 30000, 100
    base = rng.randn(n, 12).dot(rng.randn(12, s_)) + 0.3 * rng.randn(n, s_)     # the recipe of test_seeded_parity_vs_oracle
    return base - base.mean(axis=1)[:, None]


@pytest.fixture(scope='module')
def seeded(bc):
    """The seeded 30000 x 100 problem, resident once; the oracle's 25 OrthoPursuit steps on it."""
    from oracle import RefOrthoPursuit
    phi = seeded_phi()
    ref = RefOrthoPursuit(phi.T, phi.sum(axis=0))
    ref.build(25)
    return dict(phi=phi, dphi=bc.DevicePhi.from_host(phi), b=phi.sum(axis=0), ref_w=ref.w.copy(), ref_err=ref.error())


def assert_matches(dev, ref_w, ref_err):
    ridx = np.where(ref_w > 0)[0]
    idx, val = dev.sparse_weights()
    np.testing.assert_array_equal(idx, ridx)
    np.testing.assert_allclose(val, ref_w[ridx], rtol=WTOL)
    np.testing.assert_allclose(dev.error(), ref_err, rtol=1e-7)


# ------------------------------------------------------------------ 1. the refit against SciPy, step-wise
CASES = list(refit_cases())


@pytest.mark.parametrize('k', range(len(CASES)), ids=['S%d_n%d' % (c[0], c[1]) for c in CASES])
def test_refit_matches_scipy(bc, k):
    S, n, cols, b, val = CASES[k]
    s = bc.snnls.FrankWolfe(cols.T, b)                     # any algorithm's list: the rows of a small Phi are the columns
    eng = s._eng
    eng.set_sparse_weights(np.arange(n), val)              # about half of the start weights are zero
    eng.refit(-1)
    idx, x = eng.sparse_weights()
    dcols = eng.columns()
    assert np.array_equal(idx, np.arange(n)) and np.array_equal(dcols, cols)
    ref = nnls(cols.T, b)[0]
    print('case', S, n, 'support', int((ref > 0).sum()), 'worst rel', np.abs(x[ref > 0] / ref[ref > 0] - 1).max() if (ref > 0).any() else 0.)
    assert np.array_equal(x > 0, ref > 0)
    np.testing.assert_allclose(x, ref, rtol=WTOL, atol=0)
    # KKT from the downloaded columns
    r = b - x.dot(dcols)
    d = dcols.dot(r) / (np.sqrt((dcols ** 2).sum(axis=1)) * np.sqrt((b ** 2).sum()))
    sup = x > 0
    assert np.all(x >= 0)
    assert np.all(np.abs(d[sup]) <= 1e-10) and np.all(d[~sup] <= 1e-10)
    np.testing.assert_allclose(eng.error(), np.sqrt((r ** 2).sum()), rtol=1e-9, atol=1e-12 * np.sqrt((b ** 2).sum()))
    assert eng.size() == int(sup.sum())


# ------------------------------------------------------------------ 2. the OMP loop against the oracle and the goldens
def test_seeded_parity_vs_oracle(bc, seeded):
    dev = bc.snnls.DeviceOrthoPursuit(seeded['dphi'].T, seeded['b'])
    assert dev._use_fused()
    dev.build(25)
    assert_matches(dev, seeded['ref_w'], seeded['ref_err'])
    refits, solves, rejected = dev._eng.refit_stats()
    print('refits', refits, 'solves', solves, 'rejected', rejected)
    assert refits == 25 and solves <= 3 * refits           # warm-started: the model needs 2 per refit


@pytest.mark.parametrize('nm', ['ll', 'bl'])
def test_f3_golden_and_optimize(bc, nm):
    g = load_golden('f3_hilbert_linreg')
    phi = g['phi_' + nm]
    key = '%s_omp_' % nm
    steps = g[key + 'sel'].shape[0]
    s = bc.snnls.DeviceOrthoPursuit(phi.T, phi.sum(axis=0))
    s.build(steps)
    idx, val = s.sparse_weights()
    np.testing.assert_array_equal(idx, g[key + 'idcs'])
    np.testing.assert_allclose(val, g[key + 'wts'], rtol=WTOL)
    np.testing.assert_allclose(s.error(), g[key + 'err'][-1], rtol=1e-7)
    f, st, er = s._eng.trace()
    np.testing.assert_allclose(er, g[key + 'err'], rtol=1e-7)
    s.optimize()
    idx, val = s.sparse_weights()
    np.testing.assert_array_equal(idx, g[key + 'opt_idcs'])
    np.testing.assert_allclose(val, g[key + 'opt_wts'], rtol=WTOL)
    assert not s.reached_numeric_limit


F1 = load_golden('f1_snnls')
EXACT = [c for c in F1['cases'] if c.startswith('gauss_N') or c.startswith('axis_aligned')]
DEGENERATE = [c for c in F1['cases'] if c not in EXACT]


@pytest.mark.parametrize('case', EXACT)
@pytest.mark.parametrize('fused', [True, False])
def test_f1_exact_sequences(bc, case, fused):
    X = F1[case + '_X']
    Wg, eg, lg = F1['%s_omp_W' % case], F1['%s_omp_err' % case], F1['%s_omp_lim' % case]
    steps = Wg.shape[0]
    s = bc.snnls.DeviceOrthoPursuit(X.T, X.sum(axis=0))
    scale = np.sqrt((X.sum(axis=0) ** 2).sum())
    W = np.zeros((steps, s.n_total))
    err = np.zeros(steps)
    for m in range(steps):
        if fused:
            s.build(1)
        elif not s.reached_numeric_limit:
            s.build_stepwise(1)
        W[m] = s.weights()
        err[m] = s.error()
    # compare while the reference is in its well-conditioned regime (error above rounding noise)
    for m in range(steps):
        if eg[m] < 1e-9 * scale or lg[m]:
            break
        assert np.array_equal(W[m] > 0, Wg[m] > 0), 'support differs at step %d' % m
        np.testing.assert_allclose(W[m], Wg[m], rtol=WTOL, atol=1e-12)
        np.testing.assert_allclose(err[m], eg[m], rtol=1e-6, atol=1e-9 * scale)
    assert np.all(W >= 0)


@pytest.mark.parametrize('case', DEGENERATE)
def test_f1_degenerate_invariants(bc, case):
    X = F1[case + '_X']
    steps = F1['%s_omp_W' % case].shape[0]
    s = bc.snnls.DeviceOrthoPursuit(X.T, X.sum(axis=0))
    xs = X.sum(axis=0)
    prev = np.inf
    for m in range(1, steps + 1):
        s.build(1)
        w = s.weights()
        assert (w > 0).sum() <= m and (w > 0).sum() == s.size() and np.all(w >= 0)
        e = np.sqrt((((w[:, None] * X).sum(axis=0) - xs) ** 2).sum())
        assert e - prev < 1e-6
        assert abs(s.error() - e) < 1e-6
        prev = e
    s.reset()
    assert s.size() == 0 and not s.reached_numeric_limit and abs(s.error() - np.sqrt((xs ** 2).sum())) < 1e-9


@pytest.mark.parametrize('n,s_', [(129, 7), (1000, 33), (3000, 257)])
def test_dense_phi_vs_oracle(bc, n, s_):
    from oracle import RefOrthoPursuit
    phi = np.random.RandomState(n + s_).randn(n, s_)
    steps = min(s_ - 1, 60)
    ref = RefOrthoPursuit(phi.T, phi.sum(axis=0))
    ref.build(steps)
    dev = bc.snnls.DeviceOrthoPursuit(phi.T, phi.sum(axis=0))
    dev.build(steps)
    assert dev._eng.finish_form() == 5          # BC_FINISH_OMP: k_step_finish<BC_ALG_OMP> served the fused loop
    assert_matches(dev, ref.w, ref.error())


# ------------------------------------------------------------------ 3. one path, one result
def test_one_shot_incremental_and_stepwise_are_bit_equal(bc):
    phi = np.random.RandomState(5).randn(5000, 40)
    d = bc.DevicePhi.from_host(phi)
    b = phi.sum(axis=0)
    k = 20
    a = bc.snnls.DeviceOrthoPursuit(d.T, b)
    a.build(k)
    again = bc.snnls.DeviceOrthoPursuit(d.T, b)
    again.build(k)
    inc = bc.snnls.DeviceOrthoPursuit(d.T, b)
    for _ in range(k):
        inc.build(1)
    stp = bc.snnls.DeviceOrthoPursuit(d.T, b)
    stp.build_stepwise(k)
    ia, va = a.sparse_weights()
    assert len(ia) > 10
    for other in (again, inc, stp):
        io, vo = other.sparse_weights()
        assert np.array_equal(ia, io) and np.array_equal(va, vo)
        assert other.error() == a.error()


def test_record_route_behind_the_prefilter(bc, monkeypatch):
    rng = np.random.RandomState(8)
    phi = rng.randn(200000, 6).dot(rng.randn(6, 24)) + 0.3 * rng.randn(200000, 24)
    d = bc.DevicePhi.from_host(phi)
    b = phi.sum(axis=0)
    res = []
    for form in ('8', '0'):
        monkeypatch.setenv('BC_PREFILTER', form)
        s = bc.snnls.DeviceOrthoPursuit(d.T, b)
        assert s._eng.prefilter == int(form)
        s.build(15)
        res.append(s.sparse_weights() + (s.error(),))
    assert len(res[0][0]) > 5
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]) and res[0][2] == res[1][2]


# ------------------------------------------------------------------ 4. optimize(device=True) on GIGA and FrankWolfe
@pytest.mark.parametrize('alg', ['GIGA', 'FrankWolfe'])
def test_optimize_device_matches_host(bc, seeded, alg):
    cls = getattr(bc.snnls, alg)
    host = cls(seeded['dphi'].T, seeded['b'])
    dev = cls(seeded['dphi'].T, seeded['b'])
    host.build(40)
    dev.build(40)
    host.optimize()
    dev.optimize(device=True)
    ih, vh = host.sparse_weights()
    idv, vd = dev.sparse_weights()
    np.testing.assert_array_equal(idv, ih)
    np.testing.assert_allclose(vd, vh, rtol=WTOL)
    print(alg, 'error host', host.error(), 'device', dev.error())
    assert dev.error() <= host.error() * (1. + 1e-7)
    assert host.reached_numeric_limit == dev.reached_numeric_limit


@pytest.mark.parametrize('alg', ['GIGA', 'FrankWolfe'])
def test_optimize_at_rounding_level_error(bc, alg):
    X = F1['gauss_N10_D3_X']
    cls = getattr(bc.snnls, alg)
    for device in (False, True):
        s = cls(X.T, X.sum(axis=0))
        s.build(30)
        s.optimize(device=device)                          # neither path may raise
        assert np.all(s.weights() >= 0)


# ------------------------------------------------------------------ 5. limits and conventions
def test_list_limit(bc):
    rng = np.random.RandomState(7)
    phi = rng.randn(300, 150)
    s = bc.snnls.GIGA(phi.T, phi.sum(axis=0))
    val = np.abs(rng.randn(129)) + 0.1
    s._eng.set_sparse_weights(np.arange(128), val[:128])
    s._eng.refit(-1)                                       # 128 columns refit
    ref = nnls(phi[:128].T, phi.sum(axis=0))[0]
    idx, x = s._eng.sparse_weights()
    assert np.array_equal(x > 0, ref > 0)
    np.testing.assert_allclose(x, ref, rtol=WTOL, atol=0)
    s._eng.set_sparse_weights(np.arange(129), val)
    for call in (lambda: s._eng.refit(-1), lambda: s._eng.refit(200), lambda: s._eng.optimize_device()):
        with pytest.raises(ValueError, match='128'):
            call()
        idx, x = s._eng.sparse_weights()
        assert np.array_equal(idx, np.arange(129)) and np.array_equal(x, val)      # untouched


def test_build_past_the_limit_consumes_nothing(bc):
    phi = np.random.RandomState(9).randn(400, 140)
    s = bc.snnls.DeviceOrthoPursuit(phi.T, phi.sum(axis=0))
    s.build(5)
    w0 = s.weights()
    n0 = len(s._eng.trace()[0])
    assert n0 == 5
    with pytest.raises(ValueError, match='128'):
        s.build(124)                                       # 5 listed + 124 could reach 129
    assert len(s._eng.trace()[0]) == n0 and np.array_equal(s.weights(), w0) and not s.reached_numeric_limit
    s.build(3)
    assert len(s._eng.trace()[0]) == n0 + 3


def test_conventions(bc):
    from beta_cores_amd import _native as N

    class World2:
        world, rank = 2, 0
    phi = np.random.RandomState(1).randn(50, 5)
    with pytest.raises(ValueError, match='single-rank'):
        bc.snnls.DeviceOrthoPursuit(phi.T, phi.sum(axis=0), comm=World2())
    plain = bc.snnls.OrthoPursuit(phi.T, phi.sum(axis=0))
    assert not plain._use_fused()                          # still the step-wise route with the host refit
    lim = C.c_int()
    lib = N.load()
    assert lib.bc_snnls_build(plain._eng.h, 1, C.byref(lim)) == N.BC_INVALID_ARGUMENT
    assert b'OrthoPursuit' in lib.bc_last_error()
    assert lib.bc_snnls_reweight(plain._eng.h, 3) == N.BC_INVALID_ARGUMENT
    dev = bc.snnls.DeviceOrthoPursuit(phi.T, phi.sum(axis=0))
    assert lib.bc_snnls_reweight(dev._eng.h, 3) == N.BC_INVALID_ARGUMENT          # the closed-form reweight keeps refusing OMP
    dev._eng.enable_device_refit(False)                    # opting out restores the refusal
    assert lib.bc_snnls_build(dev._eng.h, 1, C.byref(lim)) == N.BC_INVALID_ARGUMENT
    plain.build(3)
    dev._eng.enable_device_refit(True)
    dev.build(3)
    ip, vp = plain.sparse_weights()
    idv, vd = dev.sparse_weights()
    np.testing.assert_array_equal(idv, ip)
    np.testing.assert_allclose(vd, vp, rtol=WTOL)


def test_hilbert_coreset_accepts_the_class(bc):
    rng = np.random.RandomState(0)
    X = rng.randn(2000, 8)
    Z = np.hstack((X, (X.dot(rng.randn(8)) + rng.randn(2000))[:, None]))
    th = rng.randn(40, 8) * 0.2
    prj = bc.DeviceProjector(lambda n, w, p: th, 40, bc.likelihoods.LinearRegression(1.0))
    res = []
    for cls in (bc.snnls.OrthoPursuit, bc.snnls.DeviceOrthoPursuit):
        h = bc.HilbertCoreset(Z, prj, snnls=cls)
        h.build(12, 12)
        res.append(h.get())
    np.testing.assert_array_equal(res[0][2], res[1][2])
    np.testing.assert_allclose(res[0][0], res[1][0], rtol=WTOL)


# ------------------------------------------------------------------ 6. lists that grow outside the OMP kernels
@pytest.mark.parametrize('alg', ['GIGA', 'FrankWolfe'])
def test_build_optimize_build_optimize(bc, seeded, alg):
    """The closed-form steps of GIGA / FrankWolfe append columns without a refit: the Gram state has to follow them.  build,
    optimize, build, optimize -- and once more after a reset -- on the device against the same sequence with the host optimize."""
    cls = getattr(bc.snnls, alg)
    host = cls(seeded['dphi'].T, seeded['b'])
    dev = cls(seeded['dphi'].T, seeded['b'])
    for rnd, steps in enumerate((30, 10, 15)):
        for s, device in ((host, False), (dev, True)):
            s.build(steps)
            s.optimize(device=device)
            assert not s.reached_numeric_limit, (rnd, device)
        ih, vh = host.sparse_weights()
        idv, vd = dev.sparse_weights()
        np.testing.assert_array_equal(idv, ih)
        np.testing.assert_allclose(vd, vh, rtol=WTOL)
        assert dev.error() <= host.error() * (1. + 1e-7)
    n_before = len(dev.sparse_weights()[0])
    for s, device in ((host, False), (dev, True)):
        s.reset()
        s.build(8)
        s.optimize(device=device)
    ih, vh = host.sparse_weights()
    idv, vd = dev.sparse_weights()
    assert len(idv) < n_before
    np.testing.assert_array_equal(idv, ih)
    np.testing.assert_allclose(vd, vh, rtol=WTOL)


def test_refit_column_on_a_giga_list(bc, seeded):
    """bc_snnls_refit(f) on a list GIGA built, after an earlier refit: orthopursuit.py:37-41 over its positive entries plus f."""
    s = bc.snnls.GIGA(seeded['dphi'].T, seeded['b'])
    s.build(12)
    s._eng.refit(-1)
    s.build(6)
    idx, val = s._eng.sparse_weights()
    cols = s._eng.columns()
    f = 4321
    assert f not in idx
    act = val > 0
    A = np.vstack((cols[act], seeded['phi'][f][None, :]))
    ref = nnls(A.T, seeded['b'])[0]
    s._eng.refit(f)
    idx2, val2 = s._eng.sparse_weights()
    got = np.array([val2[np.flatnonzero(idx2 == i)[0]] for i in list(idx[act]) + [f]])
    assert np.array_equal(got > 0, ref > 0)
    np.testing.assert_allclose(got, ref, rtol=WTOL, atol=0)
    assert np.all(val2[~np.isin(idx2, list(idx[act]) + [f])] == 0.)


def test_refused_refit_leaves_the_gram_state_alone(bc):
    """128 entries put there from the host, a refit of one more column is refused by the kernel, and the refit of the list that
    follows still computes its Gram state."""
    rng = np.random.RandomState(7)
    phi = rng.randn(300, 150)
    b = phi.sum(axis=0)
    s = bc.snnls.GIGA(phi.T, b)
    val = np.abs(rng.randn(128)) + 0.1
    s._eng.set_sparse_weights(np.arange(128), val)
    with pytest.raises(ValueError, match='128'):
        s._eng.refit(200)
    idx, x = s._eng.sparse_weights()
    assert np.array_equal(idx, np.arange(128)) and np.array_equal(x, val)
    s._eng.refit(5)                                        # listed already: no new slot needed
    s._eng.set_sparse_weights(np.arange(128), val)
    with pytest.raises(ValueError, match='128'):
        s._eng.refit(200)
    s._eng.refit(-1)
    ref = nnls(phi[:128].T, b)[0]
    idx, x = s._eng.sparse_weights()
    assert np.array_equal(x > 0, ref > 0)
    np.testing.assert_allclose(x, ref, rtol=WTOL, atol=0)
