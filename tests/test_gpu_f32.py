"""float32 data rows on the GPU (include/beta_cores_f32.h, DeviceData(dtype=np.float32)).

Only the STORAGE is float32: every kernel widens the rows in registers, which is exact, and computes in float64.  So for
float32 input Z32 every result must have THE SAME BITS as the existing float64 path gives on Z32.astype(np.float64):
np.array_equal throughout, no tolerances (one exception, stated where it is used: the float64 K4 takes another kernel by
default, and the bound between the two K4 kernels is the one tests/test_gpu_gram.py already uses)."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FLT_MAX = float(np.finfo(np.float32).max)


@pytest.fixture(scope='module')
def bc():
    import beta_cores_amd as bc
    bc.default_context()
    return bc


@contextlib.contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update({k: str(v) for k, v in kw.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def fixed(th):
    return lambda n, w, p: th


def models(bc, rng, dz):
    """(name, model, d, [(model id, params)...]) of the three families for rows of dz columns: all seven model ids."""
    out = []
    if dz >= 2:
        m = bc.likelihoods.LinearRegression(1.3)
        out.append(('linreg', m, dz - 1, [(m.model_id, m.params()), (m.beta_model_id, m.params(beta=0.3))]))
    m = bc.likelihoods.LogisticRegression()
    out.append(('logistic', m, dz, [(m.model_id, m.params()), (m.beta_model_id, m.params(beta=0.2))]))
    Sig = np.diag(rng.uniform(0.5, 2.0, dz))
    m = bc.likelihoods.GaussianLocation(np.linalg.inv(Sig), np.linalg.slogdet(Sig)[1])
    out.append(('gauss', m, dz, [(m.model_id, m.params()), (m.beta_model_id, m.params(beta=0.5)),
                                 (m.beta_grad_model_id, m.params(beta=0.5))]))
    return out


def rows32(rng, n, dz, d, special=True):
    """float32 rows with the values a widening load could get wrong: subnormals, +-0, magnitudes near FLT_MAX, an
    all-zero-feature row (the constant-row path), and rows whose |z . theta| passes 100 (the logistic branches)."""
    Z = rng.randn(n, dz).astype(np.float32)
    if not special:
        return Z
    tiny = np.float32(1e-41)                                    # a float32 subnormal
    assert 0. < tiny < np.finfo(np.float32).tiny
    r = lambda: rng.randint(n)
    c = lambda: rng.randint(dz)
    for _ in range(3):
        Z[r(), c()] = tiny
        Z[r(), c()] = -tiny
        Z[r(), c()] = np.float32(1.4e-45)                       # the smallest one
        Z[r(), c()] = np.float32(-0.)
        Z[r(), c()] = np.float32(0.)
    Z[r(), c()] = np.float32(0.9 * FLT_MAX)
    Z[r(), c()] = np.float32(-0.9 * FLT_MAX)
    Z[r(), :] = np.float32(300.) * np.sign(Z[r(), :] + np.float32(1e-3))      # |m| > 100 for the logistic models
    if n > 4:
        Z[r(), :d] = 0.                                         # a constant row (with its y, where the model has one)
    return Z


def project_all(bc, prj, dd, ids, want_colsum=True):
    """Everything K1 produces for each (model id, params): Phi, norms, column sums, store-free column sums, norm statistics."""
    from beta_cores_amd import _native as N
    from beta_cores_amd.device import _ptr
    out = []
    theta = prj.model.theta_for_device(prj.samples)
    S = int(theta.shape[0])
    for mid, params in ids:
        phi = prj._run(dd, mid, params)
        rec = [phi.to_host(), phi.norms(), phi.colsum(), phi.norm_stats()]
        if want_colsum and S <= 256:
            params = np.ascontiguousarray(params, dtype=np.float64)
            sf = np.empty(S)
            N.call('bc_project_colsum', prj.ctx.h, dd.h, int(mid), _ptr(theta), S, _ptr(params), int(params.shape[0]), None, _ptr(sf))
            rec.append(sf)
        out.append(rec)
        del phi
    return out


def assert_same(got, want, what, equal_nan=False):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        for i, (x, y) in enumerate(zip(a, b)):
            if isinstance(x, tuple):
                ok = x[0] == y[0] and (x[1] == y[1] or (equal_nan and x[1] != x[1] and y[1] != y[1]))
            else:
                ok = np.array_equal(x, y, equal_nan=equal_nan)
            assert ok, '%s: model #%d, result #%d (0 Phi, 1 norms, 2 colsum, 3 norm stats, 4 store-free colsum) differs' % (what, k, i)


# ------------------------------------------------------------------ K1
@pytest.mark.parametrize('n,dz,s', [(1, 3, 5), (127, 7, 16), (129, 33, 97), (5000, 129, 100), (129, 7, 112), (127, 33, 300),
                                    (5000, 3, 100), (129, 129, 16), (1, 129, 100), (127, 3, 300), (129, 17, 200), (127, 9, 256)])
def test_k1_is_bit_identical_on_float32_rows(bc, n, dz, s):
    """All seven model ids, odd row widths, ragged row counts, every sample-tile variant of the staged kernel and the
    multi-pass mode of S > 256: float32 rows against the same rows widened on the host."""
    rng = np.random.RandomState(1000 * n + 10 * dz + s)
    for name, model, d, ids in models(bc, rng, dz):
        Z32 = rows32(rng, n, dz, d)
        th = rng.randn(s, d) * 0.4
        prj = bc.DeviceBetaProjector(fixed(th), s, model)
        d32 = bc.DeviceData(Z32, dtype=np.float32)
        d64 = bc.DeviceData(Z32.astype(np.float64))
        assert d32.dtype == np.float32 and d32.nbytes == 4 * n * dz and d64.dtype == np.float64 and d64.nbytes == 8 * n * dz
        want = project_all(bc, prj, d64, ids)
        for rec in want:
            assert not np.isnan(rec[0]).any(), 'the reference of this case is meant to be NaN-free'
        assert_same(project_all(bc, prj, d32, ids), want, '%s n=%d dz=%d S=%d' % (name, n, dz, s))


def test_k1_nan_and_inf_rows(bc):
    rng = np.random.RandomState(5)
    n, dz, s = 300, 9, 48
    for name, model, d, ids in models(bc, rng, dz):
        Z32 = rows32(rng, n, dz, d)
        Z32[17, 2] = np.nan
        Z32[130, :] = np.inf
        Z32[131, 0] = -np.inf
        th = rng.randn(s, d) * 0.4
        prj = bc.DeviceBetaProjector(fixed(th), s, model)
        want = project_all(bc, prj, bc.DeviceData(Z32.astype(np.float64)), ids)
        got = project_all(bc, prj, bc.DeviceData(Z32, dtype=np.float32), ids)
        assert_same(got, want, name, equal_nan=True)


@pytest.mark.parametrize('staged', [False, True])
def test_k1_large_shard_both_kernels(bc, staged):
    """At least 8 tiles per wave slot (262 144 rows on 256 CUs), S = 100, D = 128: the Theta-resident kernel reads float32 rows
    with one 16-byte load per row and stage; BC_K1_STAGED=1 runs the staged kernel at the same shape."""
    rng = np.random.RandomState(77)
    n, d, s = 262_144 + 77, 128, 100
    fam = {nm: (model, dd, ids) for nm, model, dd, ids in models(bc, rng, d + 1)[:1] + models(bc, rng, d)[-2:]}
    with env(BC_K1_STAGED='1' if staged else '0'):
        for name, (model, dcols, ids) in fam.items():
            dz = dcols + (1 if name == 'linreg' else 0)
            Z32 = rows32(rng, n, dz, dcols)
            Z32[n - 1, :dcols] = 0.                              # a constant row in the ragged last group
            th = rng.randn(s, dcols) * (0.6 / np.sqrt(dcols))
            prj = bc.DeviceBetaProjector(fixed(th), s, model)
            ids = ids[:2]
            want = project_all(bc, prj, bc.DeviceData(Z32.astype(np.float64)), ids)
            got = project_all(bc, prj, bc.DeviceData(Z32, dtype=np.float32), ids)
            assert_same(got, want, '%s staged=%s' % (name, staged))


def test_k1_resident_kernel_odd_width(bc):
    """The resident kernel where a row is not a multiple of 16 bytes and D not a multiple of 32: the 16-byte loads of the last
    stage straddle the row's end (the y column, the next row, the end of the group's range)."""
    rng = np.random.RandomState(78)
    n, s = 262_144 + 33, 16
    for dz in (7, 33):
        for name, model, d, ids in models(bc, rng, dz)[:2]:
            Z32 = rows32(rng, n, dz, d)
            th = rng.randn(s, d) * 0.4
            prj = bc.DeviceBetaProjector(fixed(th), s, model)
            want = project_all(bc, prj, bc.DeviceData(Z32.astype(np.float64)), ids[:1])
            got = project_all(bc, prj, bc.DeviceData(Z32, dtype=np.float32), ids[:1])
            assert_same(got, want, '%s dz=%d' % (name, dz))


# ------------------------------------------------------------------ host route
@pytest.mark.parametrize('chunk', [0, 65536])
def test_host_route_uploads_float32_as_it_is(bc, chunk, monkeypatch):
    from beta_cores_amd import device
    from beta_cores_amd.coreset import projector as P
    rng = np.random.RandomState(3)
    n, d, s = P._PIPE_ROWS + 70001, 20, 64
    model = bc.likelihoods.LinearRegression(0.7)
    Z32 = rows32(rng, n, d + 1, d)
    th = rng.randn(s, d) * 0.3
    prj = bc.DeviceProjector(fixed(th), s, model)
    res64 = prj.project(bc.DeviceData(Z32.astype(np.float64)))
    want = (res64.to_host(), res64.norms(), res64.colsum())
    del res64
    res32 = prj.project(bc.DeviceData(Z32, dtype=np.float32))
    assert all(np.array_equal(a, b) for a, b in zip((res32.to_host(), res32.norms(), res32.colsum()), want))
    del res32

    def no_f64_copy(a, what):
        raise AssertionError('a float64 host copy of a float32 array was asked for')
    monkeypatch.setattr(device, '_as_f64', no_f64_copy)      # the one place host rows are widened
    with env(**({'BC_PIPE_CHUNK_ROWS': chunk} if chunk else {})):
        got = prj.project(Z32)                                       # a live float32 ndarray of >= _PIPE_ROWS rows
        assert all(np.array_equal(a, b) for a, b in zip((got.to_host(), got.norms(), got.colsum()), want))
        phi, dd = prj._run_from_host(Z32, model.model_id, model.params())
    assert dd.dtype == np.float32 and dd.nbytes == 4 * n * (d + 1) and dd.shape == (n, d + 1)
    assert np.array_equal(phi.colsum(), want[2])
    idx = np.array([0, 1, n - 1, 65535, 65536])
    assert np.array_equal(dd.rows(idx), Z32[idx].astype(np.float64))
    # a live array between _SMALL_ROWS and _PIPE_ROWS rows, and a pinned one, stay float32 on the device too
    mid = Z32[:P._SMALL_ROWS + 5].copy()
    dmid, transient = prj.device_data(mid)
    assert dmid.dtype == np.float32 and not transient
    pinned = prj.pin(mid)
    assert pinned.dtype == np.float32 and pinned.nbytes == mid.nbytes
    prj.unpin(mid)
    monkeypatch.undo()
    small, transient = prj.device_data(Z32[:100].astype(np.float64))
    assert small.dtype == np.float64 and transient


def test_default_dtype_keeps_widening(bc):
    Z32 = np.random.RandomState(0).randn(50, 4).astype(np.float32)
    dd = bc.DeviceData(Z32)
    assert dd.dtype == np.float64 and dd.nbytes == 8 * Z32.size
    assert np.array_equal(dd.rows(np.arange(50)), Z32.astype(np.float64))


# ------------------------------------------------------------------ shards, torch, gather
def test_float32_shard_keeps_global_indices(bc):
    rng = np.random.RandomState(8)
    n, d, s = 9000, 12, 64
    lo, hi = 1001, 8003                                              # lo is not a multiple of 128
    Z32 = rows32(rng, n, d + 1, d, special=False)
    th = rng.randn(s, d) * 0.3
    prj = bc.DeviceProjector(fixed(th), s, bc.likelihoods.LinearRegression(1.0))
    traces = []
    phis = []
    for dd in (bc.DeviceData(Z32[lo:hi], dtype=np.float32, row_offset=lo), bc.DeviceData(Z32[lo:hi].astype(np.float64), row_offset=lo)):
        phi = prj.project(dd)
        assert phi.row_offset == lo
        phis.append(phi.to_host())
        alg = bc.snnls.GIGA(phi.T, phi.colsum())
        alg.build(30)
        traces.append(alg._eng.trace())
    assert np.array_equal(phis[0], phis[1])
    assert len(traces[0][0]) == 30 and traces[0][0].min() >= lo and traces[0][0].max() < hi
    for a, b in zip(traces[0], traces[1]):
        assert np.array_equal(a, b)


def test_from_torch_borrows_float32(bc):
    import torch
    rng = np.random.RandomState(9)
    n, d, s = 5000, 16, 32
    Z32 = rows32(rng, n, d + 1, d)
    t = torch.from_numpy(Z32).cuda()
    ptr = t.data_ptr()
    dd = bc.DeviceData.from_torch(t)
    assert dd.dtype == np.float32 and dd.nbytes == 4 * n * (d + 1) and t.data_ptr() == ptr and dd._keep is t
    th = rng.randn(s, d) * 0.3
    prj = bc.DeviceProjector(fixed(th), s, bc.likelihoods.LinearRegression(1.0))
    want = prj.project(bc.DeviceData(Z32.astype(np.float64))).to_host()
    assert np.array_equal(prj.project(dd).to_host(), want)
    assert np.array_equal(t.cpu().numpy(), Z32)                      # borrowed, not written
    t64 = torch.from_numpy(Z32.astype(np.float64)).cuda()
    assert bc.DeviceData.from_torch(t64).dtype == np.float64
    with pytest.raises(AssertionError):
        bc.DeviceData.from_torch(t.half())


def test_rows_are_gathered_as_float64(bc):
    rng = np.random.RandomState(10)
    Z32 = rows32(rng, 700, 9, 8)
    dd = bc.DeviceData(Z32, dtype=np.float32)
    idx = np.array([699, 0, 5, 5, 128, 127])
    got = dd.rows(idx)
    assert got.dtype == np.float64 and np.array_equal(got, Z32[idx].astype(np.float64))
    assert np.array_equal(np.signbit(got), np.signbit(Z32[idx]))     # -0 stays -0
    assert np.array_equal(dd[3], Z32[3].astype(np.float64))


def test_zero_feature_keys_of_float32_rows(bc):
    """The scan that finds the constant rows (bc_data_zero_feature_keys) on float32 rows, and its host twin on a float32 array."""
    from beta_cores_amd.coreset import projector as P
    rng = np.random.RandomState(14)
    n, d = P._SMALL_ROWS + 300, 6
    Z32 = rows32(rng, n, d + 1, d, special=False)
    zero = rng.choice(n, 40, replace=False)
    Z32[zero, :d] = 0.
    Z32[zero[:5], 0] = np.float32(-0.)                               # -0 features count as zero
    Z32[zero[5], d] = np.float32(1e-41)                              # a subnormal y is a key of its own
    Z32[zero[6], 1] = np.float32(1.4e-45)                            # a subnormal feature is NOT zero
    prj = bc.DeviceBetaProjector(fixed(rng.randn(8, d)), 8, bc.likelihoods.LinearRegression(1.0))
    want = np.unique(Z32[np.setdiff1d(zero, zero[6:7]), d].astype(np.float64))
    assert np.array_equal(prj._zero_feature_keys(bc.DeviceData(Z32, dtype=np.float32), d), want)
    assert np.array_equal(prj._zero_feature_keys(bc.DeviceData(Z32.astype(np.float64)), d), want)
    assert np.array_equal(prj._zero_feature_keys(Z32, d), want)


# ------------------------------------------------------------------ end to end
def _linreg_problem(rng, n, d):
    X = rng.randn(n, d)
    y = X.dot(rng.randn(d)) + rng.randn(n)
    return np.hstack((X, y[:, None])).astype(np.float32)


def test_hilbert_coreset_end_to_end(bc):
    rng = np.random.RandomState(11)
    n, d, s = 70000, 10, 64                                          # >= _PIPE_ROWS: the ndarray goes through the host route
    Z32 = _linreg_problem(rng, n, d)
    th = rng.randn(s, d) * 0.2
    res = []
    for Z in (Z32, Z32.astype(np.float64), bc.DeviceData(Z32, dtype=np.float32)):
        np.random.seed(5)
        alg = bc.HilbertCoreset(Z, bc.DeviceProjector(fixed(th), s, bc.likelihoods.LinearRegression(1.0)), snnls=bc.snnls.GIGA)
        alg.build(40, 40)
        res.append((alg.idcs, alg.wts, np.asarray(alg.pts, dtype=np.float64), alg.error(), np.random.rand()))
    for other in res[1:]:
        assert np.array_equal(res[0][0], other[0]) and np.array_equal(res[0][1], other[1]) and np.array_equal(res[0][2], other[2])
        assert res[0][3] == other[3] and res[0][4] == other[4]


@pytest.mark.parametrize('fused', [True, False])
def test_beta_coreset_linreg_end_to_end(bc, fused):
    rng = np.random.RandomState(12)
    n, d, s = 6000, 8, 48
    Z32 = _linreg_problem(rng, n, d)
    res = []
    for Z in (Z32, Z32.astype(np.float64)):
        np.random.seed(6)
        sampler = bc.samplers.LinregPosteriorSampler(np.zeros(d), np.eye(d), 1.0, rng=np.random.RandomState(4))
        alg = bc.BetaCoreset(Z, bc.DeviceBetaProjector(sampler, s, bc.likelihoods.LinearRegression(1.0)), opt_itrs=6,
                             step_sched=lambda i: 0.1 / (1. + i), beta=0.1, learn_beta=False, fused_gradient=fused)
        if Z.dtype == np.float32:
            assert alg._dev_data.dtype == np.float32                 # the pinned copy of a float32 array is float32
        steps = []
        for m in (1, 2, 3, 4):
            alg.build(1, m)
            steps.append((alg.idcs.copy(), alg.wts.copy(), np.asarray(alg.pts, dtype=np.float64).copy(), alg.error()))
        res.append((steps, np.random.rand()))
    for a, b in zip(res[0][0], res[1][0]):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]
    assert res[0][1] == res[1][1]


def test_beta_coreset_logistic_end_to_end(bc):
    rng = np.random.RandomState(13)
    n, d, s = 5000, 6, 37
    X = rng.randn(n, d)
    y = np.where(rng.rand(n) < 1. / (1. + np.exp(-X.dot(rng.randn(d)))), 1., -1.)
    Z32 = (y[:, None] * X).astype(np.float32)
    res = []
    for Z in (Z32, Z32.astype(np.float64)):
        np.random.seed(7)
        sampler = bc.samplers.LogisticLaplaceSampler(np.zeros(d), solver='newton', rng=np.random.RandomState(3))
        alg = bc.BetaCoreset(Z, bc.DeviceBetaProjector(sampler, s, bc.likelihoods.LogisticRegression()), opt_itrs=5,
                             step_sched=lambda i: 0.5 / (1. + i), beta=0.1, learn_beta=False)
        steps = []
        for m in (1, 2, 3):
            alg.build(1, m)
            steps.append((alg.idcs.copy(), alg.wts.copy(), np.asarray(alg.pts, dtype=np.float64).copy(), alg.error()))
        res.append((steps, np.random.rand()))
    for a, b in zip(res[0][0], res[1][0]):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]
    assert res[0][1] == res[1][1]


# ------------------------------------------------------------------ K4
@pytest.mark.parametrize('d', [7, 64, 127, 128, 200, 512])
def test_k4_weighted_gram(bc, d):
    rng = np.random.RandomState(d)
    n = 20011
    Z32 = rows32(rng, n, d + 1, d, special=False)
    Z32[5, 3] = np.float32(1e-41)
    Z32[6, 0] = np.float32(-0.)
    d32 = bc.DeviceData(Z32, dtype=np.float32)
    d64 = bc.DeviceData(Z32.astype(np.float64))
    for w in (None, rng.rand(n)):
        G32, v32 = bc.weighted_gram(d32, w)
        with env(BC_GRAM_DMA=0):                                     # the register-staged kernel, the one float32 rows take
            G64, v64 = bc.weighted_gram(d64, w)
        assert np.array_equal(G32, G64) and np.array_equal(v32, v64)
        # the float64 default (k_gram_dma at D = 127 / 128 unweighted): the bound tests/test_gpu_gram.py uses between the two kernels
        Gd, vd = bc.weighted_gram(d64, w)
        assert np.abs(G32 - Gd).max() <= 1e-13 * np.abs(Gd).max()
        np.testing.assert_allclose(v32, vd, rtol=1e-12, atol=1e-12 * np.abs(vd).max())
    # a large float32 ndarray is uploaded as it is
    with env(BC_GRAM_DMA=0):
        Gh, vh = bc.weighted_gram(Z32)
        G64, v64 = bc.weighted_gram(d64)
    assert np.array_equal(Gh, G64) and np.array_equal(vh, v64)


# ------------------------------------------------------------------ K5
@pytest.mark.parametrize('n,d', [(5000, 7), (30011, 64), (20000, 128), (9000, 200), (3001, 300), (2000, 512), (1500, 513), (1000, 1024)])
def test_k5_newton_pass(bc, n, d):
    rng = np.random.RandomState(n + d)
    Z32 = rows32(rng, n, d, d, special=False)
    Z32[3, :] = np.float32(40.)                                      # m beyond +-100 at the theta below
    Z32[4, 0] = np.float32(1e-41)
    th = rng.randn(d) * 0.5
    d32 = bc.DeviceData(Z32, dtype=np.float32)
    d64 = bc.DeviceData(Z32.astype(np.float64))
    for w in (None, rng.rand(n) * 3.):
        a = bc.logistic_newton_pass(d32, th, w=w, hessian=True, diag=True)
        b = bc.logistic_newton_pass(d64, th, w=w, hessian=True, diag=True)
        assert a[0] == b[0]
        for x, y in zip(a[1:], b[1:]):
            assert np.array_equal(x, y)
    a = bc.logistic_newton_pass(Z32, th, hessian=False)              # a float32 ndarray is uploaded as it is
    b = bc.logistic_newton_pass(d64, th, hessian=False)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])


def test_logistic_laplace_on_float32_rows(bc):
    rng = np.random.RandomState(21)
    n, d = 40000, 12
    X = rng.randn(n, d)
    y = np.where(rng.rand(n) < 1. / (1. + np.exp(-X.dot(rng.randn(d)))), 1., -1.)
    Z32 = (y[:, None] * X).astype(np.float32)
    w = rng.rand(n)
    out = [bc.samplers.logistic_laplace(w, dd, np.zeros(d), solver='newton')
           for dd in (bc.DeviceData(Z32, dtype=np.float32), bc.DeviceData(Z32.astype(np.float64)))]
    for x, y in zip(out[0], out[1]):
        assert np.array_equal(x, y)
    smp = [bc.samplers.LaplaceFullDataSampler(dd, np.zeros(d), rng=np.random.RandomState(2))
           for dd in (bc.DeviceData(Z32, dtype=np.float32), bc.DeviceData(Z32.astype(np.float64)))]
    assert np.array_equal(smp[0].mu, smp[1].mu) and np.array_equal(smp[0].LSig, smp[1].LSig)


# ------------------------------------------------------------------ refusals
def test_float64_only_entry_points_refuse_float32_rows(bc):
    from beta_cores_amd import _native as N
    from beta_cores_amd.device import _ptr
    rng = np.random.RandomState(30)
    Z32 = rng.randn(20, 5).astype(np.float32)
    dd = bc.DeviceData(Z32, dtype=np.float32)
    lib = N.load()
    z64 = np.zeros((20, 5))
    assert lib.bc_data_upload(dd.h, _ptr(z64), 20) == N.BC_INVALID_ARGUMENT
    assert b'float32' in lib.bc_last_error() and b'bc_data_upload' in lib.bc_last_error()
    th = rng.randn(3, 4)
    params = np.array([1.0])
    out = np.zeros((20, 3, 5))
    rc = lib.bc_project_grad_x(dd.ctx.h, dd.h, 0, _ptr(th), 3, _ptr(params), 1, _ptr(out))
    assert rc == N.BC_INVALID_ARGUMENT and b'float32' in lib.bc_last_error() and b'bc_project_grad_x' in lib.bc_last_error()
    # a float32 weights handle of the Newton pass
    w32 = bc.DeviceData(np.ones((20, 1), dtype=np.float32), dtype=np.float32)
    with pytest.raises(ValueError, match='float32'):
        bc.logistic_newton_pass(dd, np.zeros(5), w=w32)
    nb = C.c_int32()
    N.call('bc_data_elem_bytes', dd.h, C.byref(nb))
    assert nb.value == 4
    N.call('bc_data_elem_bytes', bc.DeviceData(z64).h, C.byref(nb))
    assert nb.value == 8
