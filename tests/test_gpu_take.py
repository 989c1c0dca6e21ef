"""Resident rows sub-sampled on the device (DeviceData.take, bc_data_take_rows, k_take_rows) and the coresets that use it:
the gather is NumPy's bit for bit on every lane mapping and access width, a re-used buffer neither leaks nor goes stale,
refusals leave the destination alone, offsets beyond 4 GiB are 64-bit, and BetaCoreset / SparseVI / HilbertCoreset /
BatchPSVICoreset on resident rows select and weigh what they do on the host array."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_ROWS = 3001
DZS = [1, 2, 3, 64, 127, 129, 130, 257]
MS = [0, 1, 63, 64, 65, 1000, 4097]


@pytest.fixture(scope='module')
def bc():
    import beta_cores_amd as bc
    bc.default_context()
    return bc


def fixed(th):
    return lambda n, w, p: th


def table(n, dz, dtype):
    """Distinct, float32-exact values: any misplaced word shows."""
    return (np.arange(n, dtype=np.float64)[:, None] * 1000. + np.arange(dz, dtype=np.float64)[None, :]).astype(dtype)


def patterns(rng, n, m):
    yield 'random', rng.randint(n, size=m)
    yield 'one row', np.full(m, n // 3, dtype=np.int64)
    yield 'ascending', np.sort(rng.randint(n, size=m))
    yield 'descending', np.sort(rng.randint(n, size=m))[::-1]


# ------------------------------------------------------------------ 1. the gather
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('dz', DZS)
def test_take_equals_numpy_bit_for_bit(bc, dz, dtype):
    import torch
    n = N_ROWS
    Z = table(n, dz, dtype)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    whole = torch.from_numpy(Z).cuda()
    padded = torch.zeros(n * dz + 1, dtype=tdt, device='cuda')
    padded[1:] = whole.flatten()
    shifted = padded[1:1 + n * dz].view(n, dz)              # its base is only element-aligned
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == np.dtype(dtype).itemsize
    sources = [('owned', bc.DeviceData(Z, dtype=dtype)), ('borrowed', bc.DeviceData.from_torch(whole)),
               ('borrowed, element-aligned base', bc.DeviceData.from_torch(shifted))]
    rng = np.random.RandomState(dz)
    for name, dd in sources:
        assert dd.dtype == np.dtype(dtype)
        cases = [('ends', np.array([0, n - 1]))]
        for m in MS:
            cases += [('%s m=%d' % (k, m), idx) for k, idx in patterns(rng, n, m)]
        for what, idx in cases:
            got = dd.take(idx)
            assert isinstance(got, bc.DeviceData) and got.shape == (len(idx), dz) and got.dtype == dd.dtype and got.row_offset == 0
            back = got.rows(np.arange(len(idx)))
            assert np.array_equal(back, Z[idx].astype(np.float64)), (name, what)
    # any integer array
    dd = sources[0][1]
    for idx in (np.array([5, 1, 5], dtype=np.int32), np.array([7, 0], dtype=np.uint8), [3, 2, 1]):
        assert np.array_equal(dd.take(idx).rows(np.arange(len(idx))), Z[np.asarray(idx)].astype(np.float64))
    # [] and rows() still hand out float64 host rows
    assert isinstance(dd[[1, 2]], np.ndarray) and dd[[1, 2]].dtype == np.float64 and dd.rows([4]).dtype == np.float64


# ------------------------------------------------------------------ 2. re-use
def test_take_into_a_reused_buffer(bc):
    rng = np.random.RandomState(2)
    n, dz = 20000, 17
    Z = rng.randn(n, dz)
    dd = bc.DeviceData(Z)
    buf = dd.take(rng.randint(n, size=10))
    for m in (10, 5000, 10):
        idx = rng.randint(n, size=m)
        got = dd.take(idx, out=buf)
        assert got is buf and buf.shape == (m, dz)
        assert np.array_equal(buf.rows(np.arange(m)), Z[idx])
    slot = bc.DeviceData.slot(dz)                          # an upload slot serves as a destination too
    idx = rng.randint(n, size=300)
    assert dd.take(idx, out=slot) is slot and np.array_equal(slot.rows(np.arange(300)), Z[idx])


@pytest.mark.parametrize('reuse', [True, False])
def test_repeated_takes_do_not_grow_device_memory(bc, reuse):
    """40 takes of 10 000 rows, into one buffer or dropped one after the other: the bound of
    test_gpu_project.py::test_repeated_large_subsamples_do_not_grow_device_memory."""
    import torch
    rng = np.random.RandomState(3)
    n, dz = 40000, 7
    dd = bc.DeviceData(rng.randn(n, dz))
    buf, free = None, []
    for it in range(40):
        got = dd.take(rng.randint(n, size=10000), out=buf)
        if reuse:
            buf = got
        del got
        if it in (9, 39):
            bc.default_context().sync()
            free.append(torch.cuda.mem_get_info()[0])
    assert free[0] - free[1] < 8 * 2 ** 20, (free[0] - free[1]) / 2 ** 20


# ------------------------------------------------------------------ 3. refusals
def test_refused_takes_leave_the_destination_untouched(bc):
    import torch
    rng = np.random.RandomState(4)
    n, dz = 500, 5
    Z = rng.randn(n, dz)
    dd = bc.DeviceData(Z)
    keep = rng.randint(n, size=40)
    out = dd.take(keep)

    def intact(o=out, idx=keep, src=Z):
        return o.shape == (len(idx), src.shape[1]) and np.array_equal(o.rows(np.arange(len(idx))), src[idx].astype(np.float64))
    with pytest.raises(ValueError, match=r'index -1 .*out of range'):
        dd.take([3, -1, 7], out=out)
    assert intact()
    with pytest.raises(ValueError, match=r'index %d .*out of range' % n):
        dd.take([3, n, n + 5], out=out)
    assert intact()
    with pytest.raises(ValueError, match='out of range'):
        dd.take([n])                                       # ... and without a destination
    with pytest.raises(ValueError, match='columns'):
        bc.DeviceData(rng.randn(n, dz + 1)).take([1, 2], out=out)
    assert intact()
    Z32 = Z.astype(np.float32)
    with pytest.raises(ValueError, match='float32'):
        bc.DeviceData(Z32, dtype=np.float32).take([1, 2], out=out)
    assert intact()
    other = bc.Context(device=bc.default_context().device)
    with pytest.raises(ValueError, match='context'):
        bc.DeviceData(Z, ctx=other).take([1, 2], out=out)
    assert intact()
    with pytest.raises(ValueError, match='source'):
        dd.take([1, 2], out=dd)
    assert dd.shape == (n, dz) and np.array_equal(dd.rows(np.arange(n)), Z)
    t = torch.from_numpy(Z[:40].copy()).cuda()
    borrowed = bc.DeviceData.from_torch(t)
    with pytest.raises(ValueError, match='borrow'):
        dd.take([1, 2], out=borrowed)
    assert intact(borrowed, np.arange(40), Z)
    with pytest.raises(TypeError):
        dd.take([0.5, 1.0])
    with pytest.raises(TypeError):
        dd.take([1], out=Z)
    assert intact()


# ------------------------------------------------------------------ 4. offsets past 4 GiB
def test_take_beyond_four_gib(bc):
    import torch
    n, dz = 4_200_000, 129                                 # 4.33 GB of float64 rows on either side
    t = torch.zeros((n, dz), dtype=torch.float64, device='cuda')
    t[:, 0] = torch.arange(n, dtype=torch.float64, device='cuda')
    t[:, dz - 1] = t[:, 0]
    dd = bc.DeviceData.from_torch(t)
    idx = np.random.RandomState(5).randint(n, size=n)
    idx[-4000:] = np.arange(n - 4000, n)                   # the tail points at the last source rows
    idx[4_161_785:4_161_805] = n - 1 - np.arange(20)       # around output byte 2^32 (row 4 161 789.8 at 1 032 bytes a row)
    got = dd.take(idx)
    assert got.shape == (n, dz)
    probe = np.concatenate(([0], np.arange(4_161_790, 4_161_801), np.arange(n - 10, n)))
    rows = got.rows(probe)
    want = np.zeros((probe.shape[0], dz))
    want[:, 0] = want[:, dz - 1] = idx[probe]
    assert np.array_equal(rows, want)


# ------------------------------------------------------------------ 5. projection of taken rows
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('model', ['linreg', 'logistic'])
def test_projection_of_taken_rows_equals_projection_of_host_rows(bc, model, dtype):
    """m = 100: the upload slot; 5 000: a resident copy; 70 000: the pipelined host path -- against the same rows on the device."""
    rng = np.random.RandomState(6)
    n, D, S = 20000, 8, 32
    lik, dz = (bc.likelihoods.LinearRegression(1.3), D + 1) if model == 'linreg' else (bc.likelihoods.LogisticRegression(), D)
    Z = rng.randn(n, dz).astype(dtype)
    host = Z.astype(np.float64)                            # what [] / rows() hand the host path today
    prj = bc.DeviceBetaProjector(fixed(rng.randn(S, D) * 0.4), S, lik)
    dd = bc.DeviceData(Z, dtype=dtype)
    for m in (100, 5000, 70000):
        idx = rng.randint(n, size=m)
        for beta in (None, 0.1):
            proj = (lambda x: prj.project(x)) if beta is None else (lambda x: prj.project_f(x, beta))
            a, b = proj(dd.take(idx)), proj(host[idx])
            assert a.shape == b.shape == (m, S)
            assert np.array_equal(a.to_host(), b.to_host()), (m, beta)
            assert np.array_equal(a.norms(), b.norms()) and np.array_equal(a.colsum(), b.colsum()), (m, beta)
            assert np.array_equal(prj.colsum(dd.take(idx), beta=beta), prj.colsum(host[idx], beta=beta)), (m, beta)


# ------------------------------------------------------------------ 6. a refilled buffer is never served from the key cache
def test_refilled_buffer_is_not_served_stale_constant_row_keys(bc, monkeypatch):
    from beta_cores_amd.util import numpy_bits
    monkeypatch.setattr(numpy_bits, '_cached', False)      # "this host's NumPy is not the restated one": constants come from the host
    monkeypatch.setattr(numpy_bits, '_warned', set())
    rng = np.random.RandomState(7)
    n, d, S = 6000, 6, 32
    Z = rng.randn(n, d + 1)
    zero = np.array([10, 20, 30, 40, 50])
    Z[zero, :d] = 0.                                        # five all-zero-feature rows, five different y
    with pytest.warns(UserWarning, match='evaluated on the host'):
        prj = bc.DeviceBetaProjector(fixed(rng.randn(S, d) * 0.4), S, bc.likelihoods.LinearRegression(1.7))
    assert prj._host_constants
    dd = bc.DeviceData(Z)
    first = np.concatenate((rng.randint(n, size=4500), zero[:2]))
    second = np.concatenate((rng.randint(n, size=4500), zero[2:]))
    first, second = first[~np.isin(first, zero[2:])], second[~np.isin(second, zero[:2])]
    buf = None
    for idx, n_keys in ((first, 2), (second, 3), (first, 2)):
        want = prj.project_f(Z[idx], 0.2)
        assert prj.constant_rows_from_host == n_keys
        want = want.to_host()
        prj.constant_rows_from_host = -1
        buf = dd.take(idx, out=buf)
        got = prj.project_f(buf, 0.2)
        assert prj.constant_rows_from_host == n_keys
        assert np.array_equal(got.to_host(), want)
        assert np.array_equal(prj.colsum(buf, beta=0.2), got.colsum())


# ------------------------------------------------------------------ 7. greedy VI on resident rows
def _greedy_problem(bc, model):
    rng = np.random.RandomState(8)
    n, D = 6000, 7
    X = rng.randn(n, D)
    if model == 'linreg':
        y = X.dot(rng.randn(D)) + rng.randn(n)
        Z = np.hstack((X[:, :D - 1], y[:, None]))          # 6 features and y: 7 columns
        d = D - 1
        lik = bc.likelihoods.LinearRegression(1.0)
        sampler = lambda: bc.samplers.LinregPosteriorSampler(np.zeros(d), np.eye(d), 1.0)
    else:
        y = np.where(rng.rand(n) < 1. / (1. + np.exp(-X.dot(rng.randn(D)))), 1., -1.)
        Z = y[:, None] * X                                  # rows y*x
        d = D
        lik = bc.likelihoods.LogisticRegression()
        sampler = lambda: bc.samplers.LogisticLaplaceSampler(np.zeros(d), solver='newton')
    return np.ascontiguousarray(Z.astype(np.float32).astype(np.float64)), lik, sampler      # float32-exact: one yardstick serves all


def _rng_state_equal(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.mark.parametrize('subs', [(150, 60), (5000, 4500)])
@pytest.mark.parametrize('kind', ['bcores', 'svi'])
@pytest.mark.parametrize('model', ['linreg', 'logistic'])
def test_greedy_vi_on_resident_rows_equals_the_host_array_path(bc, monkeypatch, model, kind, subs):
    """The data as an ndarray (the yardstick: rows gathered on the host, uploaded per tangent space), as float64 and float32
    DeviceData and as an ndarray the caller pinned: same seed, same draws.  fused_gradient=False: everything bit-equal.
    Default (the sub-sampled gradient fused on resident rows): same selections and RNG position, weights within the
    project's bound for fused against general (test_gpu_storefree.py).  No host gather beyond the coreset's own rows."""
    Z, lik, sampler = _greedy_problem(bc, model)
    S, its = 32, 8
    sched = lambda i: 0.1 / (1. + i)
    biggest = [0]
    orig_rows = bc.DeviceData.rows

    def spy(self, local_idx):
        biggest[0] = max(biggest[0], int(np.asarray(local_idx).size))
        return orig_rows(self, local_idx)
    monkeypatch.setattr(bc.DeviceData, 'rows', spy)

    def run(way, fused):
        if kind == 'bcores':
            prj = bc.DeviceBetaProjector(sampler(), S, lik)
            kw = dict(beta=0.1, learn_beta=False)
            cls = bc.BetaCoreset
        else:
            prj = bc.DeviceProjector(sampler(), S, lik)
            kw = {}
            cls = bc.SparseVICoreset
        if way == 'ndarray':
            data = Z
        elif way == 'f64':
            data = bc.DeviceData(Z)
        elif way == 'f32':
            data = bc.DeviceData(Z.astype(np.float32), dtype=np.float32)
        else:
            data = Z.copy()
            prj.pin(data)
        np.random.seed(99)
        alg = cls(data, prj, n_subsample_select=subs[0], n_subsample_opt=subs[1], opt_itrs=its, step_sched=sched,
                  fused_gradient=fused, **kw)
        assert (alg._dev_data is None) == (way == 'ndarray')
        biggest[0] = 0
        alg.build(3, 3)
        assert biggest[0] <= max(len(alg.idcs), 1), 'a sub-sample went through the host'
        return alg.idcs.copy(), alg.wts.copy(), alg.pts.copy(), np.random.get_state()

    for fused in (False, True):
        ref = run('ndarray', fused)
        assert len(ref[0]) >= 1
        for way in ('f64', 'f32', 'pinned'):
            got = run(way, fused)
            assert np.array_equal(got[0], ref[0]), (way, fused)
            assert _rng_state_equal(got[3], ref[3]), (way, fused)
            assert np.array_equal(got[2], ref[2]), (way, fused)
            if fused:
                np.testing.assert_allclose(got[1], ref[1], rtol=1e-9, atol=1e-13)
            else:
                assert np.array_equal(got[1], ref[1]), (way, fused)


def test_subsampled_gradient_is_fused_on_resident_rows_only(bc):
    """With n_subsample_opt every gradient of a coreset on resident rows is one bc_vi_gradient call over the taken rows,
    scaled by n / n_subsample; fused_gradient=False and a plain ndarray keep the materialising path."""
    Z, lik, sampler = _greedy_problem(bc, 'linreg')
    calls = []

    def build(data, **kw):
        prj = bc.DeviceProjector(sampler(), 32, lik)
        orig = prj.vi_gradient

        def counted(rows, core, w, scale=1., **k):
            calls.append((rows, scale))
            return orig(rows, core, w, scale, **k)
        prj.vi_gradient = counted
        np.random.seed(5)
        alg = bc.SparseVICoreset(data, prj, n_subsample_select=150, n_subsample_opt=60, opt_itrs=4, step_sched=lambda i: 0.1 / (1. + i), **kw)
        alg.build(2, 2)
        return alg
    alg = build(bc.DeviceData(Z))
    assert len(calls) == 2 * 4 and all(r is alg._sub_buf and r.shape[0] == 60 and s == Z.shape[0] / 60 for r, s in calls)
    del calls[:]
    build(bc.DeviceData(Z), fused_gradient=False)
    build(Z)
    assert not calls


# ------------------------------------------------------------------ 8. Hilbert and PSVI
def test_hilbert_subsample_of_resident_rows(bc, monkeypatch):
    rng = np.random.RandomState(9)
    n, D, S = 9000, 8, 64
    Z = rng.randn(n, D + 1)
    prj = bc.DeviceProjector(fixed(rng.randn(S, D) * 0.3), S, bc.likelihoods.LinearRegression(1.0))
    out = []
    for data in (Z, bc.DeviceData(Z)):
        np.random.seed(12)
        alg = bc.HilbertCoreset(data, prj, n_subsample=700)
        alg.build(20, 20)
        out.append(alg.get())
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)
    assert len(out[0][2]) > 5
    taken = []
    orig = bc.DeviceData.take
    monkeypatch.setattr(bc.DeviceData, 'take', lambda self, *a, **k: taken.append(1) or orig(self, *a, **k))
    np.random.seed(12)
    bc.HilbertCoreset(bc.DeviceData(Z), prj, n_subsample=700)
    assert taken == [1]


def test_psvi_subsample_of_resident_rows(bc):
    from oracle import models_ref as M
    rng = np.random.RandomState(10)
    n, D, S = 8000, 5, 32
    X = rng.randn(n, D)
    Z = np.hstack((X, (X.dot(rng.randn(D)) + rng.randn(n))[:, None]))
    E = rng.randn(S, D)

    def sampler(sz, wts, pts):
        if pts.shape[0] == 0:
            wts, pts = np.zeros(1), np.zeros((1, D + 1))
        mu, L, _ = M.linreg_weighted_post(np.zeros(D), np.eye(D), 1.0, pts, wts)
        return mu + E.dot(L.T)
    out = []
    for data in (Z, bc.DeviceData(Z)):
        np.random.seed(13)
        prj = bc.DeviceProjector(sampler, S, bc.likelihoods.LinearRegression(1.0))
        alg = bc.BatchPSVICoreset(data, prj, opt_itrs=6, n_subsample_opt=500, step_sched=lambda m: lambda i: 0.5 / (1. + i))
        alg.build(1, 4)
        out.append((alg.wts.copy(), alg.pts.copy(), np.random.get_state()))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert _rng_state_equal(out[0][2], out[1][2])
