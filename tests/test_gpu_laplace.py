"""The full-data logistic Laplace fit on the MI355X: the rows pass (K5) and its Hessian (K4 without a y column) against a
float64 NumPy evaluation, the device fit against the host routine on the reference's F19 data, first-order optimality at full
size, the two-rank sharded fit, and the sampler feeding a Hilbert coreset."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from laplace_worker import shard_problem            # noqa: E402

pytestmark = pytest.mark.gpu


def reference_terms(Z, th, w):
    """value, grad, diag, H of sum_n w_n ll_n by the formulas of model_lr.py, and the sums of |terms| they are judged against."""
    m = -Z.dot(th)
    big = m >= 100.
    ms = np.where(big, 0., m)
    ll = np.where(big, -m, -np.log1p(np.exp(ms)))
    p = np.where(big, 1., np.exp(ms) / (1. + np.exp(ms)))
    c = np.where(big, 0., p * (1. - p))
    wv = np.ones(Z.shape[0]) if w is None else w
    value, grad = (wv * ll).sum(), Z.T.dot(wv * p)
    diag, H = (wv * c).dot(Z * Z), (Z * (wv * c)[:, None]).T.dot(Z)
    aZ = np.abs(Z)
    return (value, grad, diag, H), (np.abs(wv * ll).sum(), aZ.T.dot(wv * p), (wv * c).dot(Z * Z), (aZ * (wv * c)[:, None]).T.dot(aZ))


def rows(n, d, seed):
    rng = np.random.RandomState(seed)
    Z = rng.randn(n, d)
    th = rng.randn(d) / np.sqrt(d)
    # rows whose m = -z.th sits around 0, above 100 and above 710 (exp(m) overflows there)
    tt = th.dot(th)
    for i, target in zip(range(0, n, 5), [0.3, -0.2, 150., 800., 1e-9, 102., 730.] * n):
        Z[i] = -target * th / tt + (0.01 * rng.randn(d) if target < 1 else 0.)
    return Z, th


SHAPES = [(n, d) for n in (1, 15, 16, 17, 4097) for d in (1, 6, 11, 64, 127, 128, 129, 512)] + \
         [(100_003, d) for d in (6, 128, 129, 512)] + \
         [(n, d) for n in (1, 9, 4097) for d in (256, 257, 513, 777, 1024)]      # (past 512 columns: k_lr_rows<16, 2>)


@pytest.mark.parametrize('n,d', SHAPES)
def test_pass_matches_numpy(n, d):
    import beta_cores_amd as bc
    Z, th = rows(n, d, n * 1000 + d)
    rng = np.random.RandomState(d)
    wr = rng.rand(n) * 5.
    wz = wr.copy()
    wz[rng.rand(n) < 0.3] = 0.
    dz = bc.DeviceData(Z)
    for w in (None, wr, wz):
        v, g, H, dg = bc.logistic_newton_pass(dz, th, w=w, hessian=True, diag=True)
        (rv, rg, rd, rH), (sv, sg, sd, sH) = reference_terms(Z, th, w)
        assert abs(v - rv) <= 1e-12 * sv, (v, rv)
        assert np.all(np.abs(g - rg) <= 1e-12 * sg + 1e-300), np.abs(g - rg).max()
        assert np.all(np.abs(dg - rd) <= 1e-12 * sd + 1e-300), np.abs(dg - rd).max()
        assert np.all(np.abs(H - rH) <= 1e-12 * sH + 1e-300), np.abs(H - rH).max()
        assert np.array_equal(H, H.T)
        # the same call again: the same bits
        v2, g2, H2, dg2 = bc.logistic_newton_pass(dz, th, w=w, hessian=True, diag=True)
        assert v2 == v and np.array_equal(g2, g) and np.array_equal(H2, H) and np.array_equal(dg2, dg)
        # value-only pass: the same value and gradient
        v3, g3, H3, dg3 = bc.logistic_newton_pass(dz, th, w=w, hessian=False)
        assert H3 is None and dg3 is None and v3 == v and np.array_equal(g3, g)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_more_than_1024_columns_are_refused(dtype):
    """The rows pass holds a row in 16 column slots of 64 lanes: 1025 columns are refused before anything is launched."""
    import beta_cores_amd as bc
    dz = bc.DeviceData(np.ones((3, 1025), dtype=dtype), dtype=dtype)
    for hessian in (True, False):
        with pytest.raises(ValueError, match=r'1 \.\. 1024 columns, got 1025'):
            bc.logistic_newton_pass(dz, np.zeros(1025), hessian=hessian)
    v, g, H, dg = bc.logistic_newton_pass(bc.DeviceData(np.ones((3, 1024), dtype=dtype), dtype=dtype), np.zeros(1024), hessian=False)
    assert abs(v + 3. * np.log(2.)) <= 1e-14 and np.array_equal(g, np.full(1024, 1.5))      # (the context is as usable as before)


def test_weighted_gram_unchanged_beside_the_pass():
    """K4's own callers (rows [x, y]) keep their bits after the no-y-column mode has run on the same context."""
    import beta_cores_amd as bc
    rng = np.random.RandomState(5)
    Z = rng.randn(20000, 97)
    w = rng.rand(20000)
    G0, v0 = bc.weighted_gram(bc.DeviceData(Z), w)
    bc.logistic_newton_pass(bc.DeviceData(Z[:, :96].copy()), rng.randn(96) * 0.1, w=w)
    G1, v1 = bc.weighted_gram(bc.DeviceData(Z), w)
    assert np.array_equal(G0, G1) and np.array_equal(v0, v1)


def test_f19_anchor(golden):
    import beta_cores_amd as bc
    g = golden('f19_logistic_greedy_vi')
    Z = g['S37_Z']
    D = Z.shape[1]
    dz = bc.DeviceData(Z)
    checked = 0
    for alg in ('bcores', 'svi'):
        for k in range(5):
            key = 'S37_laplace_%s_allw_%d' % (alg, k)
            if key not in g.files:
                continue
            wts, idcs = g[key], g['S37_laplace_%s_allidcs_%d' % (alg, k)]
            wfull = np.zeros(Z.shape[0])
            wfull[idcs] = wts
            h_bfgs = bc.samplers.logistic_laplace(wts, Z[idcs], np.zeros(D))
            h_newton = bc.samplers.logistic_laplace(wts, Z[idcs], np.zeros(D), solver='newton')
            d_newton = bc.samplers.logistic_laplace(wfull, dz, np.zeros(D), solver='newton')
            d_bfgs = bc.samplers.logistic_laplace(wfull, dz, np.zeros(D))
            np.testing.assert_allclose(d_newton[0], h_bfgs[0], rtol=0, atol=1e-5)
            np.testing.assert_allclose(d_bfgs[0], h_bfgs[0], rtol=0, atol=1e-5)
            np.testing.assert_allclose(d_newton[0], h_newton[0], rtol=0, atol=1e-9)
            np.testing.assert_allclose(d_newton[2], h_newton[2], rtol=0, atol=1e-9)
            np.testing.assert_allclose(d_newton[1].dot(d_newton[2]), np.eye(D), atol=1e-10)
            dd = bc.samplers.logistic_laplace(wfull, dz, np.zeros(D), diag=True, solver='newton')
            hd = bc.samplers.logistic_laplace(wts, Z[idcs], np.zeros(D), diag=True, solver='newton')
            np.testing.assert_allclose(dd[2], hd[2], rtol=0, atol=1e-9)
            checked += 1
    assert checked == 10


def test_all_zero_weights_prior():
    import beta_cores_amd as bc
    Z, _ = rows(300, 5, 3)
    mu, LSig, LSigInv = bc.samplers.logistic_laplace(np.zeros(300), bc.DeviceData(Z), np.ones(5), solver='newton')
    np.testing.assert_array_equal(mu, np.zeros(5))
    np.testing.assert_array_equal(LSigInv, np.eye(5))


@pytest.mark.parametrize('n,d', [(10_000_000, 128), (2_000_000, 512)])
def test_full_size(n, d):
    import torch
    import beta_cores_amd as bc
    dev = torch.device('cuda', 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234 + d)
    Z = torch.randn((n, d), dtype=torch.float64, device=dev, generator=gen)
    ths = torch.randn(d, dtype=torch.float64, device=dev, generator=gen) * (2. / np.sqrt(d))
    u = torch.rand(n, dtype=torch.float64, device=dev, generator=gen)
    y = torch.where(u < torch.sigmoid(Z @ ths), 1., -1.).to(torch.float64)
    Z.mul_(y[:, None])
    del y, u
    w_t = torch.rand(n, dtype=torch.float64, device=dev, generator=gen) * 2.
    w_t[::11] = 0.
    w = w_t.cpu().numpy()
    torch.cuda.synchronize()
    dz = bc.DeviceData.from_torch(Z)
    mu, LSig, LSigInv = bc.samplers.logistic_laplace(w, dz, np.zeros(d), solver='newton')
    # first-order optimality, recomputed independently with chunked torch GEMMs
    mu_t = torch.from_numpy(mu).to(dev)
    zp = torch.zeros(d, dtype=torch.float64, device=dev)
    H = torch.zeros((d, d), dtype=torch.float64, device=dev)
    for a in range(0, n, 1 << 20):
        Zc = Z[a:a + (1 << 20)]
        p = torch.sigmoid(-(Zc @ mu_t))
        zp += Zc.T @ (w_t[a:a + (1 << 20)] * p)
        H += (Zc * (w_t[a:a + (1 << 20)] * p * (1. - p))[:, None]).T @ Zc
    zp, H = zp.cpu().numpy(), H.cpu().numpy()
    grad = -mu + zp
    assert np.abs(grad).max() <= 1e-8 * (1. + np.abs(zp).max()), np.abs(grad).max()
    _, _, Hd, _ = bc.logistic_newton_pass(dz, mu, w=w, hessian=True)
    assert np.abs(Hd - H).max() <= 1e-11 * np.abs(H).max(), np.abs(Hd - H).max() / np.abs(H).max()
    np.testing.assert_allclose(LSigInv.dot(LSigInv.T), np.eye(d) + Hd, rtol=0, atol=1e-9 * np.abs(Hd).max())
    mu_b = bc.samplers.logistic_laplace(w, dz, np.zeros(d))[0]
    assert np.abs(mu_b - mu).max() <= 1e-5, np.abs(mu_b - mu).max()
    del dz, Z, w_t
    torch.cuda.empty_cache()


def _launch_two_ranks(tmp_path, timeout=240):
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / 'laplace')
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), OMP_NUM_THREADS='2',
                   HSA_ENABLE_IPC_MODE_LEGACY='0')
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, 'tests', 'laplace_worker.py'), out], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = []
    try:
        for p in procs:
            o, _ = p.communicate(timeout=timeout)
            logs.append(o.decode('utf-8', 'replace'))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, p in enumerate(procs):
        assert p.returncode == 0, 'rank %d failed:\n%s' % (r, logs[r][-3000:])
    return [np.load(out + '.rank%d.npz' % r) for r in range(2)]


def test_two_rank_shards(tmp_path):
    import beta_cores_amd as bc
    Z, w = shard_problem()
    dz = bc.DeviceData(Z)
    r0, r1 = _launch_two_ranks(tmp_path)
    for solver in ('newton', 'bfgs'):
        mu, _, LSigInv = bc.samplers.logistic_laplace(w, dz, np.zeros(Z.shape[1]), solver=solver)
        for r in (r0, r1):
            np.testing.assert_allclose(r[solver + '_mu'], mu, rtol=0, atol=(1e-10 if solver == 'newton' else 1e-6) * (1. + np.abs(mu).max()))
            np.testing.assert_allclose(r[solver + '_LSigInv'], LSigInv, rtol=0, atol=1e-10 * np.abs(LSigInv).max())
        assert np.array_equal(r0[solver + '_mu'], r1[solver + '_mu'])
        assert np.array_equal(r0[solver + '_LSigInv'], r1[solver + '_LSigInv'])


def test_full_data_sampler_hilbert_end_to_end():
    import beta_cores_amd as bc
    rng = np.random.RandomState(8)
    n, d = 1_000_000, 10
    X = rng.randn(n, d)
    y = np.where(rng.rand(n) < 1. / (1. + np.exp(-X.dot(rng.randn(d)))), 1., -1.)
    Z = y[:, None] * X
    smp = bc.samplers.LaplaceFullDataSampler(bc.DeviceData(Z), np.zeros(d), rng=np.random.RandomState(1))
    th = smp(4, None, None)
    assert th.shape == (4, d) and np.all(np.isfinite(th))
    prj = bc.DeviceProjector(smp, 100, bc.likelihoods.LogisticRegression())
    alg = bc.HilbertCoreset(Z, prj)
    errs = []
    for m in range(10, 51, 10):
        alg.build(10, m)
        errs.append(alg.error())
    assert all(np.isfinite(errs)) and all(b <= a * (1. + 1e-12) for a, b in zip(errs, errs[1:])), errs
    assert alg.size() > 0


def test_example_runs():
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'logistic_hilbert.py'), '--n', '20000', '--d', '5',
                          '--sizes', '10,30'], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr[-3000:]
    assert 'GIGAO' in res.stdout and 'GIGAR' in res.stdout and 'KL' in res.stdout, res.stdout
