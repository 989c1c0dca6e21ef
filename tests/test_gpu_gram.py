"""GPU parity of K4 (weighted Gram, fp64 MFMA) and the posterior update built on it."""
import numpy as np
import pytest

from conftest import load_golden
from oracle import models_ref as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def bc():
    import beta_cores_amd as bc
    bc.default_context()
    return bc


@pytest.mark.parametrize('n,d', [(1, 1), (5, 3), (17, 16), (300, 8), (1000, 63), (1000, 64), (999, 65), (2000, 95),
                                 (2000, 96), (3000, 127), (3000, 128), (1500, 200), (700, 512),
                                 (40, 2049), (60, 2100), (30, 4200)])     # D > 2048: X^T (w*y) needs several chunk trips (k_gram_reduce2)
@pytest.mark.parametrize('weighted', [True, False])
def test_gram_matches_numpy(bc, n, d, weighted):
    rng = np.random.RandomState(n + d)
    Z = rng.randn(n, d + 1)
    w = rng.rand(n) * 2. if weighted else None
    G, v = bc.weighted_gram(Z, w)
    Gr, vr = M.linreg_xtwx(Z, w if weighted else np.ones(n))
    scale = np.abs(Gr).max()
    assert np.abs(G - Gr).max() <= 1e-12 * scale
    assert np.abs(v - vr).max() <= 1e-12 * max(1., np.abs(vr).max())
    assert np.array_equal(G, G.T)                                     # mirrored from the upper triangle: exactly symmetric


def test_f6_weighted_post_goldens(bc):
    g = load_golden('f6_weighted_post')
    for D in (8, 64):
        mu, L, Linv = bc.weighted_post(g['D%d_th0' % D], g['D%d_Sig0inv' % D], 1.7, g['D%d_Z' % D], g['D%d_w' % D])
        np.testing.assert_allclose(mu, g['D%d_mu' % D], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(L, g['D%d_L' % D], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(Linv, g['D%d_Linv' % D], rtol=1e-9, atol=1e-12)
        # the reference's mean is NOT the true posterior mean on this anisotropic design (quirk kept)
        mu_true = bc.weighted_post_corrected(g['D%d_th0' % D], g['D%d_Sig0inv' % D], 1.7, g['D%d_Z' % D], g['D%d_w' % D])[0]
        assert np.abs(mu_true - mu).max() > 1e-3
    mu, L, Linv = bc.gaussian_weighted_post(np.zeros(8), np.eye(8), g['g_Siginv'], g['g_X'], g['g_w'])
    np.testing.assert_allclose(mu, g['g_mu'], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(L, g['g_L'], rtol=1e-12)


def test_gram_large_rows_splitk(bc):
    rng = np.random.RandomState(0)
    n, d = 200_000, 64
    Z = rng.randn(n, d + 1)
    w = rng.rand(n)
    G, v = bc.weighted_gram(Z, w)
    Gr, vr = M.linreg_xtwx(Z, w)
    assert np.abs(G - Gr).max() <= 1e-12 * np.abs(Gr).max()
    assert np.abs(v - vr).max() <= 1e-11 * np.abs(vr).max()
    G2, v2 = bc.weighted_gram(Z, w)
    assert np.array_equal(G, G2) and np.array_equal(v, v2)            # fixed split order: run-to-run deterministic


@pytest.mark.parametrize('n', [4096, 10_007, 100_001, 262_145])
@pytest.mark.parametrize('d', [127, 128])
def test_gram_lds_dma_kernel(bc, n, d, monkeypatch):
    """One unweighted diagonal tile whose rows hold >= 128 doubles (the drivers' full-data posterior at D = 128,
    model_linreg.py:25-34 with w = 1) runs k_gram_dma: slabs go from global memory straight into LDS, 32 rows at a time,
    double-buffered.  Row counts that end inside a slab (zero-filled rows), one that is a multiple of 32, one row more than
    a multiple of the split size.  Run-to-run deterministic; against the register-staged kernel (BC_GRAM_DMA=0) the results
    agree to rounding (the row splits, and with them the association of the partial sums, follow the slab size); both
    match NumPy."""
    rng = np.random.RandomState(n + d)
    Z = rng.randn(n, d + 1)
    Z[-1, -1] = 7.5                                       # the last row's y: the end of the array is read exactly, not past
    monkeypatch.setenv('BC_GRAM_DMA', '1')
    G, v = bc.weighted_gram(Z, None)
    G2, v2 = bc.weighted_gram(Z, None)
    assert np.array_equal(G, G2) and np.array_equal(v, v2)
    monkeypatch.setenv('BC_GRAM_DMA', '0')
    G0, v0 = bc.weighted_gram(Z, None)
    assert np.abs(G - G0).max() <= 1e-13 * np.abs(G0).max()
    np.testing.assert_allclose(v, v0, rtol=1e-12, atol=1e-12 * np.abs(v0).max())
    Gr, vr = M.linreg_xtwx(Z, np.ones(n))
    assert np.abs(G - Gr).max() <= 1e-12 * np.abs(Gr).max()
    assert np.abs(v - vr).max() <= 1e-11 * max(1., np.abs(vr).max())
    assert np.array_equal(G, G.T)


# ---------------------------------------------------------------------------------------------------------------------
# Every route into K4 against a long-double reference and the derived element-wise bound of tests/gram_cases.py
# (|G - Gr| <= (n + 3) 2^-53 |X|^T diag(|w|) |X|): the coreset-sized host entry on both sides of 512 rows, resident rows down to
# one, every split count at which the two reduction levels change their shape, the LDS-DMA kernel's edge, reused scratch, and
# NaN containment.  tests/test_gram_cases_cpu.py holds the lists against the split arithmetic the launch code uses.
import gram_cases as GC                                                          # noqa: E402


def need_longdouble():
    if not GC.LONGDOUBLE_OK:
        pytest.skip(GC.LONGDOUBLE_WHY)


def host_gram(bc, Z, w, d=None):
    """bc_weighted_gram_host called directly: the coreset-sized host entry and nothing else"""
    from beta_cores_amd import _native as N
    from beta_cores_amd.device import _ptr
    d = Z.shape[1] - 1 if d is None else d
    G, v = np.full((d, d), np.nan), np.full(d, np.nan)
    N.call('bc_weighted_gram_host', bc.default_context().h, _ptr(Z), int(Z.shape[0]), int(Z.shape[1]), _ptr(w) if w is not None else None,
           _ptr(G), _ptr(v))
    return G, v


def same_bits(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def inside(route, G, v, n, dz, kind, w, ref):
    """G and v lie inside the bound (the figure is printed first: profiles/k4_routes_notes.md) and G is exactly symmetric"""
    r = GC.ratio(G, v, n, ref)
    print('K4 error/bound %s n=%d dz=%d %s %s %.4f' % (route, n, dz, kind, 'w' if w is not None else '1', r))
    assert r <= 1., (route, n, dz, kind, w is not None, r)
    assert np.array_equal(G, G.T, equal_nan=True)


@pytest.mark.parametrize('n,dz', GC.SMALL)
def test_gram_small_host_entry(bc, n, dz):
    """k_gram_small (n <= 512), called directly through the native entry point so that the route is certain."""
    need_longdouble()
    for kind in GC.KINDS:
        for weighted in (True, False):
            Z, w, ref = GC.case(n, dz, kind, weighted)
            G, v = host_gram(bc, Z, w)
            inside('small', G, v, n, dz, kind, w, ref)
            assert same_bits(host_gram(bc, Z, w), (G, v))                        # run-to-run
            assert same_bits(bc.weighted_gram(Z, w), (G, v))                     # the public call takes this route for an ndarray
        G0, v0 = host_gram(bc, Z, np.zeros(n))
        assert not G0.any() and not v0.any()                                     # all-zero weights: exact zeros


@pytest.mark.parametrize('n,dz', GC.HOST_BIG)
def test_gram_host_entry_past_512_rows(bc, n, dz):
    """The host entry's other half: run_gram<64 / 128> on a view of the staging buffer.  The same run_gram, n, dz and weights as
    the resident route, hence the same splits and the same bits."""
    need_longdouble()
    for kind in GC.KINDS:
        for weighted in (True, False):
            Z, w, ref = GC.case(n, dz, kind, weighted)
            G, v = host_gram(bc, Z, w)
            inside('host-big', G, v, n, dz, kind, w, ref)
            assert same_bits(bc.weighted_gram(bc.DeviceData(Z), w), (G, v))
            assert same_bits(bc.weighted_gram(Z, w), (G, v))


def test_gram_host_entry_limits(bc):
    need_longdouble()
    Z, w, ref = GC.case(129, 18, 'plain', True)
    before = host_gram(bc, Z, w)
    inside('small', before[0], before[1], 129, 18, 'plain', w, ref)
    with pytest.raises(ValueError, match='coreset-sized'):
        host_gram(bc, np.ones((70_000, 2)), None)
    assert same_bits(host_gram(bc, Z, w), before)
    with pytest.raises(ValueError, match='rows must be'):
        host_gram(bc, np.ones((5, 1)), None, d=1)                                # dz = 1: no x column
    assert same_bits(host_gram(bc, Z, w), before)
    G, v = host_gram(bc, np.zeros((0, 18)), None)
    assert G.shape == (17, 17) and not G.any() and not v.any()                   # zero rows: zeros (not the NaN the buffers held)
    assert same_bits(host_gram(bc, Z, w), before)


def resident_case(bc, route, n, d, f32=False):
    for kind in GC.KINDS:
        Z = GC.case(n, d + 1, kind, True)[0]
        data = bc.DeviceData(Z)
        if f32:
            Z32 = Z.astype(np.float32)
            d32, d64 = bc.DeviceData(Z32, dtype=np.float32), bc.DeviceData(Z32.astype(np.float64))
        for weighted in (True, False):
            Z, w, ref = GC.case(n, d + 1, kind, weighted)
            G, v = bc.weighted_gram(data, w)
            inside(route, G, v, n, d + 1, kind, w, ref)
            assert same_bits(bc.weighted_gram(data, w), (G, v))
            if f32:                                                              # float32 rows: the bits of the float64 handle of the widened rows
                assert same_bits(bc.weighted_gram(d32, w), bc.weighted_gram(d64, w))


@pytest.mark.parametrize('n,d', GC.RESIDENT_FEW)
def test_gram_few_resident_rows(bc, n, d):
    """Fewer rows than a slab, than two, a last split of one row or of one slab, through k_gram (weighted: two panels;
    unweighted: one) for both tile sizes and one, three and six tiles."""
    need_longdouble()
    resident_case(bc, 'resident-few', n, d, f32=d in GC.RESIDENT_F32_D)


@pytest.mark.parametrize('n,d', GC.SPLIT_EDGES)
def test_gram_split_edges(bc, n, d):
    """Split counts at which k_gram_reduce1 (runs of 16, eight at a time plus a remainder) and k_gram_reduce2 (eight parts of
    ceil(splits / 8); the runs eight at a time) change shape, each with its n + 1 whose last split holds one row."""
    need_longdouble()
    resident_case(bc, 'split-edges', n, d)


@pytest.mark.parametrize('n,d', [(4095, 128), (4097, 128), (4096, 126)])
def test_gram_dma_kernel_edge(bc, n, d, monkeypatch):
    """The shapes next to the ones k_gram_dma takes (unweighted, 4096 rows or more of 128 doubles or more): one row fewer, one
    more (a last split of one row), one column too few."""
    need_longdouble()
    monkeypatch.setenv('BC_GRAM_DMA', '1')
    for kind in GC.KINDS:
        Z, w, ref = GC.case(n, d + 1, kind, False)
        data = bc.DeviceData(Z)
        G, v = bc.weighted_gram(data, None)
        inside('dma-edge', G, v, n, d + 1, kind, None, ref)
        if GC.route(n, d, False)['dma']:
            # both kernels take the rows in the same k-step order (bc_gram.hip): where the splits agree, the same bits in G
            # (X^T y is summed in another order and agrees to rounding)
            monkeypatch.setenv('BC_GRAM_DMA', '0')
            G0, v0 = bc.weighted_gram(data, None)
            monkeypatch.setenv('BC_GRAM_DMA', '1')
            inside('dma-edge(staged)', G0, v0, n, d + 1, kind, None, ref)
            r1, r0 = GC.route(n, d, False), GC.route(n, d, False, dma_env=0)
            assert not r0['dma']
            if (r1['rps'], r1['splits']) == (r0['rps'], r0['splits']):
                assert G.tobytes() == G0.tobytes()


def test_gram_reused_scratch(bc):
    """The partial-tile buffers grow only and are reused, and the sub-tiles below the diagonal of a diagonal tile are never
    written: a small Gram after a larger one of another shape and tile size has the bits it had before."""
    need_longdouble()
    Za, wa, refa = GC.case(40, 6, 'plain', True)
    Zb, wb, _ = GC.case(2000, 201, 'plain', True)
    da, db = bc.DeviceData(Za), bc.DeviceData(Zb)
    A = bc.weighted_gram(da, wa)
    inside('resident-few', A[0], A[1], 40, 6, 'plain', wa, refa)
    B = bc.weighted_gram(db, wb)
    assert same_bits(bc.weighted_gram(da, wa), A)
    assert same_bits(bc.weighted_gram(db, wb), B)
    Gb, vb = M.linreg_xtwx(Zb, wb)
    assert np.abs(B[0] - Gb).max() <= 1e-12 * np.abs(Gb).max() and np.abs(B[1] - vb).max() <= 1e-12 * np.abs(vb).max()
    # the host entry: k_gram_small, then run_gram<64>, then run_gram<128>, and back
    hs, hb, hc = GC.case(129, 18, 'plain', True), GC.case(900, 65, 'plain', True), GC.case(513, 101, 'plain', True)
    S, C = host_gram(bc, hs[0], hs[1]), host_gram(bc, hc[0], hc[1])
    Bh = host_gram(bc, hb[0], hb[1])
    assert same_bits(host_gram(bc, hs[0], hs[1]), S)
    assert same_bits(host_gram(bc, hc[0], hc[1]), C)
    assert same_bits(host_gram(bc, hb[0], hb[1]), Bh)
    inside('host-big', Bh[0], Bh[1], 900, 65, 'plain', hb[1], hb[2])


@pytest.mark.parametrize('where', ['x', 'y'])
@pytest.mark.parametrize('route,n,dz,weighted', [('small', 129, 33, True), ('resident', 65, 64, True), ('resident', 1000, 200, True),
                                                 ('dma', 4096, 128, False)])
def test_gram_nan_stays_where_it_belongs(bc, route, n, dz, weighted, where):
    """One NaN in the last row (whose weight is positive): in the last x column, next to y, or in y itself.  Rows past the end and
    columns past D are zero-filled or range-rejected, and at D = 127 k_gram_dma carries y as panel column 127: the NaN must
    reach the row and column of G (the entries of v) it belongs to and nothing else."""
    need_longdouble()
    Z, w = GC.inputs(n, dz, 'plain')
    w = w if weighted else None
    Z[n - 1, dz - 2 if where == 'x' else dz - 1] = np.nan
    assert GC.route(n, dz - 1, weighted)['dma'] == (route == 'dma')
    ref = GC.reference(Z, w)
    with np.errstate(invalid='ignore'):
        Gn, vn = M.linreg_xtwx(Z, w if weighted else np.ones(n))
    want = np.zeros((dz - 1, dz - 1), dtype=bool)
    if where == 'x':
        want[dz - 2, :] = want[:, dz - 2] = True
    assert np.array_equal(np.isnan(Gn), want) and np.array_equal(np.isnan(ref[0]), want)
    assert np.array_equal(np.isnan(vn), np.isnan(ref[1])) and np.isnan(vn).sum() == (1 if where == 'x' else dz - 1)
    G, v = host_gram(bc, Z, w) if route == 'small' else bc.weighted_gram(bc.DeviceData(Z), w)
    assert np.array_equal(np.isnan(G), np.isnan(Gn)) and np.array_equal(np.isnan(v), np.isnan(vn))
    inside('nan-' + route, G, v, n, dz, 'plain', w, ref)


def test_sampler_shapes_end_to_end(bc):
    """The samplers' shapes (M = 250 .. 300 coreset rows, D = 100) through the posterior update, with the F6 test's tolerances;
    Sig0inv = I keeps the condition number of the Cholesky near 15."""
    Z, w = GC.inputs(300, 101, 'plain')
    th0 = np.linspace(-1., 1., 100)
    got = bc.weighted_post(th0, np.eye(100), 1.7, Z, w)
    for a, b in zip(got, M.linreg_weighted_post(th0, np.eye(100), 1.7, Z, w)):
        np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-12)
    X, w = GC.inputs(250, 100, 'plain')
    th0 = np.linspace(-1., 1., 100)
    Siginv = np.diag(np.linspace(0.5, 1.5, 100))
    got = bc.gaussian_weighted_post(th0, np.eye(100), Siginv, X, w)
    for a, b in zip(got, M.gauss_weighted_post(th0, np.eye(100), Siginv, X, w)):
        np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-12)
