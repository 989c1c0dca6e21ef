"""The device feature encoder (k_encode_mlp, bc_data_encode, encoders.MLPEncoder, DeviceData.encode) and the projectors and
coresets that run on RAW resident rows through it.

Values are checked against the NumPy float64 restatement `MLPEncoder.host(bound=True)`, which carries an elementwise forward
error bound e through the layers (u = 2^-53, gamma_k = k u / (1 - k u)):
    a = |W||h| + |b|;   e_pre = |W| e_in + 2 gamma_{K+2} a;   e_post = |s| e_pre + 4 u (|pre * s| + |t|);   e_in = 0
(a K-term dot product plus the bias in any order is within gamma_{K+1} a of the exact value; two such evaluations are compared,
hence the factor 2 and the +1 of slack; the epilogue is three roundings on each side).  A float64 device result must lie within
e of the restatement, a float32 one within e + ulp32/2 + 2^-150.  Everything else is bit equality."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encode_shapes as ES            # noqa: E402

pytestmark = pytest.mark.gpu

NS = [1, 15, 16, 17, 127, 129, 1000]
WIDTHS = [(13, 20, 20), (1, 1), (3, 5, 7), (32, 512), (13, 100, 100), (512, 512, 512), (33, 130, 4, 9), (20, 20, 20, 20, 20)]
PASS = [0, 1, 2]
DTYPES = [np.float64, np.float32]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'f23_neural_encoder.npz')


def _cases():
    """A fixed, seeded thinning of the full product (2 688 combinations): every width set at n = 17 and n = 129, every n twice
    more, the other factors cycled so that every value of every factor occurs (checked by test_case_list_covers_every_factor)."""
    rng = np.random.RandomState(20)
    out, i = [], 0
    pairs = [(n, w) for w in WIDTHS for n in (17, 129)] + [(n, WIDTHS[rng.randint(len(WIDTHS))]) for n in NS for _ in range(2)]
    for n, w in pairs:
        out.append((n, w, PASS[i % 3], DTYPES[(i // 3) % 2], DTYPES[(i // 2) % 2], bool((i // 4) % 2), bool(i % 2)))
        i += 1
    return out


CASES = _cases()


@pytest.fixture(scope='module')
def bc():
    import beta_cores_amd as bc
    bc.default_context()
    return bc


def fixed(th):
    return lambda n, w, p: th


def make_layers(rng, widths, last_relu=True, affine=True):
    layers = []
    L = len(widths) - 1
    for l in range(L):
        din, dout = widths[l], widths[l + 1]
        W = rng.randn(dout, din) / np.sqrt(din)
        b = rng.randn(dout) * 0.3
        s, t = (rng.rand(dout) + 0.5, rng.randn(dout) * 0.2) if affine else (None, None)
        layers.append((W, b, s, t, True if l < L - 1 else last_relu))
    return layers


def ulp32(h):
    return np.spacing(np.abs(h).astype(np.float32)).astype(np.float64)


def check_features(got, h, e, out_dtype, what=''):
    allow = e if out_dtype == np.float64 else e + ulp32(h) / 2. + 2.0 ** -150
    err = np.abs(got - h)
    worst = np.nanmax(err - allow) if err.size else -1.
    print('%s max err %.3e, max bound %.3e' % (what, err.max() if err.size else 0., allow.max() if allow.size else 0.))
    assert np.all(err <= allow), (what, worst)


def encode_host(bc, enc, Z, pass_cols, src_dtype, out_dtype, **kw):
    dd = bc.DeviceData(Z.astype(src_dtype), dtype=src_dtype)
    out = dd.encode(enc, pass_cols=pass_cols, dtype=out_dtype, **kw)
    assert isinstance(out, bc.DeviceData) and out.dtype == np.dtype(out_dtype)
    assert out.shape == (Z.shape[0], enc.widths[-1] + pass_cols)
    return out.rows(np.arange(Z.shape[0]))


# ------------------------------------------------------------------ 1. values
def test_case_list_covers_every_factor():
    assert {c[0] for c in CASES} == set(NS) and {c[1] for c in CASES} == set(WIDTHS) and {c[2] for c in CASES} == set(PASS)
    for k in (3, 4):
        assert {c[k] for c in CASES} == set(DTYPES)
    for k in (5, 6):
        assert {c[k] for c in CASES} == {True, False}
    for w in WIDTHS:
        assert {c[0] for c in CASES if c[1] == w} >= {17, 129}


@pytest.mark.parametrize('case', range(len(CASES)))
def test_encode_against_the_host_restatement(bc, case):
    n, widths, p, src_dtype, out_dtype, last_relu, affine = CASES[case]
    rng = np.random.RandomState(1000 + case)
    enc = bc.encoders.MLPEncoder(make_layers(rng, widths, last_relu, affine))
    assert enc.widths == widths
    Z = rng.randn(n, widths[0] + p).astype(src_dtype)
    got = encode_host(bc, enc, Z, p, src_dtype, out_dtype)
    dl = widths[-1]
    h, e = enc.host(Z[:, :widths[0]].astype(np.float64), dtype=np.float64, bound=True)
    check_features(got[:, :dl], h, e, out_dtype, 'n=%d widths=%s' % (n, widths))
    # pass-through columns: the source's values, rounded only when float64 rows are stored as float32
    want = Z[:, widths[0]:].astype(out_dtype).astype(np.float64)
    assert np.array_equal(got[:, dl:], want)
    if not last_relu:
        assert (got[:, :dl] < 0).any() or n * dl < 8
    # the restatement rounded to the storage type is what host(dtype=) returns
    assert np.array_equal(enc.host(Z[:, :widths[0]], dtype=out_dtype), h.astype(out_dtype).astype(np.float64))


@pytest.mark.parametrize('widths', WIDTHS)
def test_float32_output_is_the_float64_output_rounded(bc, widths):
    rng = np.random.RandomState(3)
    enc = bc.encoders.MLPEncoder(make_layers(rng, widths))
    for n in (17, 129):
        Z = rng.randn(n, widths[0] + 1).astype(np.float32)
        for src in DTYPES:
            a = encode_host(bc, enc, Z, 1, src, np.float64)
            b = encode_host(bc, enc, Z, 1, src, np.float32)
            assert np.array_equal(b, a.astype(np.float32).astype(np.float64)), (n, src)
        # ... and the source's storage type does not matter either (float32 rows are widened exactly)
        assert np.array_equal(encode_host(bc, enc, Z, 1, np.float32, np.float64), encode_host(bc, enc, Z, 1, np.float64, np.float64))


def test_a_rows_bits_do_not_depend_on_its_company(bc):
    rng = np.random.RandomState(4)
    for widths in ((13, 20, 20), (33, 130, 4, 9), (32, 512)):
        enc = bc.encoders.MLPEncoder(make_layers(rng, widths))
        n = 129
        Z = rng.randn(n, widths[0] + 1).astype(np.float32)
        dd = bc.DeviceData(Z, dtype=np.float32)
        whole = dd.encode(enc).rows(np.arange(n))
        for i in (0, 15, 16, 77, 128):
            alone = bc.DeviceData(Z[i:i + 1], dtype=np.float32).encode(enc).rows([0])
            assert np.array_equal(alone[0], whole[i]), (widths, i)
        buf = ebuf = None
        for m in (40, 300, 7):
            idx = rng.randint(n, size=m)
            buf = dd.take(idx, out=buf)
            first = ebuf is None
            ebuf = buf.encode(enc, out=ebuf)
            assert ebuf._transient == (not first) and ebuf.shape == (m, widths[-1] + 1)      # (a refilled buffer is transient)
            assert np.array_equal(ebuf.rows(np.arange(m)), whole[idx]), (widths, m)
        # enc(pts): host rows in, the device's bits out
        assert np.array_equal(enc(Z[:9].astype(np.float64)), whole[:9])


# ------------------------------------------------------------------ 2. edges
def test_nan_and_inf_rows(bc):
    rng = np.random.RandomState(5)
    widths = (13, 20, 20)
    enc = bc.encoders.MLPEncoder(make_layers(rng, widths))
    n = 40
    Z = rng.randn(n, 14)
    clean = encode_host(bc, enc, Z, 1, np.float64, np.float64)
    bad = Z.copy()
    bad[5, :13] = np.nan
    bad[17, 3] = np.inf
    bad[18, 7] = -np.inf
    bad[33, :13] = np.inf
    got = encode_host(bc, enc, bad, 1, np.float64, np.float64)
    ok = np.ones(n, dtype=bool)
    ok[[5, 17, 18, 33]] = False
    assert np.array_equal(got[ok], clean[ok])                    # the neighbours' bits are untouched
    assert np.all(np.isnan(got[5, :20])) and got[5, 20] == Z[5, 13]
    with np.errstate(invalid='ignore', over='ignore'):
        h = enc.host(bad[:, :13], dtype=np.float64)
    for r in (17, 18, 33):
        assert np.array_equal(np.isnan(got[r, :20]), np.isnan(h[r])), r
        assert np.array_equal(np.isinf(got[r, :20]), np.isinf(h[r])), r
        fin = np.isfinite(h[r])
        np.testing.assert_allclose(got[r, :20][fin], h[r][fin], rtol=1e-12, atol=1e-300)
    # a clean encode right after sees nothing of the infinities (no slot of the LDS panels is inherited)
    assert np.array_equal(encode_host(bc, enc, Z, 1, np.float64, np.float64), clean)


# ------------------------------------------------------------------ 2b. long walks: a block's second and third tile
# k_encode_mlp is persistent: block b walks the tiles b, b + B, b + 2 B, .. through the same two LDS panels.  At the sizes above
# every block sees one tile.  Here n = ES.long_walk_n: half of the B = n_cu * per_cu blocks make three trips, the rest two, and
# the short last tile is the third of its block.  One network per launch class (rows per tile, blocks per CU):
# tests/test_encode_shapes_cpu.py holds the list against the header.
CHUNK = 16384
PAIRS = [(np.float32, np.float64), (np.float64, np.float32), (np.float32, np.float32), (np.float64, np.float64)]      # (source, output)


def n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def chunks(n, step=CHUNK):
    for a in range(0, n, step):
        yield np.arange(a, min(n, a + step))


@functools.lru_cache(maxsize=2)
def long_case(k):
    """Network k of ES.LONG_NETS at its long-walk n: the encoder and the raw rows (float32 values, one pass-through column), on
    the host and resident as float32."""
    import beta_cores_amd as bc
    widths = ES.LONG_NETS[k]
    cu = n_cu()
    n = ES.long_walk_n(widths, cu)
    assert ES.trips(n, widths, cu) == 3 and ES.blocks(n, widths, cu) == cu * ES.per_cu(widths)
    rng = np.random.RandomState(2000 + k)
    enc = bc.encoders.MLPEncoder(make_layers(rng, widths))
    Z = rng.randn(n, widths[0] + 1).astype(np.float32)
    return dict(widths=widths, n=n, R=ES.tile_rows(widths), B=cu * ES.per_cu(widths), enc=enc, Z=Z, dd=bc.DeviceData(Z, dtype=np.float32))


def same_rows(a, b, n, skip=None, what=''):
    """Two resident row sets hold the same bits (NaNs included: compared as words), chunk by chunk; `skip`: rows left out."""
    for idx in chunks(n):
        if skip is not None:
            idx = idx[~skip[idx]]
        ra, rb = a.rows(idx), b.rows(idx)
        bad = np.flatnonzero((ra.view(np.int64) != rb.view(np.int64)).any(axis=1))
        assert bad.size == 0, (what, 'first differing row', int(idx[bad[0]]), 'of', int(bad.size))


def test_long_pairs_cover_every_dtype_pair():
    assert {PAIRS[k % 4] for k in range(len(ES.LONG_NETS))} == {(s, o) for s in DTYPES for o in DTYPES}


@pytest.mark.parametrize('k', range(len(ES.LONG_NETS)))
def test_long_walk_against_the_host_restatement(bc, k):
    """Every row of a three-trip launch within the bound e of the float64 restatement (one source / output pair per network, the
    pairs cycled over the list), pass-through columns bit-exact; the other pairs by the relations that hold at any n: a float32
    output is the float64 output rounded, and the source's storage type does not matter."""
    c = long_case(k)
    widths, n, enc, Z = c['widths'], c['n'], c['enc'], c['Z']
    d0, dl = widths[0], widths[-1]
    src_dtype, out_dtype = PAIRS[k % 4]
    srcs = {np.float32: c['dd'], np.float64: bc.DeviceData(Z.astype(np.float64))}
    outs = {(s, o): srcs[s].encode(enc, pass_cols=1, dtype=o) for s in DTYPES for o in DTYPES}
    for out in outs.values():
        assert out.shape == (n, dl + 1)
    worst, worst_allow = 0., 0.
    for idx in chunks(n):
        got = {key: out.rows(idx) for key, out in outs.items()}
        a = got[(np.float32, np.float64)]
        assert np.array_equal(got[(np.float64, np.float64)], a), int(idx[0])
        for s in DTYPES:
            assert np.array_equal(got[(s, np.float32)], a.astype(np.float32).astype(np.float64)), (s, int(idx[0]))
        h, e = enc.host(Z[idx, :d0].astype(np.float64), dtype=np.float64, bound=True)
        g = got[(src_dtype, out_dtype)]
        check_features(g[:, :dl], h, e, out_dtype, 'widths=%s rows %d..%d' % (widths, idx[0], idx[-1]))
        assert np.array_equal(g[:, dl:], Z[idx, d0:].astype(np.float64))
        worst = max(worst, np.abs(g[:, :dl] - h).max())
        worst_allow = max(worst_allow, e.max())
    print('long walk widths=%s n=%d R=%d B=%d %s->%s: max |device - restatement| %.3e, max e %.3e'
          % (widths, n, c['R'], c['B'], np.dtype(src_dtype).name, np.dtype(out_dtype).name, worst, worst_allow))


@pytest.mark.parametrize('k', range(len(ES.LONG_NETS)))
def test_long_walk_bits_do_not_depend_on_the_trip(bc, k):
    """The rows on both sides of every trip boundary, the 17 rows past the last full trip tile and 200 random rows: the bits of
    the three-trip launch are those of a launch that encodes just these rows, each block one tile."""
    c = long_case(k)
    n, R, B, enc, dd = c['n'], c['R'], c['B'], c['enc'], c['dd']
    rng = np.random.RandomState(3000 + k)
    idx = np.concatenate(([0, R * B - 1, R * B, 2 * R * B - 1, 2 * R * B, n - 1], np.arange(n - 17, n), rng.randint(n, size=200)))
    assert ES.trips(idx.size, c['widths'], n_cu()) == 1
    for out_dtype in DTYPES:
        whole = dd.encode(enc, dtype=out_dtype)
        alone = dd.take(idx).encode(enc, dtype=out_dtype)
        assert np.array_equal(alone.rows(np.arange(idx.size)).view(np.int64), whole.rows(idx).view(np.int64)), out_dtype


@pytest.mark.parametrize('k', range(len(ES.LONG_NETS)))
def test_long_walk_inherits_nothing_across_tiles(bc, k):
    """What test_nan_and_inf_rows cannot see in two one-tile launches: block t0 = 5 fills its panels with a tile of +inf rows,
    then with tile t0 + B (one all-NaN row), then with the clean tile t0 + 2 B.  Every row but the poisoned ones keeps the bits
    of the clean run -- no slot of a panel, padded or not, is read before this tile's own stage has written it."""
    c = long_case(k)
    widths, n, R, B, enc, Z = c['widths'], c['n'], c['R'], c['B'], c['enc'], c['Z']
    d0, dl = widths[0], widths[-1]
    src_dtype, out_dtype = PAIRS[k % 4]
    t0 = 5
    assert t0 + 2 * B < ES.ntiles(n, widths) and (t0 + 2 * B + 1) * R <= n      # the clean third tile exists and is full
    bad = Z.copy()
    bad[t0 * R:(t0 + 1) * R, :d0] = np.inf
    nan_row = (t0 + B) * R + 7
    bad[nan_row, :d0] = np.nan
    poisoned = np.zeros(n, dtype=bool)
    poisoned[t0 * R:(t0 + 1) * R] = True
    poisoned[nan_row] = True
    clean = bc.DeviceData(Z.astype(src_dtype), dtype=src_dtype).encode(enc, dtype=out_dtype)
    got = bc.DeviceData(bad.astype(src_dtype), dtype=src_dtype).encode(enc, dtype=out_dtype)
    same_rows(got, clean, n, skip=poisoned, what=widths)
    # the poisoned rows: the restatement's pattern of NaN and inf, its values where it is finite, the pass-through untouched
    pidx = np.flatnonzero(poisoned)
    rows = got.rows(pidx)
    with np.errstate(invalid='ignore', over='ignore'):
        h = enc.host(bad[pidx, :d0].astype(np.float64), dtype=np.float64)
    assert np.array_equal(np.isnan(rows[:, :dl]), np.isnan(h)) and np.array_equal(np.isinf(rows[:, :dl]), np.isinf(h))
    assert np.array_equal(np.signbit(rows[:, :dl])[np.isinf(h)], np.signbit(h)[np.isinf(h)])
    fin = np.isfinite(h)
    np.testing.assert_allclose(rows[:, :dl][fin], h[fin], rtol=1e-12 if out_dtype == np.float64 else 2.0 ** -23, atol=1e-300)
    assert np.isnan(rows[pidx == nan_row, :dl]).all()
    assert np.array_equal(rows[:, dl:], Z[pidx, d0:].astype(np.float64))


@pytest.mark.parametrize('k', range(len(ES.LONG_NETS)))
def test_long_walk_refills_a_buffer_across_sizes(bc, k):
    """encode(out=buf) at n = 40 -> long -> 40: the buffer grows and the grid goes from one block to B blocks and back; every
    result has the bits of a fresh encode."""
    c = long_case(k)
    widths, n, enc, Z = c['widths'], c['n'], c['enc'], c['Z']
    out_dtype = PAIRS[k % 4][1]
    w = widths[-1] + 1
    buf = bc.DeviceData(np.full((100, w), np.nan, dtype=out_dtype), dtype=out_dtype)
    for m, lo in ((40, 0), (n, 0), (40, 1000)):
        dd = c['dd'] if m == n else bc.DeviceData(Z[lo:lo + m], dtype=np.float32)
        got = dd.encode(enc, dtype=out_dtype, out=buf)
        assert got is buf and buf.shape == (m, w) and buf._transient
        same_rows(buf, dd.encode(enc, dtype=out_dtype), m, what=(widths, m))


def test_all_negative_preactivations_give_exact_zeros(bc):
    rng = np.random.RandomState(6)
    W = rng.randn(20, 13) * 0.01
    enc = bc.encoders.MLPEncoder([(W, np.full(20, -100.), None, None, True)])
    Z = rng.randn(50, 14).astype(np.float32)
    Z[7] = 0.                                                     # a zero row
    for out_dtype in DTYPES:
        got = encode_host(bc, enc, Z, 1, np.float32, out_dtype)
        assert np.array_equal(got[:, :20], np.zeros((50, 20))) and not np.signbit(got[:, :20]).any()
        assert np.array_equal(got[:, 20], Z[:, 13].astype(np.float64))


def test_a_refilled_buffer_shows_nothing_stale(bc):
    rng = np.random.RandomState(7)
    widths = (13, 20, 20)
    enc = bc.encoders.MLPEncoder(make_layers(rng, widths))
    for out_dtype in DTYPES:
        buf = bc.DeviceData(np.full((100, 21), np.nan, dtype=out_dtype), dtype=out_dtype)
        for n in (40, 300, 16):                                   # smaller than the buffer, larger (it grows), smaller again
            Z = rng.randn(n, 14).astype(np.float32)
            dd = bc.DeviceData(Z, dtype=np.float32)
            got = dd.encode(enc, dtype=out_dtype, out=buf)
            assert got is buf and buf.shape == (n, 21) and buf._transient
            rows = buf.rows(np.arange(n))
            assert np.isfinite(rows).all()
            assert np.array_equal(rows, dd.encode(enc, dtype=out_dtype).rows(np.arange(n)))


def test_refusals_leave_the_destination_untouched(bc):
    from beta_cores_amd import _native as N
    rng = np.random.RandomState(8)
    enc = bc.encoders.MLPEncoder(make_layers(rng, (13, 20, 20)))
    Z = rng.randn(30, 14).astype(np.float32)
    dd = bc.DeviceData(Z, dtype=np.float32)
    out = dd.encode(enc)
    want = out.rows(np.arange(30))

    def intact():
        return out.shape == (30, 21) and np.array_equal(out.rows(np.arange(30)), want)
    with pytest.raises(ValueError, match='source'):
        dd.encode(enc, out=dd)                                    # out is src
    assert dd.shape == (30, 14) and np.array_equal(dd.rows(np.arange(30)), Z.astype(np.float64)) and intact()
    with pytest.raises(ValueError, match='columns'):
        bc.DeviceData(rng.randn(5, 15)).encode(enc, out=out)      # source width is not d[0] + pass_cols
    with pytest.raises(ValueError, match='columns'):
        dd.encode(enc, pass_cols=0)
    with pytest.raises(ValueError, match='columns'):
        bc.DeviceData(rng.randn(5, 15)).encode(enc, pass_cols=2, out=out)      # destination width differs
    assert intact()
    with pytest.raises(ValueError, match='pass_cols'):
        dd.encode(enc, pass_cols=-1, out=out)
    with pytest.raises(ValueError, match='float64'):
        dd.encode(enc, dtype=np.float64, out=out)                 # the destination stores float32
    with pytest.raises(ValueError):
        dd.encode(enc, dtype=np.float16)
    assert intact()
    h = C.c_void_p(out.h.value)
    assert N.load().bc_data_encode(enc.h, dd.h, 1, 2, C.byref(h)) == N.BC_INVALID_ARGUMENT and 'out_elem_bytes' in N.last_error()
    other = bc.Context(device=bc.default_context().device)
    with pytest.raises(ValueError, match='context'):
        bc.DeviceData(Z, ctx=other, dtype=np.float32).encode(enc, out=out)
    assert intact()
    # a layer that was never set
    raw = C.c_void_p()
    w = np.array([13, 20, 20], dtype=np.int32)
    N.call('bc_encoder_create', bc.default_context().h, 2, w.ctypes.data_as(C.c_void_p), C.byref(raw))
    try:
        W0 = np.ascontiguousarray(rng.randn(20, 13))
        N.call('bc_encoder_set_layer', raw, 0, W0.ctypes.data_as(C.c_void_p), None, None, None, 1)
        h = C.c_void_p(out.h.value)
        assert N.load().bc_data_encode(raw, dd.h, 1, 4, C.byref(h)) == N.BC_INVALID_ARGUMENT
        assert 'layer 1' in N.last_error() and 'never set' in N.last_error()
        with pytest.raises(ValueError, match='layer 2'):
            N.call('bc_encoder_set_layer', raw, 2, W0.ctypes.data_as(C.c_void_p), None, None, None, 1)
    finally:
        N.call('bc_encoder_destroy', raw)
    assert intact()
    with pytest.raises(ValueError):
        bc.encoders.MLPEncoder(make_layers(rng, (13, 513)))
    with pytest.raises(ValueError):
        bc.encoders.MLPEncoder(make_layers(rng, (3, 3, 3, 3, 3, 3)))


def test_zero_rows(bc):
    rng = np.random.RandomState(9)
    enc = bc.encoders.MLPEncoder(make_layers(rng, (13, 20, 20)))
    dd = bc.DeviceData(rng.randn(10, 14))
    empty = dd.take([])
    got = empty.encode(enc)
    assert got.shape == (0, 21) and got.rows([]).shape == (0, 21)
    buf = dd.encode(enc)
    assert empty.encode(enc, out=buf) is buf and buf.shape == (0, 21)
    assert enc(np.zeros((0, 14))).shape == (0, 21)


# ------------------------------------------------------------------ 3. update, the projector's cache
def test_update_replaces_the_cached_copy(bc):
    rng = np.random.RandomState(10)
    widths, S, n = (13, 20, 20), 32, 700
    first, second = make_layers(rng, widths), make_layers(rng, widths)
    enc = bc.encoders.MLPEncoder(first)
    th = rng.randn(S, 20) * 0.3
    lik = bc.likelihoods.LinearRegression(1.0)
    prj = bc.DeviceProjector(fixed(th), S, lik, encoder=enc)
    plain = bc.DeviceProjector(fixed(th), S, lik)
    Z = rng.randn(n, 14).astype(np.float32)
    dd = bc.DeviceData(Z, dtype=np.float32)
    p1 = prj.project(dd).to_host()
    assert prj.encode_launches == 1 and enc.launches == 1
    assert np.array_equal(prj.project(dd).to_host(), p1) and np.array_equal(prj.colsum(dd), prj.project(dd).colsum())
    assert prj.encode_launches == 1 and enc.launches == 1         # an unchanged version re-uses the copy
    assert np.array_equal(p1, plain.project(dd.encode(enc)).to_host())
    v = enc.version
    enc.update(second)
    assert enc.version == v + 1
    p2 = prj.project(dd).to_host()
    assert prj.encode_launches == 2 and not np.array_equal(p1, p2)
    assert np.array_equal(p2, plain.project(dd.encode(enc)).to_host())
    assert np.array_equal(p2, plain.project(dd.encode(bc.encoders.MLPEncoder(second))).to_host())
    with pytest.raises(ValueError):
        enc.update(make_layers(rng, (13, 20, 21)))
    # a pinned array: its encoded copy goes when it is unpinned
    arr = rng.randn(500, 14).astype(np.float32)
    prj.pin(arr)
    before = prj.encode_launches
    a = prj.project(arr).to_host()
    assert np.array_equal(prj.project(arr).to_host(), a) and prj.encode_launches == before + 1
    assert len(prj._enc_cache) == 2
    prj.unpin(arr)
    assert len(prj._enc_cache) == 1
    assert np.array_equal(prj.project(arr).to_host(), a)          # (a live array again: uploaded and encoded per call)
    # transient rows are never cached
    buf = dd.take(np.arange(50), transient=True)
    before = prj.encode_launches
    b1 = prj.project(buf).to_host()
    dd.take(np.arange(50, 100), out=buf)
    b2 = prj.project(buf).to_host()
    assert prj.encode_launches == before + 2 and np.array_equal(b1, p2[:50]) and np.array_equal(b2, p2[50:100])
    with pytest.raises(ValueError, match='encoder'):
        prj.project(Z[:5], grad=True)


def test_from_torch_on_the_device(bc):
    import torch
    import torch.nn as nn
    torch.manual_seed(11)
    m = nn.Sequential(nn.Linear(13, 20), nn.BatchNorm1d(20), nn.ReLU(), nn.Linear(20, 20), nn.BatchNorm1d(20), nn.ReLU())
    m.train()
    m(torch.randn(64, 13) * 2 + 1)
    m.eval()
    enc = bc.encoders.MLPEncoder.from_torch(m)
    x = np.random.RandomState(11).randn(129, 13).astype(np.float32)
    got = encode_host(bc, enc, x, 0, np.float32, np.float64)
    h, e = enc.host(x, dtype=np.float64, bound=True)
    check_features(got, h, e, np.float64)
    with torch.no_grad():
        m[3].weight.mul_(1.5)
    enc.update_from_torch(m)
    got2 = encode_host(bc, enc, x, 0, np.float32, np.float64)
    h2, e2 = enc.host(x, dtype=np.float64, bound=True)
    assert not np.array_equal(got, got2)
    check_features(got2, h2, e2, np.float64)


def test_golden_f23_on_the_device(bc):
    """The reference's NeuralLinear feature extractor after a few optimize() epochs, eval mode: the device's features of the
    recorded input against torch's recorded float32 forward.  Allowed distance: the device's bound (u = 2^-53, plus the float32
    rounding of the stored result) plus torch's (the same recurrence at u = 2^-24)."""
    import torch.nn as nn
    import torch
    g = np.load(GOLDEN)
    m = nn.Sequential(nn.Linear(13, 20), nn.BatchNorm1d(20), nn.ReLU(), nn.Linear(20, 20), nn.BatchNorm1d(20), nn.ReLU())
    m.load_state_dict({k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith('sd_')})
    for i in (1, 4):
        m[i].eps = float(g['eps'])
    m.eval()
    enc = bc.encoders.MLPEncoder.from_torch(m)
    x, want = g['x'], g['features'].astype(np.float64)
    assert x.shape == (257, 13) and x.dtype == np.float32
    h, e64 = enc.host(x, dtype=np.float64, bound=True)
    _, e32 = enc.host(x, dtype=np.float64, bound=True, u=2.0 ** -24)
    for out_dtype in DTYPES:
        got = encode_host(bc, enc, x, 0, np.float32, out_dtype)
        check_features(got, h, e64, out_dtype, 'device vs host')
        allow = e64 + e32 + (ulp32(h) / 2. + 2.0 ** -150 if out_dtype == np.float32 else 0.)
        assert np.all(np.abs(got - want) <= allow), np.max(np.abs(got - want) - allow)
    # rows whose first-layer pre-activations are all negative: exact zeros inside, so all of them get one and the same feature row
    neg = g['all_negative_rows']
    dev = encode_host(bc, enc, x, 0, np.float32, np.float64)[neg]
    assert (want[neg] == want[neg[0]]).all() and (dev == dev[0]).all()


# ------------------------------------------------------------------ 4. projectors
@pytest.fixture(scope='module')
def problem(bc):
    rng = np.random.RandomState(12)
    n, S = 600, 32
    X = rng.randn(n, 13)
    y = np.tanh(X[:, 0]) + 0.5 * X[:, 1] + 0.3 * rng.randn(n)
    Z = np.hstack((X, y[:, None])).astype(np.float32)
    layers = make_layers(rng, (13, 20, 20))
    retrained = make_layers(rng, (13, 20, 20))
    th = rng.randn(S, 20) * 0.3
    return dict(n=n, S=S, Z=Z, layers=layers, retrained=retrained, th=th)


def test_projector_with_encoder_equals_projector_on_encoded_rows(bc, problem):
    from oracle import models_ref as M
    Z, th, S, n = problem['Z'], problem['th'], problem['S'], problem['n']
    sig, beta = 1.3, 0.2
    enc = bc.encoders.MLPEncoder(problem['layers'])
    lik = bc.likelihoods.LinearRegression(sig)
    dd = bc.DeviceData(Z, dtype=np.float32)
    ZE = dd.encode(enc)
    rows = ZE.rows(np.arange(n))                                   # the features the device produced: what the oracle sees
    rng = np.random.RandomState(13)
    core_idx = rng.randint(n, size=12)
    w = rng.rand(12)

    def close(dev, raw):
        ref = raw - raw.mean(axis=1)[:, None]
        np.testing.assert_allclose(dev, ref, rtol=0., atol=1e-11 * (1. + np.abs(raw).max()))
    for cls in (bc.DeviceProjector, bc.DeviceBetaProjector):
        pe, p0 = cls(fixed(th), S, lik, encoder=enc), cls(fixed(th), S, lik)
        a, b = pe.project(dd), p0.project(ZE)
        assert a.shape == (n, S) and np.array_equal(a.to_host(), b.to_host()) and np.array_equal(a.norms(), b.norms())
        raw_ll = M.linreg_loglik(rows, th, sig)
        close(a.to_host(), raw_ll)
        # host arrays (the upload slot; a live array) and a taken buffer go the same way
        assert np.array_equal(pe.project(Z[:100]).to_host(), b.to_host()[:100])
        assert np.array_equal(pe.project(Z.astype(np.float64)[:100]).to_host(), b.to_host()[:100])
        assert np.array_equal(pe.project(dd.take(core_idx)).to_host(), b.to_host()[core_idx])
        with pytest.raises(ValueError, match='columns'):
            pe.project(rows)                                       # encoded rows handed to an encoding projector
        betas = (None,) if cls is bc.DeviceProjector else (None, beta)
        for bt in betas:
            if bt is not None:
                af, bf = pe.project_f(dd, bt), p0.project_f(ZE, bt)
                assert np.array_equal(af.to_host(), bf.to_host())
                close(af.to_host(), M.linreg_beta_lik(rows, th, bt, sig))
            raw = raw_ll if bt is None else M.linreg_beta_lik(rows, th, bt, sig)
            cs_a, cs_b = pe.colsum(dd, beta=bt), p0.colsum(ZE, beta=bt)
            assert np.array_equal(cs_a, cs_b)
            np.testing.assert_allclose(cs_a, (raw - raw.mean(axis=1)[:, None]).sum(axis=0), rtol=0., atol=n * 1e-11 * (1. + np.abs(raw).max()))
            ga, ra = pe.vi_gradient(dd, Z[core_idx].astype(np.float64), w, 1.5, beta=bt, want_resid=True)
            gb, rb = p0.vi_gradient(ZE, rows[core_idx], w, 1.5, beta=bt, want_resid=True)
            assert np.array_equal(ga, gb) and np.array_equal(ra, rb)
            phi = raw - raw.mean(axis=1)[:, None]
            resid = 1.5 * phi.sum(axis=0) - w.dot(phi[core_idx])
            tol = 1.5 * n * 1e-11 * (1. + np.abs(raw).max())
            np.testing.assert_allclose(ra, resid, rtol=0., atol=tol)
            np.testing.assert_allclose(ga, -phi[core_idx].dot(resid) / S, rtol=0., atol=tol * np.abs(phi[core_idx]).sum(axis=1).max() / S + 1e-9)


# ------------------------------------------------------------------ 4b. projector routes at 4096 rows or more and at 65 536 or more
@pytest.fixture(scope='module')
def big_problem(bc):
    """The driver's network at its long-walk n (above projector._PIPE_ROWS): float32 rows, so a live array and a pinned one keep a
    float32 device copy."""
    from beta_cores_amd.coreset import projector as P
    rng = np.random.RandomState(16)
    widths = (13, 20, 20)
    n, S = ES.long_walk_n(widths, n_cu()), 32
    assert n >= P._PIPE_ROWS and P._SMALL_ROWS <= 5000 < P._PIPE_ROWS
    X = rng.randn(n, 13)
    y = np.tanh(X[:, 0]) + 0.5 * X[:, 1] + 0.3 * rng.randn(n)
    Z = np.hstack((X, y[:, None])).astype(np.float32)
    assert Z.base is None
    return dict(n=n, S=S, Z=Z, layers=make_layers(rng, widths), retrained=make_layers(rng, widths), th=rng.randn(S, 20) * 0.3)


def _same_phi(a, b, n, S):
    assert a.shape == (n, S) and b.shape == (n, S)
    assert np.array_equal(a.to_host(), b.to_host()) and np.array_equal(a.norms(), b.norms()) and np.array_equal(a.colsum(), b.colsum())


@pytest.mark.parametrize('cls_name', ['DeviceProjector', 'DeviceBetaProjector'])
def test_projector_routes_with_an_encoder_on_many_rows(bc, big_problem, cls_name):
    """encoder= on (a) the live host array (>= _PIPE_ROWS: upload, encode, bc_project -- not bc_project_from_host), (b) a live
    5000-row slice (between _SMALL_ROWS and _PIPE_ROWS), (c) the resident raw rows and (d) pinned rows, against the plain
    projector on the pre-encoded rows: the same bits everywhere, and encode_launches counts what the docstrings promise."""
    from oracle import models_ref as M
    Z, th, S, n = big_problem['Z'], big_problem['th'], big_problem['S'], big_problem['n']
    cls = getattr(bc, cls_name)
    sig, beta, m5 = 1.3, 0.2, 5000
    betas = (None,) if cls is bc.DeviceProjector else (None, beta)
    lik = bc.likelihoods.LinearRegression(sig)
    enc = bc.encoders.MLPEncoder(big_problem['layers'])
    dd = bc.DeviceData(Z, dtype=np.float32)
    ZE, ZE5 = dd.encode(enc), bc.DeviceData(Z[:m5], dtype=np.float32).encode(enc)
    rng = np.random.RandomState(17)
    core_idx = rng.randint(m5, size=12)
    w = rng.rand(12)
    core_raw = Z[core_idx].astype(np.float64)
    core_enc = ZE.rows(core_idx)
    p0 = cls(fixed(th), S, lik)

    def reference(data):
        out = {'project': p0.project(data)}
        for bt in betas:
            if bt is not None:
                out['project_f'] = p0.project_f(data, bt)
            out['colsum', bt] = p0.colsum(data, beta=bt)
            out['grad', bt] = p0.vi_gradient(data, core_enc, w, 1.5, beta=bt, want_resid=True)
        return out
    ref, ref5 = reference(ZE), reference(ZE5)

    def calls(pe, pts, want, rows):
        """Every entry point once; returns how many there were."""
        _same_phi(pe.project(pts), want['project'], rows, S)
        k = 1
        for bt in betas:
            if bt is not None:
                _same_phi(pe.project_f(pts, bt), want['project_f'], rows, S)
                k += 1
            assert np.array_equal(pe.colsum(pts, beta=bt), want['colsum', bt])
            g, r = pe.vi_gradient(pts, core_raw, w, 1.5, beta=bt, want_resid=True)
            assert np.array_equal(g, want['grad', bt][0]) and np.array_equal(r, want['grad', bt][1])
            k += 2
        return k

    # (a), (b): live arrays are uploaded and encoded for every call, and the encoded copy goes with the temporary rows
    for pts, want, rows in ((Z, ref, n), (Z[:m5], ref5, m5)):
        pe = cls(fixed(th), S, lik, encoder=enc)
        k = calls(pe, pts, want, rows)
        assert pe.encode_launches == k and len(pe._enc_cache) == 0
        assert calls(pe, pts, want, rows) == k and pe.encode_launches == 2 * k and len(pe._enc_cache) == 0
        assert pts.flags.writeable
    # (c), (d): one encode per version of the encoder, whatever is called and how often
    pe = cls(fixed(th), S, lik, encoder=enc)
    calls(pe, dd, ref, n)
    assert pe.encode_launches == 1 and len(pe._enc_cache) == 1
    pinned = pe.pin(Z)
    assert pinned.dtype == np.float32 and pe.pinned(Z) is pinned and not Z.flags.writeable
    try:
        calls(pe, Z, ref, n)
        calls(pe, Z, ref, n)
        calls(pe, dd, ref, n)
        assert pe.encode_launches == 2 and len(pe._enc_cache) == 2
        # a live array beside the resident entries: encoded per call, nothing of it stays
        before = pe.encode_launches
        k = calls(pe, Z[:m5], ref5, m5)
        assert pe.encode_launches == before + k and len(pe._enc_cache) == 2
        # retrained parameters: each resident row set is encoded once more, at its next use
        v = enc.version
        enc.update(big_problem['retrained'])
        assert enc.version == v + 1
        ZE2 = dd.encode(enc)
        core_enc = ZE2.rows(core_idx)
        ref2 = reference(ZE2)
        assert not np.array_equal(ref2['colsum', None], ref['colsum', None])
        calls(pe, dd, ref2, n)
        assert pe.encode_launches == before + k + 1
        calls(pe, dd, ref2, n)
        calls(pe, Z, ref2, n)
        calls(pe, Z, ref2, n)
        assert pe.encode_launches == before + k + 2 and len(pe._enc_cache) == 2
    finally:
        pe.unpin(Z)
    assert len(pe._enc_cache) == 1 and Z.flags.writeable
    # ... and the oracle on the device's own features, once per class (after the update: the retrained network's)
    rows = ZE2.rows(np.arange(n))

    def close(dev, raw):
        np.testing.assert_allclose(dev, raw - raw.mean(axis=1)[:, None], rtol=0., atol=1e-11 * (1. + np.abs(raw).max()))
    raw_ll = M.linreg_loglik(rows, th, sig)
    close(ref2['project'].to_host(), raw_ll)
    for bt in betas:
        raw = raw_ll
        if bt is not None:
            raw = M.linreg_beta_lik(rows, th, bt, sig)
            close(ref2['project_f'].to_host(), raw)
        phi = raw - raw.mean(axis=1)[:, None]
        np.testing.assert_allclose(ref2['colsum', bt], phi.sum(axis=0), rtol=0., atol=n * 1e-11 * (1. + np.abs(raw).max()))
        ga, ra = ref2['grad', bt]
        resid = 1.5 * phi.sum(axis=0) - w.dot(phi[core_idx])
        tol = 1.5 * n * 1e-11 * (1. + np.abs(raw).max())
        np.testing.assert_allclose(ra, resid, rtol=0., atol=tol)
        np.testing.assert_allclose(ga, -phi[core_idx].dot(resid) / S, rtol=0., atol=tol * np.abs(phi[core_idx]).sum(axis=1).max() / S + 1e-9)


def test_a_shard_keeps_its_row_offset_through_the_encoder(bc, big_problem):
    """Rows a:b of a larger set: the encoded rows and the Phi projected from them through encoder= carry row_offset a and the
    bits of rows a:b of the unsharded projection."""
    Z, th, S, n = big_problem['Z'], big_problem['th'], big_problem['S'], big_problem['n']
    a, b = 128 * 517, 128 * 517 + 9001
    assert b < n
    lik = bc.likelihoods.LinearRegression(1.0)
    enc = bc.encoders.MLPEncoder(big_problem['layers'])
    shard = bc.DeviceData(Z[a:b], dtype=np.float32, row_offset=a)
    se = shard.encode(enc)
    assert se.row_offset == a and shard.encode(enc, dtype=np.float64, out=bc.DeviceData(np.zeros((1, 21)))).row_offset == a
    whole = bc.DeviceData(Z, dtype=np.float32)
    assert np.array_equal(se.rows(np.arange(b - a)), whole.encode(enc).rows(np.arange(a, b)))
    for cls in (bc.DeviceProjector, bc.DeviceBetaProjector):
        pe = cls(fixed(th), S, lik, encoder=enc)
        full = pe.project(whole)
        part = pe.project(shard)
        assert full.row_offset == 0 and part.row_offset == a and part.shape == (b - a, S)
        assert np.array_equal(part.to_host(), full.to_host()[a:b]) and np.array_equal(part.norms(), full.norms()[a:b])
        assert np.array_equal(part.to_host(), cls(fixed(th), S, lik).project(se).to_host())
        # the arg-max speaks global row numbers
        resid = np.random.RandomState(18).randn(S)
        best, _ = part.argmax(resid, mode=1, post_div=float(S))
        assert a <= best < b


# ------------------------------------------------------------------ 5. coresets on raw resident rows
def _initial(problem, ZE_rows):
    idcs0 = np.arange(0, 100, 10)
    return idcs0, np.ones(10), ZE_rows[idcs0]


@pytest.mark.parametrize('kind', ['bcores', 'svi'])
@pytest.mark.parametrize('mode', ['groups', 'fused', 'materialising'])
def test_greedy_vi_on_raw_rows_equals_the_pre_encoded_run(bc, problem, kind, mode):
    """The driver's arguments (groups of 20, an initial set of 10, initialized=True, sub-sampled selection and optimisation)
    with encoder=enc on the RAW resident rows against the same class on the pre-encoded rows; one retraining in between."""
    Z, th, S, n = problem['Z'], problem['th'], problem['S'], problem['n']
    lik = bc.likelihoods.LinearRegression(1.0)
    groups = [list(range(g * 20, (g + 1) * 20)) for g in range(n // 20)]
    idcs0 = np.arange(0, 100, 10)

    def run(encoded):
        enc = bc.encoders.MLPEncoder(problem['layers'])
        dd = bc.DeviceData(Z, dtype=np.float32)
        if kind == 'bcores':
            pcls, ccls, kw = bc.DeviceBetaProjector, bc.BetaCoreset, dict(beta=0.2, learn_beta=False)
        else:
            pcls, ccls, kw = bc.DeviceProjector, bc.SparseVICoreset, {}
        if mode == 'groups':
            kw.update(groups=groups, n_subsample_select=10, n_subsample_opt=10)
        else:
            kw.update(n_subsample_select=150, n_subsample_opt=60, fused_gradient=(mode == 'fused'))
        out = []
        data = dd
        for build in range(2):
            if encoded:
                data = dd.encode(enc)
                prj = pcls(fixed(th), S, lik)
            elif build == 0:
                prj = pcls(fixed(th), S, lik, encoder=enc)
            pts0 = data.rows(idcs0)
            np.random.seed(40 + build)
            alg = ccls(data, prj, opt_itrs=6, step_sched=lambda i: 0.1 / (1. + i), initialized=True, wts=np.ones(10), idcs=idcs0.copy(),
                       pts=pts0, **kw)
            alg.build(3, 200)
            got = alg.get()
            out.append((got[0].copy(), got[1].copy(), got[2].copy(), list(alg.selected_groups), np.random.get_state()[1].copy()))
            enc.update(problem['retrained'])                       # "nl.optimize(...)": the second build sees new features
        return out
    raw, pre = run(False), run(True)
    for build in range(2):
        a, b = raw[build], pre[build]
        assert np.array_equal(a[2], b[2]) and a[3] == b[3], (build, a[2], b[2])
        assert np.array_equal(a[0], b[0]), build
        assert np.array_equal(a[4], b[4])
        assert a[1].shape[1] == 14 and np.array_equal(a[1], Z[a[2]].astype(np.float64))      # get() speaks RAW rows
        assert len(a[2]) > 10 or mode != 'groups'


def test_hilbert_and_uniform_on_raw_rows(bc, problem):
    Z, th, S, n = problem['Z'], problem['th'], problem['S'], problem['n']
    lik = bc.likelihoods.LinearRegression(1.0)
    enc = bc.encoders.MLPEncoder(problem['layers'])
    dd = bc.DeviceData(Z, dtype=np.float32)
    out = []
    for data, prj in ((dd, bc.DeviceProjector(fixed(th), S, lik, encoder=enc)), (dd.encode(enc), bc.DeviceProjector(fixed(th), S, lik))):
        np.random.seed(14)
        alg = bc.HilbertCoreset(data, prj, n_subsample=200)
        alg.build(15, 15)
        out.append(alg.get())
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][2], out[1][2]) and len(out[0][2]) > 3
    assert np.array_equal(out[0][1], Z[out[0][2]].astype(np.float64)) and out[1][1].shape[1] == 21
    # the RAND baseline holds raw resident rows, by rows and by groups
    groups = [list(range(g * 20, (g + 1) * 20)) for g in range(n // 20)]
    idcs0 = np.arange(0, 100, 10)
    for g in (None, groups):
        np.random.seed(15)
        alg = bc.UniformSamplingCoreset(dd, groups=g, wts=np.ones(10), idcs=idcs0.copy(), pts=dd.rows(idcs0))
        alg.build(5, 400)
        wts, pts, idcs = alg.get()
        assert len(idcs) > 10 and np.array_equal(pts, Z[idcs].astype(np.float64))
