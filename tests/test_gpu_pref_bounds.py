"""The pre-filter's bounds, row by row, on the device (include/beta_cores_prefdiag.h; reference, checker and cases:
tests/pref_cases.py).  The other pre-filter tests compare one row per sweep -- the argmax -- with the fp64 path's; an unsound
bound changes that row only when the winner's own interval is violated by more than its margin.  Here every link of the chain
behind "by construction" is held to the exact scores for EVERY row:

  * the mirrors all six builders wrote (k_build_i8, k_build_i8_r<104>, k_build_i4, k_build_r8, k_build_u16, k_build_u32);
  * the digit records of the vectors actually swept;
  * the intervals of k_sweep_i8 and of both levels of k_sweep_i4 (their DUMP instances: the production kernels' code plus
    stores) on the solver's own vectors after 0, 1 and 12 steps and on the adversarial vectors of every case, containment and
    tightness; theta0; the two-level form's lists; level 2 bit-equal to the one-level sweep;
  * the per-row values against what the PRODUCTION sweep of the same state leaves in its tile and block lists (bit-exact);
  * walks of several tiles per wave, and of more than BC_IFLUSH;
  * the fp32 / fp16 mirrors from the buffers they write;
  * the diagnostic leaves the solver as found, and refuses what it documents.
Each test prints the worst |centre - f| / half-width it met (1 = the end of an interval) and the attainment of the targeted row."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pref_cases as P                                                      # noqa: E402
import pref_model as M                                                      # noqa: E402
from test_gpu_prefilter import correlated, prefilter, same                 # noqa: E402

pytestmark = pytest.mark.gpu
INFO = ['prec', 'ptile', 'ptiles', 'sp', 'sp4', 'sp8', 'g4', 'rb', 'i4_u', 'grid', 'grid1', 'two', 'two_active', 'iflush', 'blk_nc', 'next_form',
        'qv', 'seeds', 'hot', 'spill_cap']


@pytest.fixture(scope='module')
def bc():
    import beta_cores_amd as bc
    bc.default_context()
    return bc


def native():
    from beta_cores_amd import _native as N
    return N


def info(sv):
    out = (C.c_int64 * len(INFO))()
    native().call('bc_snnls_prefdiag_info', sv._eng.h, out)
    return dict(zip(INFO, [int(x) for x in out]))


def fetch(sv, which, dtype):
    N = native()
    nb = C.c_int64()
    assert N.load().bc_snnls_prefdiag_copy(sv._eng.h, which.encode(), None, 0, C.byref(nb)) == N.BC_INVALID_ARGUMENT and nb.value > 0, which
    buf = np.empty(nb.value, dtype=np.uint8)
    N.call('bc_snnls_prefdiag_copy', sv._eng.h, which.encode(), buf.ctypes.data_as(C.c_void_p), nb.value, None)
    return buf.view(dtype)


def sweep(sv, mode, v=None, pd=1.0, selfq=0):
    """(form run, ul [rows][2], ul8 or None, theta0 or None)"""
    i = info(sv)
    rows = i['ptiles'] * 256
    ul = np.empty((rows, 2), dtype=np.float32)
    ul8 = np.empty((rows, 2), dtype=np.float32)
    th = np.empty(max(1, i['grid1']), dtype=np.float32)
    form = C.c_int32()
    vp = None if v is None else np.ascontiguousarray(v, dtype=np.float64).ctypes.data_as(C.c_void_p)
    native().call('bc_snnls_prefdiag_sweep', sv._eng.h, mode, vp, float(pd), selfq, ul.ctypes.data_as(C.c_void_p), ul8.ctypes.data_as(C.c_void_p),
                  th.ctypes.data_as(C.c_void_p), rows, len(th), C.byref(form))
    return form.value, ul, (ul8 if form.value == 3 else None), (th[:i['grid1']] if form.value == 3 else None)


def solver(bc, phi, form, alg='giga', two_pass=False):
    cls = bc.snnls.GIGA if alg == 'giga' else bc.snnls.FrankWolfe
    old = os.environ.get('BC_BUILD_I8_TWO_PASS')
    if two_pass:
        os.environ['BC_BUILD_I8_TWO_PASS'] = '1'
    try:
        with prefilter(form):
            sv = cls(phi.T, P.finite_b(phi), allow_zero_rows=True)
    finally:
        if two_pass:
            if old is None:
                os.environ.pop('BC_BUILD_I8_TWO_PASS', None)
            else:
                os.environ['BC_BUILD_I8_TWO_PASS'] = old
    return sv


def mirrors(sv, phi):
    """The snapshot of a solver's mirrors (no vectors yet)."""
    i = info(sv)
    n, S = phi.shape
    rows = i['ptiles'] * 256
    norms = np.zeros(rows)
    norms[:n] = sv._eng.phi.norms()
    s = M.Snap(S=S, n=n, phi=phi, norms=norms, ptiles=i['ptiles'], sp4=i['sp4'], two=bool(i['two']), info=i)
    s.u8, s.rowq = fetch(sv, 'u8', np.int32), fetch(sv, 'rowq', np.uint16)
    if i['two']:
        s.sp8, s.g4, s.rb, s.i4_u = i['sp8'], i['g4'], i['rb'], i['i4_u']
        assert (s.i4_u, s.sp8, s.rb) == (M.lay_i4_batch(S), M.lay_i4_sp8(S, M.lay_i4_batch(S)), M.lay_r8_bytes(S))
        s.u4, s.rowq4, s.r8 = fetch(sv, 'u4', np.int32), fetch(sv, 'rowq4', np.uint16), fetch(sv, 'r8', np.uint8)
    assert s.sp4 == M.lay_i8_sp4(S) and s.ptiles == M.lay_i8_tiles(n)
    return s


def quantised(s, mode, v):
    """The digit records of a vector the diagnostic quantised itself are not downloadable: they are held to the model's, whose
    arithmetic is the device's (bc_i8q_wave / bc_i4q_wave: fp64, no fma), and then to the checker like any record."""
    s.qv = M.quant_i8(v, s.S, mode)
    if s.two:
        s.qv4 = M.quant_i4(v, s.S, mode)


def report(tag, stats, row=None):
    parts = []
    for lvl, st in stats.items():
        t = '%s worst %.4f (%d rows, %d uncertain)' % (lvl, st['worst'], st['rows'], st['uncertain'])
        if row is not None and 'attain_rows' in st:
            t += ' attained %.4f' % st['attain_rows'][row]
        parts.append(t)
    print('%s: %s' % (tag, '; '.join(parts)))


# ------------------------------------------------------------------ mirrors and adversarial vectors, every case matrix
@pytest.mark.parametrize('S,n', P.case_list(), ids=lambda x: str(x))
def test_mirrors_and_adversarial_vectors(bc, S, n):
    phi = np.array(P.case_phi(S, n))
    sv4 = solver(bc, phi, 4)                                   # two-level (S <= 256): k_build_i8_r / k_build_i8, k_build_i4, k_build_r8
    sv8 = solver(bc, phi, 8, two_pass=(S <= 104))              # one-level; for S <= 104 through the OTHER int8 builder
    s4, s8 = mirrors(sv4, phi), mirrors(sv8, phi)
    assert s4.two == (S <= 256) and not s8.two
    assert np.array_equal(s4.u8, s8.u8) and np.array_equal(s4.rowq, s8.rowq)      # both int8 builders: byte-equal mirrors
    memo4, memo8 = {}, {}
    if s4.two:
        native().call('bc_snnls_select_local', sv4._eng.h)     # the first sweep of a solver is the int8 one and leaves the seeds
        assert info(sv4)['next_form'] == 3
    for name, mode, v, pd, term, row in P.case_vectors(S, n):
        for s, sv, memo in ((s4, sv4, memo4), (s8, sv8, memo8)):
            form, ul, ul8, th = sweep(sv, mode, v, pd)
            assert form == (3 if s.two else 1)
            s.update(mode=mode, post_div=pd, v=np.asarray(v, dtype=np.float64))
            quantised(s, mode, v)
            s.ul_i8, s.ul_i4, s.ul8, s.theta0 = (None, ul, ul8, th) if form == 3 else (ul, None, None, None)
            report('S %d n %d %s form %d' % (S, n, name, form), P.check_all(s, memo=memo), row)
            if form == 3:
                l2 = ul8
        if s4.two:                                             # level 2 = the one-level sweep, bit for bit, on the rows it re-bounded
            done = ~np.isnan(l2[:, 0])
            assert done.any() and np.array_equal(l2[done].view(np.uint32), s8.ul_i8[done].view(np.uint32)), name
        # the one-level sweep quantising v in its own prologue: the same digits, hence the same bits
        form, ul, _, _ = sweep(sv8, mode, v, pd, selfq=1)
        assert form == 1 and np.array_equal(ul.view(np.uint32), s8.ul_i8.view(np.uint32)), name


# ------------------------------------------------------------------ the solver's own vectors
def own_vectors(sv, s, mode):
    s.update(mode=mode, post_div=1.0, v=fetch(sv, 'v', np.float64), qv=fetch(sv, 'qv', np.int32))
    if s.two:
        s.qv4 = fetch(sv, 'qv4', np.int32)
    assert fetch(sv, 'post_div', np.float64)[0] == 1.0
    if mode == 1:
        vn = fetch(sv, 'v_norm', np.float64)[0]
        assert abs(vn - np.linalg.norm(s.v)) <= 1e-12 * vn


def blocks_of(i, form):
    """tile -> sweep block: wave w of block b walks tiles 4 b + w, + 4 grid, ..."""
    grid = i['grid1'] if form == 3 else i['grid']
    return (np.arange(i['ptiles']) // 4) % grid, grid


def check_lists_two_level(sv, s, i, ul, ul8, th):
    """The two-level form's outputs against the per-row values: every row whose exact score reaches the best block bound was
    re-bounded and is listed; every listed (U, row) has U >= f(row); and the lists are what the per-row values imply.  (A block
    with more than BC_BLK_NC rows in play says -1 and hands its pairs to the spill list, whose count the rescoring stage clears.)"""
    blk_l, blk_u = fetch(sv, 'l2_blk_l', np.float64), fetch(sv, 'l2_blk_u', np.float32)
    nc, cand = fetch(sv, 'l2_blk_nc', np.int32), fetch(sv, 'l2_blk_cand', np.int32).reshape(-1, i['blk_nc'], 2)
    f = s['_exact'][0].astype(np.float64)
    done = ~np.isnan(ul8[:, 0])
    blk, grid = blocks_of(i, 3)
    rb = np.repeat(blk, 256)
    listed = {}
    for b in range(grid):
        rows_b = done & (rb == b)
        best = np.max(ul8[rows_b, 1]) if rows_b.any() else -np.inf
        assert blk_l[b] == np.float64(best), b                                   # maxima of floats are exact
        assert blk_u[b] == (np.max(ul8[rows_b, 0]) if rows_b.any() else np.float32(-np.inf)), b
        want = set((int(ul8[r, 0].view(np.uint32)), int(r)) for r in np.nonzero(rows_b & (ul8[:, 0] >= best))[0])
        assert nc[b] >= -1, 'block %d gave up' % b
        if nc[b] >= 0:
            got = set((int(np.uint32(u)), int(r)) for u, r in cand[b, :nc[b]])
            assert got == want, b
            listed.update((r, u) for u, r in got)
        else:
            assert len(want) > i['blk_nc']
    top = np.max(blk_l)
    live = s.norms != 0
    must = live & np.isfinite(f) & (f >= top)
    assert np.all(done[must]), 'a row whose exact score reaches max blk_l was not re-bounded'
    for r in np.nonzero(must)[0]:
        b = rb[r]
        assert nc[b] == -1 or int(r) in listed, r
    for r, u in listed.items():
        assert np.uint32(u).view(np.float32) >= f[r] or np.isnan(f[r]), r


def lists_one_level(sv):
    """What the last one-level sweep left (the diagnostic sweep writes the same buffers: fetch a production sweep's first)."""
    return (fetch(sv, 'tile_u', np.float32), fetch(sv, 'tile_ncand', np.int32), fetch(sv, 'tile_cand', np.float32).reshape(-1, 4, 2),
            fetch(sv, 'blk_l', np.float64), fetch(sv, 'blk_u', np.float32))


def check_lists_one_level(lists, i, ul):
    """tile_u, tile_ncand, tile_cand, blk_l, blk_u of a PRODUCTION sweep are what the dumped per-row values imply, bit-exact."""
    tile_u, ncand, tcand, blk_l, blk_u = lists
    U, L = ul[:, 0].reshape(-1, 256), ul[:, 1].reshape(-1, 256)
    assert np.array_equal(tile_u.view(np.uint32), U.max(axis=1).view(np.uint32))
    tl = L.max(axis=1)
    c = (U >= tl[:, None]) & (U != -np.inf)
    assert np.array_equal(ncand, c.sum(axis=1))
    order = np.argsort((np.arange(256) % 4) * 64 + np.arange(256) // 4, kind='stable')      # slots fill by (j, lane), row = 4 lane + j
    for t in range(len(tile_u)):
        rows = [r for r in order if c[t, r]][:4]
        for k, r in enumerate(rows):
            assert tcand[t, k, 0].view(np.uint32) == U[t, r].view(np.uint32) and tcand[t, k, 1] == np.float32(r), (t, k)
    blk, grid = blocks_of(i, 1)
    for b in range(grid):
        m = blk == b
        assert blk_l[b] == (np.float64(tl[m].max()) if m.any() else -np.inf), b
        assert blk_u[b] == (tile_u[m].max() if m.any() else np.float32(-np.inf)), b


def take_steps(sv, steps):
    """`steps` greedy steps through the step entry points of the fused loop, WITHOUT the end of the build call: there the host's
    watch (bc_pref_adapt) looks at the share of rows the 4-bit level passed on, and on a few thousand rows it puts the first
    level aside after a handful of steps -- the sweeps the steps took would no longer be the one the diagnostic runs next.
    finish_steps() ends the call."""
    N = native()
    if steps:
        N.call('bc_snnls_build_begin', sv._eng.h, steps)
        for _ in range(steps):
            N.call('bc_snnls_step_local', sv._eng.h)
            N.call('bc_snnls_step_finish', sv._eng.h)


def finish_steps(sv, steps):
    N = native()
    lim, done, pending = C.c_int(), C.c_int(), C.c_int()
    N.call('bc_snnls_build_end', sv._eng.h, C.byref(lim), C.byref(done), C.byref(pending))
    assert done.value == steps and not pending.value and not lim.value


@pytest.mark.parametrize('steps', [0, 1, 12])
@pytest.mark.parametrize('alg', ['giga', 'fw'])
def test_production_vectors(bc, alg, steps):
    """The solver's own vectors and digit records after 0, 1 and 12 steps: every row of both forms; the two-level form's theta0
    and lists; level 2 against the one-level sweep of a second solver in the same state; then the production sweep's own
    outputs (bc_snnls_select_local on the same state) against the per-row values."""
    rng = np.random.RandomState(11)
    S, n = 100, 3001
    phi = correlated(rng, n, S)
    mode = 0 if alg == 'giga' else 1
    sv4, sv8 = solver(bc, phi, 4, alg), solver(bc, phi, 8, alg)
    s4, s8 = mirrors(sv4, phi), mirrors(sv8, phi)
    for sv in (sv4, sv8):
        take_steps(sv, steps)
    tr4, tr8 = sv4._eng.trace(), sv8._eng.trace()
    assert all(np.array_equal(a, b) for a, b in zip(tr4, tr8))                 # the same state: bit-identical traces
    out = {}
    for s, sv in ((s4, sv4), (s8, sv8)):
        i = info(sv)
        own_vectors(sv, s, mode)
        form, ul, ul8, th = sweep(sv, mode)
        assert form == (3 if (s.two and steps) else 1)
        s.ul_i8, s.ul_i4, s.ul8, s.theta0 = (None, ul, ul8, th) if form == 3 else (ul, None, None, None)
        report('%s %d steps form %d' % (alg, steps, form), P.check_all(s))
        out[sv] = (form, ul, ul8)
        if form == 3:
            check_lists_two_level(sv, s, i, ul, ul8, th)
    assert np.array_equal(s4.v, s8.v) and np.array_equal(s4.qv, s8.qv)
    form, ul, ul8 = out[sv4]
    if form == 3:
        done = ~np.isnan(ul8[:, 0])
        assert done.any() and np.array_equal(ul8[done].view(np.uint32), out[sv8][1][done].view(np.uint32))
    # DUMP agrees with production.  One-level: the production sweep first (bc_snnls_select_local prepares the vectors -- a fresh
    # solver's are still zero -- and sweeps), its lists put aside, then the per-row values of the same vectors.  Two-level: the
    # per-row values first (the diagnostic restored the seeds), then the production sweep from the same seeds.
    for s, sv in ((s4, sv4), (s8, sv8)):
        form, ul, ul8 = out[sv]
        native().call('bc_snnls_select_local', sv._eng.h)
        if form == 3:
            check_lists_two_level(sv, s, info(sv), ul, ul8, None)
            continue
        lists = lists_one_level(sv)
        own_vectors(sv, s, mode)
        assert np.any(s.v != 0.)
        form2, ul, ul8, th = sweep(sv, mode)
        s.ul_i8, s.ul_i4, s.ul8, s.theta0 = (None, ul, ul8, th) if form2 == 3 else (ul, None, None, None)
        report('%s %d steps, prepared vectors, form %d' % (alg, steps, form2), P.check_all(s))
        if form2 == 1:
            check_lists_one_level(lists, info(sv), ul)
        else:                                                  # (the fresh two-level solver's first sweep was the int8 one: now it has seeds)
            check_lists_two_level(sv, s, info(sv), ul, ul8, th)
    for sv in (sv4, sv8):
        finish_steps(sv, steps)


# ------------------------------------------------------------------ long walks
def n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize('tiles_per_wave,S', [(3, 8), (33, 5)])
def test_long_walks(bc, monkeypatch, tiles_per_wave, S):
    """One wave per CU: 3 tiles per wave, and more than BC_IFLUSH = 32 (the wave flushes its parked results in the middle of its
    walk).  Per-row containment and tightness of the one-level sweep, and the production sweep's lists against them; the
    two-level form's per-row values at 3 tiles per wave."""
    monkeypatch.setenv('BC_PREF_WAVES_PER_CU', '1')
    cu = n_cu()
    n = 256 * tiles_per_wave * cu - 100
    rng = np.random.RandomState(tiles_per_wave)
    phi = correlated(rng, n, S)
    forms = (8, 4) if tiles_per_wave == 3 else (8,)
    for want in forms:
        sv = solver(bc, phi, want, 'fw')
        i = info(sv)
        assert -(-i['ptiles'] // (4 * i['grid'])) == tiles_per_wave and (tiles_per_wave > i['iflush']) == (S == 5)
        sv.build(2)
        s = mirrors(sv, phi)
        own_vectors(sv, s, 1)
        form, ul, ul8, th = sweep(sv, 1)
        assert form == (3 if want == 4 else 1)
        s.ul_i8, s.ul_i4, s.ul8, s.theta0 = (None, ul, ul8, th) if form == 3 else (ul, None, None, None)
        report('%d tiles per wave, form %d' % (tiles_per_wave, form), P.check_all(s, skip=('mirror',)))
        if form == 1:                                          # (the same vectors: select_local prepares them again from the same state)
            native().call('bc_snnls_select_local', sv._eng.h)
            check_lists_one_level(lists_one_level(sv), i, ul)


# ------------------------------------------------------------------ fp32 / fp16 mirrors (download only)
@pytest.mark.parametrize('prec', [32, 16])
@pytest.mark.parametrize('S,n', [(37, 3001), (8, 257), (105, 300)])
def test_float_mirrors(bc, prec, S, n):
    phi = np.array(P.case_phi(S, n))
    ok = np.all(np.isfinite(phi), axis=1)
    phi[~ok] = 0.                                              # (these forms have no "uncertain" rows: NaN rows become zero rows)
    sv = solver(bc, phi, prec, 'fw')
    i = info(sv)
    assert i['prec'] == prec and i['ptile'] == (256 if prec == 32 else 512)
    norms = np.zeros(i['ptiles'] * i['ptile'])
    norms[:n] = sv._eng.phi.norms()
    live = norms != 0
    u = np.zeros((len(norms), S))
    u[:n][live[:n]] = phi[live[:n]] / norms[:n][live[:n], None]
    if prec == 32:
        got = fetch(sv, 'u32', np.float32).reshape(i['ptiles'], S, 256).transpose(0, 2, 1).reshape(-1, S)
        assert np.array_equal(got, u.astype(np.float32))
    else:
        got = fetch(sv, 'u16', np.float16).reshape(i['ptiles'], i['sp'], 512).transpose(0, 2, 1).reshape(-1, i['sp'])
        assert np.array_equal(got[:, :S], u.astype(np.float32).astype(np.float16)) and not got[:, S:].any()
        bits = np.unpackbits(fetch(sv, 'live', np.uint8), bitorder='little')
        assert np.array_equal(bits.astype(bool), live)
    native().call('bc_snnls_select_local', sv._eng.h)
    v = fetch(sv, 'v', np.float64)
    f = (u.astype(np.longdouble).dot(v.astype(np.longdouble))).astype(np.float64)
    tile_u, blk_l = fetch(sv, 'tile_u', np.float32), fetch(sv, 'blk_l', np.float64)
    ft = np.where(live, f, -np.inf).reshape(-1, i['ptile'])
    assert np.all(tile_u >= ft.max(axis=1))
    assert blk_l.max() <= ft.max()
    if prec == 32:
        ub = fetch(sv, 'ub', np.float32)
        assert np.all(ub[live] >= f[live]) and np.all(ub[~live] == -np.inf)


# ------------------------------------------------------------------ state and refusals
@pytest.mark.parametrize('form', [8, 4])
@pytest.mark.parametrize('alg', ['giga', 'fw'])
def test_leaves_the_solver_as_found(bc, alg, form):
    rng = np.random.RandomState(23)
    phi = correlated(rng, 3001, 65)
    res = []
    for probe in (True, False):
        sv = solver(bc, phi, form, alg)
        sv.build(6)
        if probe:
            mode = 0 if alg == 'giga' else 1
            sweep(sv, mode)
            sweep(sv, 1, rng.randn(65))
            g = rng.randn(65, 2)
            sweep(sv, 0, (g / np.linalg.norm(g, axis=0)).reshape(-1))
            sweep(sv, mode)
        sv.build(6)
        idx, val = sv._eng.sparse_weights()
        res.append(((sv._eng.trace(), idx, val, sv.error()), sv._eng.prefilter_stats(), sv._eng.prefilter_levels(),
                    fetch(sv, 'hot', np.int64).copy() if form == 4 else None, fetch(sv, 'ctrl', np.int32).copy()))
    same(res[0][0], res[1][0])
    assert res[0][1] == res[1][1] and res[0][2] == res[1][2]
    assert np.array_equal(res[0][4], res[1][4]) and (form == 8 or np.array_equal(res[0][3], res[1][3]))


def test_refusals(bc):
    N = native()
    lib = N.load()
    rng = np.random.RandomState(3)
    phi = correlated(rng, 300, 37)
    sv = solver(bc, phi, 4)
    h = sv._eng.h
    rows = info(sv)['ptiles'] * 256
    ul = np.empty((rows, 2), dtype=np.float32)
    p = ul.ctypes.data_as(C.c_void_p)
    form = C.c_int32()
    nb = C.c_int64()
    buf = np.empty(16, dtype=np.uint8)

    def refused(rc, word):
        assert rc == N.BC_INVALID_ARGUMENT and word in N.last_error(), (rc, N.last_error())
    refused(lib.bc_snnls_prefdiag_copy(h, b'nonsense', buf.ctypes.data_as(C.c_void_p), 16, None), 'unknown buffer')
    refused(lib.bc_snnls_prefdiag_copy(h, b'u16', buf.ctypes.data_as(C.c_void_p), 16, None), 'has no buffer')
    refused(lib.bc_snnls_prefdiag_copy(h, b'u8', buf.ctypes.data_as(C.c_void_p), 16, C.byref(nb)), 'bytes')
    assert nb.value == rows * info(sv)['sp4'] * 4
    g = rng.randn(37, 2)
    g /= np.linalg.norm(g, axis=0)
    g[:, 1] *= 1. + 1e-8
    refused(lib.bc_snnls_prefdiag_sweep(h, 0, g.ctypes.data_as(C.c_void_p), 1.0, 0, p, p, p, rows, 1024, C.byref(form)), 'unit vectors')
    refused(lib.bc_snnls_prefdiag_sweep(h, 1, None, 1.0, 0, p, p, p, rows, 1024, C.byref(form)), 'own vectors')
    refused(lib.bc_snnls_prefdiag_sweep(h, 0, None, 1.0, 0, p, p, p, rows - 1, 1024, C.byref(form)), 'rows of output')
    refused(lib.bc_snnls_prefdiag_sweep(h, 0, None, 0.0, 0, p, p, p, rows, 1024, C.byref(form)), 'post_div')
    sv.build(1)
    refused(lib.bc_snnls_prefdiag_sweep(h, 0, None, 1.0, 1, p, p, p, rows, 1024, C.byref(form)), 'self_quantise')
    refused(lib.bc_snnls_prefdiag_sweep(h, 0, None, 1.0, 0, p, None, None, rows, 0, C.byref(form)), 'out_ul8')
    for prec in (16, 0):
        other = solver(bc, phi, prec)
        rc = lib.bc_snnls_prefdiag_sweep(other._eng.h, 0, None, 1.0, 0, p, p, p, rows, 1024, C.byref(form))
        refused(rc, 'per-row output' if prec else 'no pre-filter')
    os.environ['BC_I8_BB'] = '1'
    try:
        bb = solver(bc, phi, 8)
    finally:
        os.environ.pop('BC_I8_BB')
    refused(lib.bc_snnls_prefdiag_sweep(bb._eng.h, 0, None, 1.0, 0, p, p, p, rows, 1024, C.byref(form)), 'per-row output')
