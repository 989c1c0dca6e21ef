"""The cases of K3's GPU tests (tests/sweep_cases.py), on the CPU: bc_sweep_grid takes its arithmetic from csrc/bc_sweep_plan.h,
the header compiled for the host gives what the case file's restatement gives; every planted problem is what it claims in
np.longdouble (background <= 0.46, runners-up 0.999, the winner 1 and alone) and every position lands in the tile, lane, half,
wave, block and grid stride its label names; a NumPy model of the sweep's structure (per-lane best over the tiles a wave walks,
the shuffle-down tree with bc_better, four waves, per-block candidates, a strided reducer) returns the reference answer on
every case, and each of nine mutants of it is caught by a case named here; the derived value bound holds NumPy's float64
score in three summation orders and excludes a score with the last sample dropped."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import sweep_cases as SC                                                         # noqa: E402

CSRC = os.path.join(ROOT, 'beta_cores_amd', 'csrc')
N_CUS = (128, 228, 256, 304)
I64MAX = np.iinfo(np.int64).max


def need_longdouble():
    if not SC.LONGDOUBLE_OK:
        pytest.skip(SC.LONGDOUBLE_WHY)


# ------------------------------------------------------------------ the plan
def header_grids(tmp_path, rows):
    exe = str(tmp_path / 'sweep_plan_harness')
    cmd = ['gcc', '-std=c99', '-O1', '-Wall', '-Werror', '-pedantic-errors', '-I', CSRC, os.path.join(ROOT, 'tests', 'sweep_plan_harness.c'),
           '-o', exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    res = subprocess.run([exe], input=''.join('%d %d %d %d\n' % r for r in rows), capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr
    got = [int(line) for line in res.stdout.splitlines()]
    assert len(got) == len(rows)
    return got


def test_bc_sweep_grid_and_the_harness_share_the_header():
    src = open(os.path.join(CSRC, 'bc_core.hip')).read()
    assert '#include "bc_sweep_plan.h"' in src
    assert len(re.findall(r'\bbc_sweep_plan\(phi->ntiles, phi->s, phi->ctx->n_cu, env \? atoi\(env\) : 0\)', src)) == 1
    body = src[src.index('int bc_sweep_grid('):src.index('static int stat_blocks_for')]
    assert 'per_cu' not in body and 'want' not in body and '>= 64' not in body, 'bc_core.hip spells the grid arithmetic itself'
    assert body.count('getenv("BC_SWEEP_BLOCKS_PER_CU")') == 1
    hdr = open(os.path.join(CSRC, 'bc_sweep_plan.h')).read()
    assert int(re.search(r'#define BC_SWEEP_WAVES (\d+)', hdr).group(1)) == SC.WAVES
    dev = open(os.path.join(CSRC, 'bc_sweep_dev.h')).read()
    assert int(re.search(r'#define BC_SWEEP_U (\d+)', dev).group(1)) == SC.UNROLL
    assert '#include "bc_sweep_plan.h"' in dev and 'BC_SWEEP_WAVES' in dev           # (the sweep walks by the header's wave count)


def case_ntiles():
    nts = set(SC.ntiles_of(n) for n in (SC.N_ODD, SC.N_EVEN, 300, 700) + SC.TINY_N)
    for n_cu in N_CUS:
        nts |= set(SC.ntiles_of(c['n']) for c in (SC.stride_case(n_cu), SC.second_stride_case(n_cu), SC.wide_case(n_cu)))
    return sorted(nts)


def test_restated_grid_is_what_the_header_computes(tmp_path):
    rows = []
    for nt in sorted(set(list(range(0, 40)) + [511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097, 4099, 78125, 2 ** 31 + 5] + case_ntiles())):
        for s in (1, 4, 11, 23, 24, 63, 64, 600):
            for n_cu in N_CUS + (1, 152):
                for over in (0, 1, 2, 8, -1):
                    rows.append((nt, s, n_cu, over))
    have = header_grids(tmp_path, rows)
    wrong = [(r, h, SC.sweep_grid(*r)) for r, h in zip(rows, have) if h != SC.sweep_grid(*r)]
    assert not wrong, '(inputs, header, restatement) ' + repr(wrong[:5])


# ------------------------------------------------------------------ positions
def claims(label, G):
    """what a position's label says about where it lies"""
    want = {}
    m = re.search(r'\bblock (\d+)', label)
    if m:
        want['block'] = int(m.group(1))
    if 'last block' in label:
        want['block'] = G - 1
    for word, k in (('first stride', 0), ('second stride', 1), ('third stride', 2)):
        if word in label:
            want['stride'] = k
    for key in ('wave', 'lane', 'half'):
        m = re.search(r'\b%s (\d+)' % key, label)
        if m:
            want[key] = int(m.group(1))
    if re.search(r'\btile 0\b', label):
        want['tile'] = 0
    if 'first row' in label:
        want.update(lane=0, half=0)
    if 'first tile' in label:
        want['wave'] = 0
    if 'last tile' in label:
        want['wave'] = SC.WAVES - 1
    return want


def assert_lands(label, p, n, G):
    assert 0 <= p < n, label
    at = SC.locate(p, G)
    for k, val in claims(label, G).items():
        assert at[k] == val, (label, p, k, at)
    if label.endswith('last row'):
        assert p == n - 1


def test_positions_land_where_their_labels_say():
    for n in (SC.N_ODD, SC.N_EVEN):
        pos = SC.small_positions(n)
        assert len(set(pos.values())) == len(pos) >= 14
        for label, p in pos.items():
            assert_lands(label, p, n, 3)
        nt = SC.ntiles_of(n)
        assert nt == 12 and n % SC.TILE not in (0, 1) and all(SC.sweep_grid(nt, s, c) == 3 for s in SC.S_ALL for c in N_CUS)
    # the ragged last tile ends in half .x (n odd within the tile) once and in half .y once
    assert SC.locate(SC.N_ODD - 1, 3)['half'] == 0 and SC.locate(SC.N_EVEN - 1, 3)['half'] == 1
    halves = set((SC.locate(p, 3)['lane'] in (0, 63), SC.locate(p, 3)['half']) for p in SC.small_positions(SC.N_ODD).values())
    assert {(True, 0), (True, 1)} <= halves
    assert set(SC.locate(p, 3)['wave'] for p in SC.small_positions(SC.N_ODD).values()) == {0, 1, 2, 3}
    assert set(SC.SHORT) <= set(SC.small_positions(SC.N_ODD))
    for label, n, w in SC.small_ties():
        assert len(set(w)) == len(w) >= 2 and max(w) < n
    t = dict((label, w) for label, n, w in SC.small_ties())
    a, b = (SC.locate(p, 3) for p in t['two halves of a lane'])
    assert (a['tile'], a['lane']) == (b['tile'], b['lane']) and a['half'] != b['half']
    a, b = (SC.locate(p, 3) for p in t['two lanes of a wave'])
    assert a['tile'] == b['tile'] and a['lane'] != b['lane']
    a, b = (SC.locate(p, 3) for p in t['two waves of a block'])
    assert a['block'] == b['block'] and a['wave'] != b['wave'] and a['stride'] == b['stride']
    a, b = (SC.locate(p, 3) for p in t['two blocks'])
    assert a['block'] != b['block']
    # S: the remainder loop alone, the first unrolled trip, the unroll further out, the record's copy in two and three trips
    assert set(range(1, 12)) | {19, 20, 21, 30, 100, 257, 600} == set(SC.S_ALL)
    assert any(256 < s <= 512 for s in SC.S_ALL) and any(s > 512 for s in SC.S_ALL)
    # the offsets put 2^31 and 2^32 inside the Phi, between two listed positions
    for off in (2 ** 31 - 64, 2 ** 32 - 64):
        assert off in SC.OFFSETS and any(off + p < off + 64 for p in SC.OFFSET_POSITIONS) and 64 in SC.OFFSET_POSITIONS
    assert max(SC.OFFSETS) > 2 ** 33


@pytest.mark.parametrize('n_cu', N_CUS)
def test_device_sized_cases_keep_their_meaning(n_cu):
    for c in (SC.stride_case(n_cu), SC.second_stride_case(n_cu), SC.wide_case(n_cu)):
        G, n = c['grid'], c['n']
        assert SC.sweep_grid(SC.ntiles_of(n), c['S'], n_cu, c['per_cu']) == G and n % SC.TILE != 0
        assert n * c['S'] * 8 <= 24e6 * n_cu / 256.
        assert len(set(c['positions'].values())) == len(c['positions'])
        for label, p in c['positions'].items():
            assert_lands(label, p, n, G)
        for label, w in c['ties']:
            lo, hi = SC.locate(w[0], G), SC.locate(w[1], G)
            assert w[0] < w[1] < n
            if 'against' in label:          # the lower index lives in the higher block
                assert lo['block'] > hi['block'] and lo['stride'] < hi['stride'], label
            else:
                assert lo['block'] + int(label.split()[-1]) - 3 == hi['block'] and lo['stride'] == hi['stride'] == 0
    st = SC.stride_case(n_cu)
    assert set(SC.locate(p, st['grid'])['stride'] for p in st['positions'].values()) == {0, 1, 2}
    assert SC.locate(st['n'] - 1, st['grid']) == dict(SC.locate(st['n'] - 1, st['grid']), block=st['grid'] - 1, stride=2, wave=3)
    w = SC.wide_case(n_cu)
    blocks = set(SC.locate(p, w['grid'])['block'] for p in w['positions'].values())
    assert w['grid'] - 1 in blocks and any(b >= 256 for b in blocks)
    if n_cu == 256:
        assert w['grid'] == 1024 and w['n'] == 524588 and any(256 <= b < 512 for b in blocks) and any(512 <= b < 768 for b in blocks)
        assert len(w['ties']) == 3


# ------------------------------------------------------------------ the planted problems, in np.longdouble
def all_planted(n_cu=256):
    """[(label, n, S, mode, winners, per_cu)] of every planted case and tie pair"""
    out = []
    for S in SC.S_ALL:
        for mode in SC.modes_of(S):
            out += [('S %d mode %d %s' % (S, mode, label), n, S, mode, w, 0) for label, n, w in SC.small_cases(S, mode)]
    for S in SC.S_FULL:
        for mode in (0, 1):
            out += [('S %d mode %d tie: %s' % (S, mode, label), n, S, mode, w, 0) for label, n, w in SC.small_ties()]
    for c in (SC.stride_case(n_cu), SC.second_stride_case(n_cu), SC.wide_case(n_cu)):
        for mode in (0, 1):
            out += [('S %d mode %d n %d %s' % (c['S'], mode, c['n'], label), c['n'], c['S'], mode, (p,), c['per_cu'])
                    for label, p in c['positions'].items()]
            out += [('S %d mode %d n %d tie: %s' % (c['S'], mode, c['n'], label), c['n'], c['S'], mode, w, c['per_cu']) for label, w in c['ties']]
    return out


def test_planted_problems_are_what_they_claim():
    need_longdouble()
    seen, worst_bg = set(), 0.
    cases = all_planted()
    assert len(cases) > 300
    for label, n, S, mode, winners, _ in cases:
        bg, v, g_run = SC.background(n, S, mode)
        if (n, S, mode) not in seen:
            seen.add((n, S, mode))
            top = 0.
            for i in range(0, n, 65536):
                top = max(top, float(SC.ref_score(bg[i:i + 65536], v, mode).max()))
            worst_bg = max(worst_bg, top)
            assert top <= 0.46, (label, top)
            win, run = SC.special_rows(v, g_run, mode)
            sw, sr = SC.ref_score(np.stack((win, run)), v, mode)
            assert sw >= 1 - 1e-12 and 0.998 <= sr <= 0.9995, (label, sw, sr)
            if mode == 0:                                   # far from the mask's thresholds
                s1 = np.stack((win, run)).dot(v[:, 1]) / np.sqrt((np.stack((win, run)) ** 2).sum(axis=1))
                assert np.abs(s1).max() < 1e-12
        runners = SC.runner_positions(n, winners)
        assert not set(runners) & set(winners) and all(0 <= q < n for q in runners)
        p = min(winners)
        want = set(q for q in (p - 1, p + 1, p - 2, p + 2, p - 128, p + 128, 0, n - 1) if 0 <= q < n) - set(winners)
        assert set(runners) == want
        if len(winners) == 1 and n <= 2000:                 # the unique argmax, once more through the float64 oracle
            phi, v2, _ = SC.planted(n, S, mode, winners)
            sc = SC.numpy_scores(phi, v2, mode)
            assert int(np.argmax(sc)) == p and np.sort(sc)[-2] < 0.9995 if n > 1 else sc[0] > 0.99
    print('worst background score %.4f over %d backgrounds' % (worst_bg, len(seen)))


def test_sign_nan_and_mask_cases_are_what_they_claim():
    need_longdouble()
    for S in (1, 2):
        phi, v1, v0, first = SC.sign_case(S)
        sc = SC.numpy_scores(phi, v1, 1)
        assert set(np.unique(sc[np.isfinite(sc)])) == {-1., 1.} and int(np.argmax(sc)) == first and (sc[:first] < 1).all()
        assert (sc == -np.inf).sum() == 5 and (sc[first + 1:] == 1.).sum() == 150
        assert np.array_equal(SC.numpy_scores(phi, v0, 0), sc)
    for label, phi, v, mode, want in SC.nan_cases():
        sc = SC.numpy_scores(phi, v, mode)
        if want < 0:
            assert (sc == -np.inf).all()
        else:
            assert int(np.argmax(sc)) == want and np.isnan(sc[want]), label
    c = SC.nan_stride_case(256)
    sc = SC.numpy_scores(c['phi'], c['v'], 1)
    assert int(np.argmax(sc)) == c['expect'] and np.isnan(sc).sum() == 2
    lo, hi = SC.locate(c['expect'], c['grid']), SC.locate(int(np.flatnonzero(np.isnan(sc))[1]), c['grid'])
    assert lo['block'] > hi['block']
    # the mask: exact where the side of a threshold matters
    v = SC.mask_vectors()
    for label, phi, v, want in SC.mask_cases():
        sc = SC.numpy_scores(phi, v, 0)
        assert int(np.argmax(sc)) == want, label
        special = [want] + ([100, 200] if 'either side' in label else [])
        rest = np.delete(np.arange(phi.shape[0]), special)
        x = phi[rest].astype(SC.LD)
        s1 = x[:, 0] / np.sqrt((x * x).sum(axis=1))
        s1_64 = phi[rest, 0] / np.sqrt((phi[rest] ** 2).sum(axis=1))
        assert (np.abs(s1_64) == 1.).all() and (np.abs(np.abs(s1) - 1) < 2.0 ** -79).all()     # s1 = +-1 exactly in float64
        assert (sc[rest] == 0.).all() and np.array_equal(np.signbit(sc[rest]), phi[rest, 1] < 0)
        assert (np.abs(phi[rest].dot(v[:, 0]) / np.abs(phi[rest, 0])) > 10.).all(), 'a masked row with a small s0'
    t = dict((label, (phi, want)) for label, phi, _, want in SC.mask_cases())
    phi, _ = t['a -0.0 score before a +0.0 score']
    sc = SC.numpy_scores(phi, v, 0)
    assert np.signbit(sc[0]) and not np.signbit(sc[1]) and sc[0] == sc[1] == 0.
    phi, want = t['all masked but one modest row']
    sc = SC.numpy_scores(phi, v, 0)
    assert 0.3 < sc[want] < 0.5
    below, above = SC.threshold_rows()
    for row, masked in ((below, True), (above, False)):
        s64, sld = SC.threshold_s1(row)
        assert (s64 <= SC.THRESH) == masked and (sld <= SC.LD(SC.THRESH)) == masked
        assert abs(s64 - SC.THRESH) >= SC.THRESH_MARGIN and abs(sld - SC.LD(SC.THRESH)) >= SC.THRESH_MARGIN
    phi, want = t['s1 on either side of -1 + 1e-14']
    sc = SC.numpy_scores(phi, v, 0)
    assert sc[100] == 0. and 0.4 < sc[200] / SC.MASK_CDIR_SCALE < 0.6
    b = SC.bound(phi[200], v, 0)[0]
    assert np.isfinite(b) and 1e-3 < b / SC.ref_score(phi[200], v, 0)[0] < 0.2          # large, by derivation
    assert abs(sc[200] - SC.ref_score(phi[200], v, 0)[0]) <= b


# ------------------------------------------------------------------ the model of the sweep's structure, and its mutants
MUTANTS = ('r + 1 < n_rows dropped', 'r < n_rows read as <=', 'the remainder loop skipped', 'a tie goes to the higher index', 'NaN loses',
           'the reducer stops after one trip', 'the grid stride off by one block', 'the high word of the index lost in the shuffle',
           "the mask's > read as >=")


def better(av, ai, bv, bi, mut):
    """bc_better (bc_internal.h), element-wise"""
    an, bn = np.isnan(av), np.isnan(bv)
    tie = (ai > bi) if mut == 'a tie goes to the higher index' else (ai < bi)
    with np.errstate(invalid='ignore'):
        plain = np.where(av > bv, True, np.where(av < bv, False, tie))
    nans = ~an if mut == 'NaN loses' else np.where(an & bn, tie, an)
    return np.where(an | bn, nans, plain)


def model_scores(phi, v, mode, post_div, mut):
    """(scores, norms) over ntiles * 128 rows, the dot products as chains in k order; the rows past n hold what a Phi
    re-used at a smaller row count may hold there -- a non-zero norm and a NaN score -- and are the kernel's to leave alone"""
    n, S = phi.shape
    K = (S // SC.UNROLL) * SC.UNROLL if mut == 'the remainder loop skipped' else S
    V = v if mode == 0 else v[:, None]
    acc = np.zeros((n, V.shape[1]))
    nr2 = np.zeros(n)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        for k in range(S):
            if k < K:
                acc += phi[:, k:k + 1] * V[k][None, :]
            nr2 += phi[:, k] ** 2
        nr = np.sqrt(nr2)
        safe = np.where(nr != 0., nr, 1.)
        if mode == 1:
            sc = acc[:, 0] / safe / post_div
        else:
            s0, s1 = acc[:, 0] / safe, acc[:, 1] / safe
            rest = 1. - s1 * s1
            ok = (s1 > -1. + 1e-14) & ((rest >= 0.) if mut == "the mask's > read as >=" else (rest > 0.))
            sc = s0 / np.where(ok, np.sqrt(np.where(ok, rest, 1.)), np.inf)
    nt = SC.ntiles_of(n)
    full_sc, full_nr = np.full(nt * SC.TILE, np.nan), np.ones(nt * SC.TILE)
    full_sc[:n], full_nr[:n] = sc, nr
    return full_sc, full_nr


def shuffle_tree(bv, bi, mut):
    """bc_wave_argmax over the last axis (64 lanes); the result is lane 0's"""
    d = 32
    while d >= 1:
        ov, oi = bv.copy(), bi.copy()
        ov[..., :64 - d], oi[..., :64 - d] = bv[..., d:], bi[..., d:]        # (__shfl_down past the wave returns the lane's own)
        if mut == 'the high word of the index lost in the shuffle':
            oi = oi & 0xffffffff
        up = better(ov, oi, bv, bi, mut)
        bv, bi = np.where(up, ov, bv), np.where(up, oi, bi)
        d //= 2
    return bv[..., 0], bi[..., 0]


def fold(bv, bi, mut):
    """thread 0's sequential pass over the waves' results (axis -1)"""
    cv, ci = bv[..., 0], bi[..., 0]
    for w in range(1, bv.shape[-1]):
        up = better(bv[..., w], bi[..., w], cv, ci, mut)
        cv, ci = np.where(up, bv[..., w], cv), np.where(up, bi[..., w], ci)
    return cv, ci


def model(phi, v, mode, post_div=1., n_cu=256, per_cu=0, row_offset=0, threads=256, mut=None):
    """(index or -1, score): k_sweep<MODE> over grid blocks of four waves, then a reducer of `threads` threads"""
    n, S = phi.shape
    nt = SC.ntiles_of(n)
    grid = SC.sweep_grid(nt, S, n_cu, per_cu)
    sc, nr = model_scores(phi, v, mode, post_div, mut)
    bv = np.full((grid, SC.WAVES, 64), -np.inf)
    bi = np.full((grid, SC.WAVES, 64), I64MAX, dtype=np.int64)
    t = np.arange(grid, dtype=np.int64)[:, None] * SC.WAVES + np.arange(SC.WAVES, dtype=np.int64)[None, :]
    step = (grid + (1 if mut == 'the grid stride off by one block' else 0)) * SC.WAVES
    lane2 = 2 * np.arange(64, dtype=np.int64)[None, None, :]
    while (t < nt).any():
        live = (t < nt)[:, :, None]
        r = np.where(t < nt, t, 0)[:, :, None] * SC.TILE + lane2
        for half in (0, 1):
            if half == 0:
                inside = (r <= n) if mut == 'r < n_rows read as <=' else (r < n)
            else:
                inside = np.ones(r.shape, dtype=bool) if mut == 'r + 1 < n_rows dropped' else (r + 1 < n)
            cv, ci = sc[r + half], row_offset + r + half
            up = live & inside & (nr[r + half] != 0.) & better(cv, ci, bv, bi, mut)
            bv, bi = np.where(up, cv, bv), np.where(up, ci, bi)
        t = t + step
    wv, wi = shuffle_tree(bv, bi, mut)                       # [grid x 4]
    blk_v, blk_i = fold(wv, wi, mut)                         # [grid]: blk_val, blk_idx
    trips = 1 if mut == 'the reducer stops after one trip' else (grid + threads - 1) // threads
    pv = np.full(trips * threads, -np.inf)
    pi = np.full(trips * threads, I64MAX, dtype=np.int64)
    m = min(grid, trips * threads)
    pv[:m], pi[:m] = blk_v[:m], blk_i[:m]
    tv, ti = fold(pv.reshape(trips, threads).T, pi.reshape(trips, threads).T, mut)      # each thread over its trips
    wv, wi = shuffle_tree(tv.reshape(threads // 64, 64), ti.reshape(threads // 64, 64), mut)
    fv, fi = fold(wv[None, :], wi[None, :], mut)
    return (int(fi[0]) if fi[0] != I64MAX else -1), float(fv[0])


def oracle(phi, v, mode, post_div=1., row_offset=0):
    sc = SC.numpy_scores(phi, v, mode, post_div)
    if (sc == -np.inf).all():
        return -1, -np.inf
    f = int(np.argmax(sc))
    return f + row_offset, sc[f]


def agrees(got, want):
    return got[0] == want[0] and (got[1] == want[1] or (np.isnan(got[1]) and np.isnan(want[1])) or abs(got[1] - want[1]) <= 1e-12 * abs(want[1]))


def test_model_returns_the_reference_answer_on_every_case():
    ran = 0
    for label, n, S, mode, winners, per_cu in all_planted():
        if n > 2000 and mode == 0 and 'tie' not in label and 'last row' not in label:
            continue                                         # (the large problems: every tie, every mode-1 position, the last rows)
        phi, v, _ = SC.planted(n, S, mode, winners)
        want = oracle(phi, v, mode)
        assert want[0] == min(winners), label
        for threads in sorted(set(SC.PICK_THREADS.values())):
            assert agrees(model(phi, v, mode, per_cu=per_cu, threads=threads), want), (label, threads)
        ran += 1
    pos = SC.small_positions(SC.N_ODD)
    for S in SC.S_ALL:
        for mode in SC.modes_of(S):
            for key in ('last row', 'block 1 first tile'):
                phi, v, want = SC.runners_alone(SC.N_ODD, S, mode, pos[key])
                got = oracle(phi, v, mode)
                assert got[0] == want == pos[key] - SC.TILE and 0.998 < got[1] < 0.9995 and agrees(model(phi, v, mode), got)
    for off in SC.OFFSETS:
        for p in SC.OFFSET_POSITIONS:
            phi, v, _ = SC.planted(SC.N_ODD, 4, 1, (p,))
            assert model(phi, v, 1, row_offset=off)[0] == off + p
    for S in (1, 2):
        phi, v1, v0, first = SC.sign_case(S)
        assert model(phi, v1, 1) == (first, 1.) and model(phi, v0, 0) == (first, 1.)
    for label, phi, v, mode, want in SC.nan_cases():
        got = model(phi, v, mode)
        assert got[0] == want and (want < 0 or np.isnan(got[1])), label
    c = SC.nan_stride_case(256)
    for threads in (256, 512):
        assert model(c['phi'], c['v'], 1, per_cu=1, threads=threads)[0] == c['expect']
    for label, phi, v, want in SC.mask_cases():
        got = model(phi, v, 0)
        assert agrees(got, oracle(phi, v, 0)) and got[0] == want, label
    print('the model agrees with the oracle on %d planted cases and the sign, NaN and mask cases' % ran)


def catching_cases():
    """{mutant: (name of the case that catches it, arguments of model())}"""
    st, wd = SC.stride_case(256), SC.wide_case(256)
    pos = SC.small_positions(SC.N_ODD)
    t = dict((label, w) for label, n, w in SC.small_ties())
    nan = dict((c[0], c) for c in SC.nan_cases())
    mask = dict((c[0], c) for c in SC.mask_cases())
    p1 = SC.planted(SC.N_ODD, 4, 1, (pos['block 0 wave 1'],))
    p2 = SC.planted(SC.N_EVEN, 4, 1, (SC.small_positions(SC.N_EVEN)['block 0 wave 1'],))
    return {
        'r + 1 < n_rows dropped': ('S 4 mode 1 n 1445 block 0 wave 1 (a ragged tile whose last row is in half .x)', dict(phi=p1[0], v=p1[1], mode=1)),
        'r < n_rows read as <=': ('S 4 mode 1 n 1446 block 0 wave 1 (a ragged tile whose last row is in half .y)', dict(phi=p2[0], v=p2[1], mode=1)),
        'the remainder loop skipped': ('S 4 mode 1 n 1445 block 0 wave 1 (S < 10: the remainder loop alone)', dict(phi=p1[0], v=p1[1], mode=1)),
        'a tie goes to the higher index': ('S 4 mode 1 tie: two blocks', dict(zip(('phi', 'v'), SC.planted(SC.N_ODD, 4, 1, t['two blocks'])[:2]), mode=1)),
        'NaN loses': ('mode 1: a NaN row after the winner', dict(phi=nan['mode 1: a NaN row after the winner'][1], v=nan['mode 1: a NaN row after the winner'][2], mode=1)),
        'the reducer stops after one trip': ('S 4 mode 1 n %d block 259' % wd['n'],
                                             dict(zip(('phi', 'v'), SC.planted(wd['n'], 4, 1, (wd['positions']['block 259'],))[:2]), mode=1)),
        'the grid stride off by one block': ('S 4 mode 1 n %d block 0 second stride (BC_SWEEP_BLOCKS_PER_CU=1)' % st['n'],
                                             dict(zip(('phi', 'v'), SC.planted(st['n'], 4, 1, (st['positions']['block 0 second stride'],))[:2]), mode=1, per_cu=1)),
        'the high word of the index lost in the shuffle': ('S 4 mode 1 n 1445 block 0 wave 1 at row_offset 2^33 + 5', dict(phi=p1[0], v=p1[1], mode=1, row_offset=2 ** 33 + 5)),
        "the mask's > read as >=": ('all rows masked: row 0', dict(phi=mask['all rows masked: row 0'][1], v=mask['all rows masked: row 0'][2], mode=0)),
    }


def test_every_mutant_is_caught_by_a_named_case():
    catch = catching_cases()
    assert set(catch) == set(MUTANTS)
    for mut in MUTANTS:
        name, kw = catch[mut]
        want = oracle(kw['phi'], kw['v'], kw['mode'], row_offset=kw.get('row_offset', 0))
        assert agrees(model(**kw), want), name
        got = model(mut=mut, **kw)
        assert got[0] != want[0], 'mutant "%s" survives %s' % (mut, name)
        print('mutant "%s": caught by %s (index %d for %d)' % (mut, name, got[0], want[0]))
    # the 512-thread reducers take their second trip at block 512
    wd = SC.wide_case(256)
    phi, v, _ = SC.planted(wd['n'], 4, 1, (wd['positions']['block 515'],))
    assert model(phi, v, 1, threads=512)[0] == wd['positions']['block 515']
    assert model(phi, v, 1, threads=512, mut='the reducer stops after one trip')[0] != wd['positions']['block 515']


# ------------------------------------------------------------------ the value bound
def chain_scores(row, v, mode, post_div, order):
    """the score in float64 NumPy, the S products added in one of three orders"""
    V = v if mode == 0 else v[:, None]
    S = row.shape[0]
    if order == 'forward':
        ks = range(S)
    elif order == 'backward':
        ks = range(S - 1, -1, -1)
    if order == 'pairwise':
        a = (row[:, None] * V).sum(axis=0)
        nr = np.sqrt((row * row).sum())
    else:
        a, nr2 = np.zeros(V.shape[1]), 0.
        for k in ks:
            a = a + row[k] * V[k]
            nr2 = nr2 + row[k] * row[k]
        nr = np.sqrt(nr2)
    if mode == 1:
        return a[0] / nr / post_div
    s0, s1 = a[0] / nr, a[1] / nr
    return s0 / np.sqrt(1. - s1 * s1)


def test_numpy_float64_lies_inside_the_bound_and_a_dropped_sample_outside():
    need_longdouble()
    worst = (0., None)
    for S in SC.S_ALL:
        for mode in SC.modes_of(S):
            bg, v, g_run = SC.background(SC.N_ODD, S, mode)
            win, run = SC.special_rows(v, g_run, mode)
            for post_div in ((1., float(S)) if mode == 1 else (1.,)):
                for name, row in (('winner', win), ('runner-up', run), ('background', bg[17]), ('background', bg[1444])):
                    for order in ('forward', 'backward', 'pairwise'):
                        r = SC.ratio(chain_scores(row, v, mode, post_div, order), row, v, mode, post_div)
                        worst = max(worst, (r, (S, mode, post_div, name, order)))
                        assert r <= 1., (S, mode, post_div, name, order, r)
                    if name == 'winner' and mode == 1:          # (the norm is the full row's: only the dot product loses its last term)
                        assert abs(v[-1]) > 1e-4, 'the last sample of v carries nothing'
                        drop = row[:-1].dot(v[:-1]) / np.sqrt((row ** 2).sum()) / post_div
                        assert SC.ratio(drop, row, v, mode, post_div) > 1., (S, mode, name)
    print('worst error / bound of NumPy float64: %.3f at %r' % worst)
    assert worst[0] > 0.01
    # mode 0, the last sample dropped from both dot products of the winner
    for S in (4, 11, 100):
        bg, v, g_run = SC.background(SC.N_ODD, S, 0)
        win, _ = SC.special_rows(v, g_run, 0)
        nr = np.sqrt((win ** 2).sum())
        s0, s1 = win[:-1].dot(v[:-1, 0]) / nr, win[:-1].dot(v[:-1, 1]) / nr
        assert SC.ratio(s0 / np.sqrt(1. - s1 * s1), win, v, 0) > 1.
