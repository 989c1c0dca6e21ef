"""The two-level sweep's hand-over to the rescoring stage (csrc/bc_prefilter_i4.h: the end of k_sweep_i4; bc_rescore_dev.h: its
consumer), pair by pair, on all three ways through: a block's own list of 8, the spill list (code -1) and the give-up (code -2).
The checker is tests/handover_cases.py (tests/test_handover_cases_cpu.py shows that it can fail).

Shapes: 4, 8 or 12 sweep blocks of four 256-row tiles, the last tile ragged; every wave walks one tile and block b owns tiles
4b .. 4b+3 (asserted from the seam).  Data: the recipe of concentrated_phi (tests/test_gpu_two_level.py) -- correlated rows,
copies of the row that tops the first step's scores planted in chosen blocks; the other rows of a planted block are the
lowest-scoring ones of the data, so that level 2 re-bounds the copies there and nothing else and the number of rows the block
holds does not depend on the order of its waves' atomics.  The solver is warmed (a step and a reset, twice: where the first
step overflows into the exact sweep it leaves no seeds, the second -- a two-level sweep -- leaves each block's strongest row)
so that theta0 sits at the copies' level.

  (a) per case and algorithm: the DIAGNOSTIC sweep's lists, spill list and spill count against its own per-row values; then the
      PRODUCTION sweep of the same state (lists fetched between step_local and step_finish) against the same values.  A
      diagnostic sweep of an unrelated vector in between leaves the spill list without the pairs of the first.
  (b) on one solver: a step that spills 400 pairs, then a step that spills 9 from another block (the count, not the contents
      of the list, is what bounds the rescoring stage's scan); a block that spills without being in play next to a listed one
      that is; the count is 0 after every step_finish.
  (c) the consumers: 12 steps against the fp64 sweep under the three finish forms (rescoring inside k_step_finish_pf, k_rescore
      as its own launch, the plain finish kernel).
No test repeats a run or looks at compiled code."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import handover_cases as H                                                  # noqa: E402
from test_gpu_pref_bounds import blocks_of, fetch, info, native, sweep     # noqa: E402
from test_gpu_prefilter import correlated, prefilter, same                 # noqa: E402

pytestmark = pytest.mark.gpu
SPILL_N = 14                                                                # BC_PCTL_SPILL_N (csrc/bc_pref_ctrl.h)
PLAIN, ONE_ROUND, ONE_ROUND_RESCORE = 1, 2, 3                               # include/beta_cores.h: BC_FINISH_*
KNOBS = {None: ONE_ROUND_RESCORE, 'BC_FINISH_NOFUSE': ONE_ROUND, 'BC_FINISH_NOPF': PLAIN}

#        blocks, S, exact copies?, [(block, copies, first row within the block)]
CASES = {
    'k8': (4, 64, True, [(1, 8, 250)]),                                      # the list is full: two tiles, code 8
    'k9': (4, 64, True, [(1, 9, 250)]),                                      # one more: code -1, nine pairs
    'k300': (4, 100, False, [(2, 300, 0)]),                                  # a wave parks more than 128 rows: level 2 runs mid-tile
    'k512': (4, 64, True, [(1, 512, 0)]),                                    # all the block can hold
    'k513': (4, 64, True, [(1, 513, 0)]),                                    # one more: code -2
    'three': (8, 64, False, [(0, 20, 100), (3, 150, 200), (5, 400, 0)]),     # three blocks take their bases by atomicAdd
    'four': (8, 100, False, [(0, 20, 100), (3, 150, 200), (5, 400, 0), (7, 5, 800)]),      # ... and a listed one in the ragged tile
    'cap': (12, 64, True, [(b, 450, 0) for b in (0, 1, 2, 3, 4, 5, 6, 7, 8, 11)]),          # 4500 pairs for 4096 slots
}
GIVES_UP = ('k513', 'cap')
RAGGED = 37


@pytest.fixture(scope='module')
def bc():
    import beta_cores_amd as bc
    bc.default_context()
    return bc


_PHI, _REF = {}, {}


@pytest.fixture(scope='module', autouse=True)
def release():
    yield
    _PHI.clear()
    _REF.clear()


def low_rows_into(phi, fixed, blocks):
    """Permute the rows that are not `fixed` so that those of `blocks` are the lowest-scoring ones (first-step scores)."""
    n = len(phi)
    score = phi.dot(phi.sum(axis=0)) / np.linalg.norm(phi, axis=1)
    inside = np.zeros(n, dtype=bool)
    for b in blocks:
        inside[1024 * b:1024 * (b + 1)] = True
    free_in, free_out = np.nonzero(inside & ~fixed)[0], np.nonzero(~inside & ~fixed)[0]
    pool = np.nonzero(~fixed)[0]
    pool = pool[np.argsort(score[pool], kind='stable')]
    out = phi.copy()
    out[free_in] = phi[pool[:len(free_in)]]
    out[free_out] = phi[np.sort(pool[len(free_in):])]
    return out


def case_phi(name):
    """(phi, {block: rows planted})"""
    if name not in _PHI:
        blocks, s, exact, plants = CASES[name]
        n = 1024 * blocks - RAGGED
        rng = np.random.RandomState(sum(map(ord, name)))
        phi = correlated(rng, n, s)
        top = int(np.argmax(phi.dot(phi.sum(axis=0)) / np.linalg.norm(phi, axis=1)))
        src = phi[top].copy()
        phi[top] = correlated(rng, 1, s)[0]                                  # (the original goes: the copies are the only rows at the top)
        fixed = np.zeros(n, dtype=bool)
        rows = {}
        for b, k, at in plants:
            rows[b] = 1024 * b + at + np.arange(k)
            assert rows[b][-1] < n
            phi[rows[b]] = src if exact else src * (1. + 1e-9 * rng.randn(k, s))
            fixed[rows[b]] = True
        phi = low_rows_into(phi, fixed, rows.keys())
        score = phi.dot(phi.sum(axis=0)) / np.linalg.norm(phi, axis=1)
        assert score[fixed].min() > score[~fixed].max()                      # the data do what they are for
        _PHI[name] = (phi, rows)
    return _PHI[name]


def solver_class(bc, alg):
    return bc.snnls.GIGA if alg == 'giga' else bc.snnls.FrankWolfe


def warm_solver(bc, alg, phi, form=4, knob=None):
    old = dict((k, os.environ.get(k)) for k in KNOBS if k)
    for k in old:
        os.environ.pop(k, None)
    if knob:
        os.environ[knob] = '1'
    try:
        with prefilter(form):
            sv = solver_class(bc, alg)(phi.T, phi.sum(axis=0))
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    if form == 4:
        assert sv._eng.prefilter == 8 and sv._eng.prefilter_form == 3
        for _ in range(2):
            sv.build(1)
            sv.reset()
    return sv


def geometry(sv, blocks):
    i = info(sv)
    blk, grid = blocks_of(i, 3)
    assert i['grid1'] == grid == blocks and i['ptiles'] == 4 * blocks and np.array_equal(blk, np.arange(4 * blocks) // 4)
    assert i['blk_nc'] == H.BLK_NC and i['spill_cap'] == H.SPILL_CAP
    return i, blk, grid


def begin(sv, steps):
    native().call('bc_snnls_build_begin', sv._eng.h, steps)


def end(sv):
    lim, done, pending = C.c_int(), C.c_int(), C.c_int()
    native().call('bc_snnls_build_end', sv._eng.h, C.byref(lim), C.byref(done), C.byref(pending))
    return done.value, pending.value


def spill_count(sv, which='ctrl'):
    return int(fetch(sv, which, np.int32)[SPILL_N])


def outputs(sv, which):
    """What the last two-level sweep handed over; which: 'ctrl' (a production sweep in flight) or 'ctrl_swept' (the diagnostic)."""
    return dict(blk_nc=fetch(sv, 'l2_blk_nc', np.int32).copy(), blk_cand=fetch(sv, 'l2_blk_cand', np.int32).copy(),
                blk_l=fetch(sv, 'l2_blk_l', np.float64).copy(), blk_u=fetch(sv, 'l2_blk_u', np.float32).copy(),
                spill=fetch(sv, 'spill', np.int32).reshape(-1, 2).copy(), count=spill_count(sv, which))


def held_to(ul8, out, blk, grid, **kw):
    return H.check_handover(ul8, out['blk_nc'], out['blk_cand'], out['blk_l'], out['blk_u'], out['spill'], out['count'], blk, grid, **kw)


def diagnostic(sv, mode, blk, grid, tag, **kw):
    """One diagnostic sweep of the solver's own vectors, held to its own per-row values: (ul8, outputs, report)."""
    assert info(sv)['next_form'] == 3 and spill_count(sv) == 0
    form, _, ul8, th = sweep(sv, mode)
    assert form == 3
    out = outputs(sv, 'ctrl_swept')
    assert spill_count(sv) == 0                                              # (the diagnostic restored the control block)
    rep = held_to(ul8, out, blk, grid, **kw)
    print('%s: theta0 %.6f .. %.6f, spill count %d, blocks {b: (in play, re-bounded, code)} %s' % (tag, th.min(), th.max(), out['count'], rep))
    return ul8, out, rep


def expect(name, rows, rep, out):
    """The case's own precondition, from the per-row values, and the codes it is there for."""
    for b, r in rows.items():
        k = len(r)
        want, done, code = rep[b]
        assert want == k and (done == k or done <= H.L2_LCAP or k > H.L2_LCAP), (name, b, rep[b])
        if name == 'cap':
            assert code in (-1, -2)
        else:
            assert code == (k if k <= H.BLK_NC else (-1 if k <= H.L2_LCAP else -2)), (name, b, rep[b])
    total = sum(len(r) for r in rows.values() if len(r) > H.BLK_NC)
    if name == 'cap':
        assert out['count'] == total == 4500 and sorted(rep[b][2] for b in rows) == [-2] + 9 * [-1]
    elif name == 'k513':
        assert out['count'] == 0
    else:
        assert out['count'] == total


# ------------------------------------------------------------------ (a) pair level
@pytest.mark.parametrize('alg', ['giga', 'fw'])
@pytest.mark.parametrize('name', list(CASES))
def test_pairs_of_the_diagnostic_and_the_production_sweep(bc, name, alg):
    phi, rows = case_phi(name)
    blocks, s = CASES[name][:2]
    mode = 0 if alg == 'giga' else 1
    sv = warm_solver(bc, alg, phi)
    i, blk, grid = geometry(sv, blocks)
    begin(sv, 1)
    ul8, out, rep = diagnostic(sv, mode, blk, grid, '%s %s diagnostic' % (name, alg))
    expect(name, rows, rep, out)
    # an unrelated sweep: whatever it spills carries other bits, and the rest of the spill list reads (-1, -1)
    sweep(sv, 1, np.random.RandomState(1).randn(s))
    stale = fetch(sv, 'spill', np.int32).reshape(-1, 2)
    planted = np.concatenate(list(rows.values()))
    assert not (np.isin(stale[:, 1], planted) & np.isin(stale[:, 0], out['spill'][:, 0])).any()
    falls = sv._eng.prefilter_fallbacks()
    native().call('bc_snnls_step_local', sv._eng.h)
    prod = outputs(sv, 'ctrl')                                               # (the rescoring stage has not run: the step is in flight)
    native().call('bc_snnls_step_finish', sv._eng.h)
    assert sv._eng.finish_form() == ONE_ROUND_RESCORE
    rep2 = held_to(ul8, prod, blk, grid)
    print('%s %s production: spill count %d, blocks %s' % (name, alg, prod['count'], rep2))
    expect(name, rows, rep2, prod)
    assert spill_count(sv) == 0                                              # consumed (or abandoned) by the rescoring stage
    done, pending = end(sv)
    falls = sv._eng.prefilter_fallbacks() - falls
    print('%s %s: fallbacks %d, pending %d' % (name, alg, falls, pending))
    if name in GIVES_UP:
        assert pending == 1 and done == 0 and falls >= 1                    # the step is to be redone by the exact sweep
    else:
        assert pending == 0 and done == 1 and falls == 0
        first = int(sv._eng.trace()[0][0])
        assert first in planted and (not CASES[name][2] or first == planted.min())      # of exact ties, the lowest index


# ------------------------------------------------------------------ (b) sequences on one solver
def sequence_phi():
    """Block 1: 400 exact copies of the row `a` that tops the first step's scores (400 rows of -a in block 4 keep b the data's
    own).  Row z (block 0), at 18 degrees from a: with the weight w on it -- state 2 -- both algorithms sweep with the part of b
    orthogonal to z, and the 9 exact copies of that direction in block 3 (c; rows of -c in block 0 keep b as it is) score 1, the
    copies of a 0.1 (Frank-Wolfe) and 0.4 (GIGA).  Under GIGA the 4-bit level cannot bound a row at 18 degrees from the iterate
    and passes the copies of a and of -a on; among themselves they would tie and spill again, so blocks 1 and 4 hold one more
    copy of c each, whose int8 lower bound is above their upper bounds: these blocks list one pair."""
    if 'seq' not in _PHI:
        blocks, s = 8, 64
        n = 1024 * blocks - RAGGED
        rng = np.random.RandomState(77)
        phi = correlated(rng, n, s)
        rows = {1: 1024 + 300 + np.arange(400), 3: 3 * 1024 + 700 + np.arange(9)}
        zrow, neg, lone, nega = 40, 60 + np.arange(11), 1024 + 100, 4 * 1024 + 50 + np.arange(400)
        lones = [lone, 4 * 1024 + 10]                                        # a copy of c beside the copies of a and of -a, see below
        fixed = np.zeros(n, dtype=bool)
        fixed[np.concatenate((rows[1], rows[3], neg, nega, [zrow], lones))] = True
        phi[fixed] = 0.
        score = np.where(fixed, -np.inf, phi.dot(phi.sum(axis=0)) / np.maximum(np.linalg.norm(phi, axis=1), 1e-300))
        top = int(np.argmax(score))
        a = phi[top].copy()
        phi[top] = correlated(rng, 1, s)[0]
        b0 = phi.sum(axis=0)
        phi[rows[1]] = a
        phi[nega] = -a                                                       # (b stays the data's own: the copies do not pull it onto a)
        an = np.linalg.norm(a)
        q = rng.randn(s)
        q -= q.mean()
        for _ in range(2):                                                   # orthogonal to a and to b
            q -= q.dot(a) / an ** 2 * a
            q -= q.dot(b0) / b0.dot(b0) * b0
            q -= q.dot(a) / an ** 2 * a
        phi[zrow] = 0.95 * a + 0.3122 * an * q / np.linalg.norm(q)
        z = phi[zrow]
        b = phi.sum(axis=0)
        w = b.dot(z) / z.dot(z)
        c = b - w * z
        c *= an / np.linalg.norm(c)
        phi[rows[3]] = c
        phi[lones] = c
        phi[neg] = -c
        phi = low_rows_into(phi, fixed, (1, 3))
        b = phi.sum(axis=0)
        u = phi / np.linalg.norm(phi, axis=1)[:, None]
        p = b - w * phi[zrow]
        s1, s2 = u.dot(b) / np.linalg.norm(b), u.dot(p) / np.linalg.norm(p)      # the scores of state 1 (both algorithms), of state 2 ...
        g2 = s2 / np.sqrt(np.maximum(1. - u.dot(z / np.linalg.norm(z)) ** 2, 1e-300))      # ... and GIGA's, on the geodesic from z
        free = ~fixed
        assert s1[rows[1]].min() > max(s1[free].max(), s1[zrow], s1[rows[3]].max() + 0.15)
        for sc in (s2, g2):
            assert sc[rows[3]].min() > max(sc[free].max(), sc[rows[1]].max() + 0.25) and sc[lone] == sc[rows[3][0]]
        _PHI['seq'] = (phi, rows, zrow, w, lone)
    return _PHI['seq']


@pytest.mark.parametrize('alg', ['giga', 'fw'])
def test_a_small_spill_after_a_large_one(bc, alg):
    phi, rows, zrow, w, lone = sequence_phi()
    mode = 0 if alg == 'giga' else 1
    sv = warm_solver(bc, alg, phi)
    i, blk, grid = geometry(sv, 8)

    def state2(s_):
        s_._eng.set_sparse_weights([zrow], [w])

    for _ in range(2):                                                       # seeds for state 2 as well
        state2(sv)
        sv.build(1)
    # what a sweep of state 2 hands over, from its own per-row values
    state2(sv)
    begin(sv, 0)
    ul8_2, out2, rep2 = diagnostic(sv, mode, blk, grid, 'sequence %s, state 2' % alg, allow_give_up=False)
    end(sv)
    assert rep2[3] == (9, 9, -1) and out2['count'] == 9 and all(code >= 0 for b, (_, _, code) in rep2.items() if b != 3)
    nine = set((H.bits(ul8_2[r, 0]), int(r)) for r in rows[3])
    # step 1: block 1 spills 400 pairs
    sv.reset()
    begin(sv, 1)
    ul8_1, out1, rep1 = diagnostic(sv, mode, blk, grid, 'sequence %s, state 1' % alg, allow_give_up=False)
    assert rep1[1][0] == 400 and rep1[1][2] == -1 and out1['count'] == 400
    native().call('bc_snnls_step_local', sv._eng.h)
    prod1 = outputs(sv, 'ctrl')
    native().call('bc_snnls_step_finish', sv._eng.h)
    assert held_to(ul8_1, prod1, blk, grid, allow_give_up=False) == rep1 and prod1['count'] == 400
    # (no end of the build call here: it lets the host's watch look at the share of rows the first level passed on in the four
    # two-level sweeps so far, the badly seeded first one of state 2 among them, and the watch would put the form aside)
    assert spill_count(sv) == 0 and sv._eng.trace()[0].tolist() == [rows[1][0]]
    # step 2: block 3 spills 9 pairs over the head of the 400
    state2(sv)
    falls = sv._eng.prefilter_fallbacks()
    begin(sv, 1)
    native().call('bc_snnls_step_local', sv._eng.h)
    prod2 = outputs(sv, 'ctrl')
    native().call('bc_snnls_step_finish', sv._eng.h)
    print('sequence %s, step 2: spill count %d, codes %s' % (alg, prod2['count'], prod2['blk_nc'].tolist()))
    assert prod2['count'] == 9 and prod2['blk_nc'][3] == -1 and (np.delete(prod2['blk_nc'], 3) >= 0).all()
    assert set((int(u) & 0xffffffff, int(r)) for u, r in prod2['spill'][:9]) == nine
    assert np.isin(prod2['spill'][9:400, 1], rows[1]).all()                  # behind them, what step 1 left: the count bounds the scan
    assert spill_count(sv) == 0 and end(sv)[1] == 0 and sv._eng.prefilter_fallbacks() == falls
    with prefilter(0):
        ref = solver_class(bc, alg)(phi.T, phi.sum(axis=0))
    state2(ref)
    ref.build(1)
    assert int(sv._eng.trace()[0][-1]) == int(ref._eng.trace()[0][-1]) == lone      # of the eleven exact ties, the lowest index
    assert np.array_equal(sv._eng.sparse_weights()[0], ref._eng.sparse_weights()[0]) and \
        np.array_equal(sv._eng.sparse_weights()[1], ref._eng.sparse_weights()[1]) and sv.error() == ref.error()


def idle_spill_phi():
    """Block 1: 5 exact copies of the top row.  Block 2: 20 exact copies of a row d at 18 degrees from it -- near enough to pass
    the 4-bit level, too far for its int8 upper bound to reach the copies' lower bound: block 2 spills and is not in play."""
    if 'idle' not in _PHI:
        blocks, s = 4, 64
        n = 1024 * blocks - RAGGED
        rng = np.random.RandomState(99)
        phi = correlated(rng, n, s)
        top = int(np.argmax(phi.dot(phi.sum(axis=0)) / np.linalg.norm(phi, axis=1)))
        a = phi[top].copy()
        phi[top] = correlated(rng, 1, s)[0]
        rows = {1: 1024 + 500 + np.arange(5), 2: 2048 + 250 + np.arange(20)}
        b = phi.sum(axis=0)
        q = rng.randn(s)
        q -= q.mean()
        q -= q.dot(a) / a.dot(a) * a
        q -= q.dot(b) / b.dot(b) * (b - b.dot(a) / a.dot(a) * a)
        phi[rows[1]] = a
        phi[rows[2]] = 0.95 * a + 0.3122 * np.linalg.norm(a) * q / np.linalg.norm(q)
        fixed = np.zeros(n, dtype=bool)
        fixed[np.concatenate(list(rows.values()))] = True
        phi = low_rows_into(phi, fixed, (1, 2))
        score = phi.dot(phi.sum(axis=0)) / np.linalg.norm(phi, axis=1)
        assert score[rows[1]].min() > score[rows[2]].max() > score[~fixed].max()
        _PHI['idle'] = (phi, rows)
    return _PHI['idle']


@pytest.mark.parametrize('alg', ['giga', 'fw'])
def test_a_spilled_block_out_of_play_beside_a_listed_one_in_play(bc, alg):
    """The rescoring stage scans the spill list only if a block in play says -1: here none does, the 20 pairs stay unread and
    the count is cleared all the same."""
    phi, rows = idle_spill_phi()
    mode = 0 if alg == 'giga' else 1
    sv = warm_solver(bc, alg, phi)
    i, blk, grid = geometry(sv, 4)
    begin(sv, 2)
    ul8, out, rep = diagnostic(sv, mode, blk, grid, 'idle spill %s' % alg, allow_give_up=False)
    print('idle spill %s: blk_l %s blk_u %s' % (alg, out['blk_l'].tolist(), out['blk_u'].tolist()))
    assert rep[1][0] == 5 and rep[1][2] == 5 and rep[2][0] == 20 and rep[2][2] == -1 and out['count'] == 20
    assert out['blk_u'][2] < out['blk_l'].max()                              # block 2 is not in play
    native().call('bc_snnls_step_local', sv._eng.h)
    prod = outputs(sv, 'ctrl')
    native().call('bc_snnls_step_finish', sv._eng.h)
    assert held_to(ul8, prod, blk, grid, allow_give_up=False) == rep and prod['count'] == 20
    assert spill_count(sv) == 0
    native().call('bc_snnls_step_local', sv._eng.h)
    native().call('bc_snnls_step_finish', sv._eng.h)
    assert spill_count(sv) == 0 and end(sv) == (2, 0)
    assert int(sv._eng.trace()[0][0]) == rows[1][0]
    with prefilter(0):
        ref = solver_class(bc, alg)(phi.T, phi.sum(axis=0))
    ref.build(2)
    assert np.array_equal(sv._eng.trace()[0], ref._eng.trace()[0])


# ------------------------------------------------------------------ (c) the consumers
def fp64_run(bc, name, alg):
    if (name, alg) not in _REF:
        phi, _ = case_phi(name)
        ref = warm_solver(bc, alg, phi, form=0)
        assert ref._eng.prefilter == 0
        ref.build(12)
        idx, val = ref._eng.sparse_weights()
        _REF[name, alg] = (ref._eng.trace(), idx, val, ref.error())
    return _REF[name, alg]


@pytest.mark.parametrize('knob', list(KNOBS), ids=lambda k: k or 'fused')
@pytest.mark.parametrize('alg', ['giga', 'fw'])
@pytest.mark.parametrize('name', list(CASES))
def test_twelve_steps_under_every_finish_form(bc, name, alg, knob):
    """The first step apart (build(1), then build(11): the trace, weights and error of one build(12), as
    test_two_level_form_across_reset_and_repeated_build_calls holds) so that its fallbacks can be read."""
    phi, rows = case_phi(name)
    sv = warm_solver(bc, alg, phi, knob=knob)
    falls = sv._eng.prefilter_fallbacks()
    sv.build(1)
    first = sv._eng.prefilter_fallbacks() - falls
    assert sv._eng.finish_form() == (KNOBS[knob] if name not in GIVES_UP else (PLAIN if knob == 'BC_FINISH_NOPF' else ONE_ROUND))
    sv.build(11)
    total = sv._eng.prefilter_fallbacks() - falls
    print('%s %s %s: fallbacks %d in the first step, %d in twelve; two-level sweeps %d' % (name, alg, knob or 'fused', first, total,
                                                                                          sv._eng.prefilter_levels()[0]))
    idx, val = sv._eng.sparse_weights()
    got = (sv._eng.trace(), idx, val, sv.error())
    same(got, fp64_run(bc, name, alg))
    if name in GIVES_UP:
        assert first >= 1 and total >= 1
    else:
        assert first == 0
    planted = np.concatenate(list(rows.values()))
    f0 = int(got[0][0][0])
    assert f0 in planted and (not CASES[name][2] or f0 == planted.min())     # of exact ties, the lowest index


def test_ctrl_swept_is_there_after_a_two_level_diagnostic_sweep(bc):
    """The buffer "ctrl_swept" is the test aid's own: a solver that never ran a two-level diagnostic sweep has none; after one it
    holds what the sweep left, and "ctrl" what it held before."""
    N = native()
    phi, _ = case_phi('k9')
    with prefilter(4):
        sv = bc.snnls.GIGA(phi.T, phi.sum(axis=0))
    buf = np.empty(256, dtype=np.uint8)
    for _ in range(2):                                                       # fresh; after the one-level sweep of the first step
        rc = N.load().bc_snnls_prefdiag_copy(sv._eng.h, b'ctrl_swept', buf.ctypes.data_as(C.c_void_p), 256, None)
        assert rc == N.BC_INVALID_ARGUMENT and 'has no buffer' in N.last_error()
        sv.build(1)
        sv.reset()
    begin(sv, 0)
    before = fetch(sv, 'ctrl', np.int32).copy()
    assert sweep(sv, 0)[0] == 3
    swept = fetch(sv, 'ctrl_swept', np.int32)
    assert swept[SPILL_N] == 9 and before[SPILL_N] == 0 and np.array_equal(fetch(sv, 'ctrl', np.int32), before)
    end(sv)
