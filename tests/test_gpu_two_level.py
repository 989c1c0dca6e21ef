"""The two-level sweep (csrc/bc_prefilter_i4.h: k_sweep_i4<MODE, U>, a 4-bit first level, int8 records behind it) at the shapes
its code depends on, each against the fp64 sweep (BC_PREFILTER=0) with the comparison of tests/test_gpu_prefilter.py (`same`:
trace arrays, weight indices and values, error, all bit-identical):

  * every (U, batches per tile, lines per int8 record) class of S = 1 .. 256 (tests/two_level_shapes.py): the five template
    instances, one to five batches per 256-row tile (the `U < SP8` prologue, the turn-overs of the two register buffers
    inside and at the end of a tile), records of one, two and three cache lines (`nch > 1` in bc_r8_interval);
  * walks of several tiles per wave at a few hundred thousand rows (BC_PREF_WAVES_PER_CU=1): the steady state of the
    two-buffer loop, theta tightening along the walk, the hand-over of the next tile's row codes;
  * hundreds of rows in play inside ONE block's tiles: the level-2 pass in the middle of a walk (more than 128 rows parked),
    the spill list behind the per-block list of 8, and the exit to the exact sweep past 512 rows in play;
  * the host's watch putting the first level aside BETWEEN two steps of one build call and probing it again 256 sweeps later.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_prefilter import correlated, prefilter, run, same            # noqa: E402
from two_level_shapes import S_LIST, class_of, rounds                      # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def bc():
    import beta_cores_amd as bc
    bc.default_context()
    return bc


@pytest.fixture(scope='module', autouse=True)
def release_device_matrices():
    yield
    long_walk_phi.cache_clear()
    concentrated_phi.cache_clear()


def solver_class(bc, alg):
    return bc.snnls.GIGA if alg == 'giga' else bc.snnls.FrankWolfe


def form_now(sv):
    """The sweep form the solver would use for its next step (3 two-level, 1 the one-level int8 sweep)."""
    from beta_cores_amd import _native as N
    form = C.c_int()
    N.call('bc_snnls_prefilter_form', sv._eng.h, C.byref(form))
    return form.value


def run_two_level(cls, phi, steps, warm=False):
    """`run(bc, cls, phi, steps, 4)` that also hands back the solver (its counters are part of what these tests assert).
    warm: one step and a reset first -- the first sweep of a solver has no seeds and is the int8 one; after it the two-level
    form serves the first step of the run as well (test_two_level_form_across_reset_and_repeated_build_calls: a reset solver
    returns what a fresh one returns)."""
    with prefilter(4):
        sv = cls(phi.T, phi.sum(axis=0))
    assert sv._eng.prefilter == 8 and sv._eng.prefilter_form == 3
    if warm:
        sv.build(1)
        sv.reset()
        assert sv._eng.prefilter_levels()[0] == 0 and form_now(sv) == 3
    sv.fallbacks_before = sv._eng.prefilter_fallbacks()
    sv.build(steps)
    tr = sv._eng.trace()
    idx, val = sv._eng.sparse_weights()
    return (tr, idx, val, sv.error()), sv


def served_by_the_two_level_sweep(sv, steps):
    """At least 90 % of the steps came from the two-level sweep: that many were launched in this form (the first sweep of a solver
    has no seeds and is the int8 one), and no more than the remaining tenth were redone by the exact sweep -- a redo cannot
    stand in for the form under test."""
    l1, listed, refined = sv._eng.prefilter_levels()
    falls = sv._eng.prefilter_fallbacks()
    print('two-level sweeps %d of %d steps, rows listed %d, exact redos %d' % (l1, steps, listed, falls))
    need = -(-9 * steps // 10)
    assert l1 >= need, (l1, steps)
    assert falls <= steps - need, (falls, steps)
    assert listed > 0


# ------------------------------------------------------------------ every batch class
@pytest.mark.parametrize('alg', ['giga', 'fw'])
@pytest.mark.parametrize('s', S_LIST, ids=lambda s: 'S%d-U%d-b%d-l%d' % ((s,) + class_of(s)))
def test_every_batch_class(bc, s, alg):
    """20 011 rows (79 tiles, the last one ragged), S from every class; 20 exact duplicate pairs at scattered rows (ties the 4-bit
    and the int8 level must both pass on, lowest index wins)."""
    rng = np.random.RandomState(7000 + s)
    n = 20_011
    phi = correlated(rng, n, s)
    where = rng.choice(n, 40, replace=False)
    phi[where[20:]] = phi[where[:20]]
    dphi = bc.DevicePhi.from_host(phi)
    cls = solver_class(bc, alg)
    got, sv = run_two_level(cls, dphi, 60)
    same(got, run(bc, cls, dphi, 60, 0))
    served_by_the_two_level_sweep(sv, 60)


# ------------------------------------------------------------------ long walks
def n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=1)
def long_walk_phi(r, s, cu):
    """256 r cu - 100 rows: with one wave per CU every wave walks r tiles (the last wave's last tile is ragged).  Kept on the
    device for the two solvers and both algorithms of a case."""
    import beta_cores_amd as bc
    n = 256 * r * cu - 100
    phi = correlated(np.random.RandomState(100 * r + s), n, s)
    return bc.DevicePhi.from_host(phi)


LONG_WALKS = [(7, 40), (7, 72), (7, 100), (7, 200), (3, 253)]


@pytest.mark.parametrize('r,s,alg', [(r, s, alg) for r, s in LONG_WALKS for alg in ('giga', 'fw')])
def test_long_walks(bc, monkeypatch, r, s, alg):
    """R = 7 tiles per wave at one batch per tile (S = 40), two (72), one of 13 loads (100) and five (200: an odd count, the
    buffers change roles from tile to tile); R = 3 with three-line records (253)."""
    monkeypatch.setenv('BC_PREF_WAVES_PER_CU', '1')
    cu = n_cu()
    dphi = long_walk_phi(r, s, cu)
    n = dphi.shape[0]
    assert n == 256 * r * cu - 100 and rounds(n, cu, 1) == r
    cls = solver_class(bc, alg)
    steps = 40 if alg == 'giga' else 25
    got, sv = run_two_level(cls, dphi, steps)
    same(got, run(bc, cls, dphi, steps, 0))
    served_by_the_two_level_sweep(sv, steps)


# ------------------------------------------------------------------ candidates concentrated in one block
@functools.lru_cache(maxsize=1)
def concentrated_phi(case, cu):
    """R = 5, S = 64.  Rows 0 .. k-1 are copies of the row that tops the first step's scores (as the clusters of
    test_clusters_of_near_duplicates do at their size; at this one the row has to be chosen): with one wave per CU tiles
    0 .. 3 belong to the four waves of block 0, so the copies sit in one block's tiles.  They tie (B) or nearly tie (A) at the
    top of the FIRST step's scores, which the tests below let the two-level form serve; under GIGA they are parallel to the
    iterate in the second step as well (no usable bound: every one of them is passed on).  A NumPy run of the two algorithms
    on these data selects no copy after the first step: without the warm start Frank-Wolfe would never see them in play."""
    import beta_cores_amd as bc
    n, s = 256 * 5 * cu - 100, 64
    rng = np.random.RandomState(41)
    phi = correlated(rng, n, s)
    top = int(np.argmax(phi.dot(phi.sum(axis=0)) / np.linalg.norm(phi, axis=1)))
    src = phi[top].copy()
    phi[top] = correlated(rng, 1, s)[0]                   # (the original goes: the copies are the only rows at the top)
    k = 300 if case == 'A' else 700
    phi[:k] = src * (1. + 1e-9 * rng.randn(k, s)) if case == 'A' else src
    score = phi.dot(phi.sum(axis=0)) / np.linalg.norm(phi, axis=1)
    assert score[:k].min() > score[k:].max()              # the data do what they are for
    return bc.DevicePhi.from_host(phi), k


@pytest.mark.parametrize('case,alg', [(c, a) for c in 'AB' for a in ('giga', 'fw')])
def test_candidates_concentrated_in_one_block(bc, monkeypatch, case, alg):
    """A: 300 copies perturbed at 1e-9 in tiles 0 and 1 -- a wave parks more than 128 rows (level 2 runs in the middle of its
    walk) and block 0 is left with more than 8 rows in play (the spill list).  B: 700 exact copies in tiles 0 .. 2 -- more than
    512 rows in play, the step is redone by the exact sweep; the lowest index wins among the ties, as in the fp64 sweep.
    (The solver has taken one step and been reset, so that the first of the 30 steps is a two-level sweep too.)"""
    monkeypatch.setenv('BC_PREF_WAVES_PER_CU', '1')
    cu = n_cu()
    dphi, k = concentrated_phi(case, cu)
    assert rounds(dphi.shape[0], cu, 1) == 5
    cls = solver_class(bc, alg)
    got, sv = run_two_level(cls, dphi, 30, warm=True)
    same(got, run(bc, cls, dphi, 30, 0))
    first = int(got[0][0][0])
    assert first < k and (case == 'A' or first == 0)      # a copy is selected first; of the exact ties, the lowest index
    l1, listed, _ = sv._eng.prefilter_levels()
    print('case %s %s: two-level sweeps %d, rows listed %d, exact redos %d' % (case, alg, l1, listed, sv._eng.prefilter_fallbacks()))
    if case == 'B':
        assert sv._eng.prefilter_fallbacks() - sv.fallbacks_before >= 1


# ------------------------------------------------------------------ the watch: mid-call and re-probe
def test_watch_mid_call_and_reprobe(bc):
    """The data of test_two_level_watch_puts_the_first_level_aside_where_it_does_not_select (the first level passes on more than
    4 % of the rows).  build(70): the look after step 64 of the call puts the first level aside between two enqueued steps, the
    last 6 are int8 sweeps.  build(340): the 256th int8 sweep since then falls at the call's fourth look, which turns the first
    level on again (its seeds are 250 steps old); the fifth look, 64 two-level sweeps later, puts it aside again.  Selections
    are the fp64 sweep's throughout."""
    import torch
    g = torch.Generator(device='cuda'); g.manual_seed(11)
    n, d, s = 400_000, 32, 100
    Z = torch.randn((n, d + 1), generator=g, dtype=torch.float64, device='cuda')
    th = np.random.default_rng(1).standard_normal((s, d)) * 0.3
    phi = bc.DeviceProjector(lambda k, w, p: th, s, bc.likelihoods.LinearRegression(1.0)).project(bc.DeviceData.from_torch(Z))
    with prefilter(4):
        sv = bc.snnls.GIGA(phi.T, phi.colsum())
    assert sv._eng.prefilter_form == 3
    sv.build(70)
    l1, listed, _ = sv._eng.prefilter_levels()
    print('after build(70): two-level sweeps %d, rows listed %d (%.3f of the rows per sweep)' % (l1, listed, listed / (max(l1, 1) * n)))
    assert 4 <= l1 <= 64 and listed > 0.04 * l1 * n          # (the precondition: these data trigger the watch)
    assert form_now(sv) == 1                                 # put aside inside the call: at its end too few int8 sweeps for a probe
    sv.build(340)
    l1b = sv._eng.prefilter_levels()[0]
    print('after build(340): two-level sweeps %d' % l1b)
    assert l1b >= l1 + 4                                     # the re-probe ran ...
    assert form_now(sv) == 1                                 # ... and was put aside again
    tr = sv._eng.trace()
    idx, val = sv._eng.sparse_weights()
    with prefilter(0):
        ref = bc.snnls.GIGA(phi.T, phi.colsum())
    assert ref._eng.prefilter == 0
    ref.build(410)
    ridx, rval = ref._eng.sparse_weights()
    same((tr, idx, val, sv.error()), (ref._eng.trace(), ridx, rval, ref.error()))
