"""The solver's three counter entries (bc_snnls_prefilter_fallbacks, _stats, _levels) against the pre-filter's raw control block,
fetched through the diagnostic seam ("ctrl": 64 ints, include/beta_cores_prefdiag.h) and read here by the word positions that
csrc/bc_pref_ctrl.h names: overflows at word 3, u64 sweeps at 4, u64 rows rescored at 6, u64 rows passed on by the first level
at 12.  Once per form of the pre-filter -- each form's kernels write the block themselves -- and per algorithm mode, at
3000 rows x S = 20: 12 int8 tiles and 6 fp16 tiles, the last one ragged, more than one tile per wave."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_prefilter import correlated, prefilter, same                 # noqa: E402
from test_gpu_pref_bounds import fetch                                      # noqa: E402

pytestmark = pytest.mark.gpu

N_ROWS, S, STEPS = 3000, 20, 12
W_OVERFLOWS, W_SWEEPS, W_RESCORED, W_L1_PASSED = 3, 4, 6, 12


@pytest.fixture(scope='module')
def bc():
    import beta_cores_amd as bc
    bc.default_context()
    return bc


@pytest.fixture(scope='module')
def phi():
    return correlated(np.random.RandomState(20), N_ROWS, S)


def block(sv):
    ctrl = fetch(sv, 'ctrl', np.int32)
    assert ctrl.size == 64
    u64 = lambda w: int(ctrl[w:w + 2].copy().view(np.uint64)[0])
    return int(ctrl[W_OVERFLOWS]), u64(W_SWEEPS), u64(W_RESCORED), u64(W_L1_PASSED)


def entries_equal_block(sv, two_level=False):
    """The three entries against the block; returns (overflows, sweeps, rescored, l1_sweeps, passed)."""
    falls = sv._eng.prefilter_fallbacks()
    stats = sv._eng.prefilter_stats()
    l1, listed, refined = sv._eng.prefilter_levels()
    overflows, sweeps, rescored, passed = block(sv)
    print('block: overflows %d sweeps %d rescored %d passed on %d | fallbacks %d stats %s levels %s'
          % (overflows, sweeps, rescored, passed, falls, stats, (l1, listed, refined)))
    assert falls == overflows
    assert stats == (sweeps, rescored, overflows)
    if two_level:
        assert listed == refined == passed
    else:
        assert (l1, listed, refined) == (0, 0, 0)
    return overflows, sweeps, rescored, l1, passed


def solver(bc, alg, phi, on, cap=None):
    cls = bc.snnls.GIGA if alg == 'giga' else bc.snnls.FrankWolfe
    with prefilter(on, cap):
        sv = cls(phi.T, phi.sum(axis=0))
    return sv


FORMS = {'int8': (8, 1), 'fp16': (16, 1), 'fp32': (32, 1), 'two_level': (4, 3), 'bb': (8, 2)}


@pytest.mark.parametrize('alg', ['giga', 'fw'])
@pytest.mark.parametrize('form', sorted(FORMS))
def test_entries_read_the_block(bc, phi, monkeypatch, form, alg):
    on, want_form = FORMS[form]
    monkeypatch.setenv('BC_I8_BB', '1' if form == 'bb' else '0')
    monkeypatch.setenv('BC_I8_BLKLIST', '0')
    sv = solver(bc, alg, phi, on)
    assert sv._eng.prefilter == (8 if on == 4 else on) and sv._eng.prefilter_form == want_form
    two = form == 'two_level'
    assert entries_equal_block(sv, two) == (0, 0, 0, 0, 0)            # a new solver: the block is zero
    sv.build(STEPS)
    overflows, sweeps, rescored, l1, passed = entries_equal_block(sv, two)
    steps_swept = len(sv._eng.trace()[0])
    assert overflows == 0 and steps_swept == STEPS                    # (the premise of the two counts below: no step was redone or skipped)
    assert sweeps == steps_swept
    assert rescored > 0                                               # (a live counter: the winner at least is rescored)
    if two:
        assert l1 == STEPS - 1                                        # the first sweep has no seeds: plain int8
        assert passed > 0                                             # (its value depends on the block scheduling: not asserted)


def test_overflow_is_counted_and_changes_nothing(bc, phi, monkeypatch):
    monkeypatch.setenv('BC_I8_BB', '0')
    monkeypatch.setenv('BC_I8_BLKLIST', '0')
    first = solver(bc, 'giga', phi, 0)
    first.build(1)
    winner = int(first._eng.trace()[0][0])
    planted = phi.copy()
    others = np.setdiff1d(np.arange(N_ROWS), [winner])
    planted[np.random.RandomState(21).choice(others, 40, replace=False)] = phi[winner]      # 40 exact copies of the winning row
    res = []
    for on, cap in ((8, 1), (0, None)):
        sv = solver(bc, 'giga', planted, on, cap)
        sv.build(STEPS)
        idx, val = sv._eng.sparse_weights()
        res.append((sv._eng.trace(), idx, val, sv.error()))
        if on:
            overflows = entries_equal_block(sv)[0]
            assert overflows > 0
    same(res[0], res[1])
