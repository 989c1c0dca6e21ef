"""tests/handover_cases.py can fail: a synthetic hand-over of six sweep blocks that is right passes, and each way a block or the
spill list can be wrong is refused with a message that names the block.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import handover_cases as H                                                  # noqa: E402

GRID, TILES = 6, 24
BLK = np.arange(TILES) // 4                                                 # block b owns tiles 4b .. 4b+3
#          rows in play, rows re-bounded below the best lower bound
SHAPE = {0: (8, 30), 1: (9, 0), 2: (300, 200), 3: (513, 0), 4: (0, 0), 5: (3, 497)}
CODE = {0: 8, 1: -1, 2: -1, 3: -2, 4: 0, 5: 3}


def hand_over():
    """Per-row values and the lists a correct sweep leaves for them.  In play: U8 = 0.9 + a few ulps (distinct bit patterns),
    L8 = 0.85 for one row (the block's best) and lower for the rest; not in play: U8 < 0.85."""
    rng = np.random.RandomState(5)
    ul8 = np.full((TILES * 256, 2), np.nan, dtype=np.float32)
    nc = np.zeros(GRID, dtype=np.int32)
    cand = np.full((GRID, 8, 2), -7, dtype=np.int32)
    blk_l = np.full(GRID, -np.inf)
    blk_u = np.full(GRID, -np.inf, dtype=np.float32)
    spill = np.full((H.SPILL_CAP, 2), -1, dtype=np.int32)
    count = 0
    for b in (2, 0, 5, 1, 3, 4):                                             # (the spill list is not in block order)
        k, low = SHAPE[b]
        rows = 1024 * b + rng.choice(1024, k + low, replace=False)
        for j, r in enumerate(rows[:k]):
            ul8[r] = (np.float32(0.9) + np.float32(j % 7) * np.float32(2.0 ** -23), np.float32(0.85 if j == 0 else 0.8))
        for r in rows[k:]:
            ul8[r] = (np.float32(0.84), np.float32(0.7))
        if k + low:
            blk_l[b], blk_u[b] = np.max(ul8[rows, 1]), np.max(ul8[rows, 0])
        pairs = [(H.bits(ul8[r, 0]), int(r)) for r in rng.permutation(rows[:k])]
        nc[b] = CODE[b]
        if CODE[b] > 0:
            cand[b, :k] = pairs
        elif CODE[b] == -1:
            spill[count:count + k] = pairs
            count += k
    return dict(ul8=ul8, blk_nc=nc, blk_cand=cand, blk_l=blk_l, blk_u=blk_u, spill=spill, count=count, blk_of_tile=BLK, grid=GRID)


def check(h, **kw):
    return H.check_handover(h['ul8'], h['blk_nc'], h['blk_cand'], h['blk_l'], h['blk_u'], h['spill'], h['count'], h['blk_of_tile'], h['grid'], **kw)


def without(h, b):
    """The hand-over with block b's rows not re-bounded at all (and its spilled pairs gone)."""
    h = dict((k, np.copy(v)) for k, v in h.items())
    rows = slice(1024 * b, 1024 * (b + 1))
    keep = [i for i in range(int(h['count'])) if not 1024 * b <= h['spill'][i, 1] < 1024 * (b + 1)]
    h['ul8'][rows] = np.nan
    h['spill'][:len(keep)] = h['spill'][keep]
    h['spill'][len(keep):] = -1
    h['count'] = len(keep)
    h['blk_nc'][b], h['blk_l'][b], h['blk_u'][b] = 0, -np.inf, -np.inf
    return h


def test_a_correct_hand_over_passes():
    h = hand_over()
    rep = check(h)
    assert rep == {0: (8, 38, 8), 1: (9, 9, -1), 2: (300, 500, -1), 3: (513, 513, -2), 5: (3, 500, 3)} and h['count'] == 309
    with pytest.raises(AssertionError, match=r'block 3 .*gave up'):
        check(h, allow_give_up=False)
    assert 3 not in check(without(h, 3), allow_give_up=False)               # (without a give-up the multiset rule applies: it holds)


def spilled_by(h, b):
    return [i for i in range(int(h['count'])) if 1024 * b <= h['spill'][i, 1] < 1024 * (b + 1)]


def drop_a_pair(h):
    i = spilled_by(h, 2)[17]
    h['spill'][i:-1] = h['spill'][i + 1:].copy()                             # (the count stays: the last slot reads what was behind it)
    return r'block 2 .*1 of its pairs are not in spill'


def stale_pair(h):
    i = spilled_by(h, 2)[40]
    free = [r for r in range(2048, 3072) if np.isnan(h['ul8'][r, 0])][0]      # a row of the same block level 2 never saw
    h['spill'][i] = (h['spill'][i, 0], free)
    return r'block 2 .*1 of its pairs are not in spill'


def repeat_a_pair(h):
    n = int(h['count'])
    h['spill'][n] = h['spill'][spilled_by(h, 1)[3]]
    h['count'] = n + 1
    return r'block 1, block 2 spilled 309 pairs; spill\[0:310\] also holds 1 that are stale or repeated \(of blocks \[1\]'


def count_one_too_large(h):
    h['count'] = int(h['count']) + 1
    return r'block 1, block 2 spilled 309 pairs; spill\[0:310\] also holds 1 that are stale or repeated \(of blocks \[-1\]'


def spill_code_on_eight(h):
    h['blk_nc'][0] = -1
    return r'block 0 \(code -1, 8 pairs in play, 38 rows re-bounded\): 8 pairs fit the list'


def list_on_nine(h):
    h['blk_nc'][1] = 8
    h['blk_cand'][1] = h['spill'][spilled_by(h, 1)[:8]]
    return r'block 1 \(code 8, 9 pairs in play, 9 rows re-bounded\): a list of 8 cannot hold 9'


def give_up_on_500(h):
    h['blk_nc'][2] = -2
    return r'block 2 \(code -2, 300 pairs in play, 500 rows re-bounded\): gave up with 500 rows re-bounded and a spill count of 309'


def spill_code_on_513(h):
    h['blk_nc'][3] = -1
    return r'block 3 \(code -1, 513 pairs in play, 513 rows re-bounded\): more than 512 pairs cannot be held'


MUTATIONS = [drop_a_pair, stale_pair, repeat_a_pair, count_one_too_large, spill_code_on_eight, list_on_nine, give_up_on_500, spill_code_on_513]


@pytest.mark.parametrize('mutate', MUTATIONS, ids=lambda f: f.__name__)
def test_every_mutation_is_refused_by_name(mutate):
    h = hand_over()
    if mutate not in (give_up_on_500, spill_code_on_513):
        h = without(h, 3)                                                    # no block gives up: the multiset rule is in force
        check(h, allow_give_up=False)
    message = mutate(h)
    with pytest.raises(AssertionError, match=message):
        check(h)


def test_dropped_pair_is_seen_next_to_a_block_that_gave_up():
    """With a -2 block the list is no longer compared as a multiset, but every pair of a -1 block must still be there."""
    h = hand_over()
    message = drop_a_pair(h)
    h['spill'][int(h['count']) - 1] = -1
    with pytest.raises(AssertionError, match=message):
        check(h)


def test_the_band_is_refused_by_name():
    h = hand_over()
    k, low = 20, 500                                                         # 20 pairs in play, 520 rows re-bounded
    h = without(h, 1)
    rows = 1024 + np.arange(k + low)
    h['ul8'][rows[:k]] = (np.float32(0.9), np.float32(0.85))
    h['ul8'][rows[k:]] = (np.float32(0.84), np.float32(0.7))
    h['blk_l'][1], h['blk_u'][1], h['blk_nc'][1] = np.float32(0.85), np.float32(0.9), -2
    with pytest.raises(AssertionError, match=r'block 1 .*lies in ' + H.BAND):
        check(h)


def test_a_full_spill_list():
    """Ten blocks of 450: nine fit below the cap of 4096, the tenth gives up; the count says 4500."""
    grid = 12
    blk = np.arange(4 * grid) // 4
    ul8 = np.full((4 * grid * 256, 2), np.nan, dtype=np.float32)
    nc = np.zeros(grid, dtype=np.int32)
    blk_l = np.full(grid, -np.inf)
    blk_u = np.full(grid, -np.inf, dtype=np.float32)
    spill = np.full((H.SPILL_CAP, 2), -1, dtype=np.int32)
    at = 0
    for b in range(10):
        rows = 1024 * b + 2 * np.arange(450)
        ul8[rows] = (np.float32(0.5), np.float32(0.25))
        blk_l[b], blk_u[b] = 0.25, 0.5
        nc[b] = -1 if b != 6 else -2
        if b != 6:
            spill[at:at + 450] = [(H.bits(0.5), int(r)) for r in rows]
            at += 450
    args = (ul8, nc, np.zeros((grid, 8, 2), dtype=np.int32), blk_l, blk_u)
    rep = H.check_handover(*args, spill, 4500, blk, grid)
    assert rep[6] == (450, 450, -2) and rep[9] == (450, 450, -1)
    with pytest.raises(AssertionError, match=r'block 6 .*gave up with 450 rows re-bounded and a spill count of 4050'):
        H.check_handover(*args, spill, 4050, blk, grid)
    spill[4049] = -1
    with pytest.raises(AssertionError, match=r'block 9 .*1 of its pairs are not in spill'):
        H.check_handover(*args, spill, 4500, blk, grid)
