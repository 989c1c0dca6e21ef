"""The hand-over of the two-level sweep (csrc/bc_prefilter_i4.h: k_sweep_i4) to the rescoring stage, pair by pair, for all three
codes a sweep block can leave in blk_nc -- no test in this module; tests/test_handover_cases_cpu.py shows that the checker can
fail, tests/test_gpu_handover.py holds the device to it.

Per sweep block b, from the per-row level-2 values (U8, L8; NaN where level 2 did not re-bound the row):

    done_b = the rows of b's tiles that were re-bounded
    best_b = max L8 over done_b
    want_b = {(bits of U8, row) : row in done_b, U8 >= best_b}          the rows "in play"

  code 0 .. 8   exactly want_b in the block's own list (BC_BLK_NC = 8 pairs)
  code -1       8 < |want_b| <= 512, every pair of want_b in spill[0 : count]
  code -2       the block gave up: it held more than BC_L2_LCAP = 512 rows, or the spill list (BC_PREF_SPILL_CAP = 4096) is full

and, when no block gave up, spill[0 : count] is the union of want_b over the -1 blocks AS A MULTISET: no pair missing, none
stale, none repeated.

The number of rows a block HOLDS lies between |want_b| and |done_b|: a re-bounded row is held if its U8 reaches the best L8 the
block had seen WHEN the row was re-bounded, which depends on the order of the waves' atomics.  A block with
|want_b| <= 512 < |done_b| may therefore legitimately say -2, -1 or a count; the checker refuses such a block by name instead of
accepting all three -- cases are built so that none occurs."""
import collections

import numpy as np

BLK_NC = 8          # BC_BLK_NC
L2_LCAP = 512       # BC_L2_LCAP
SPILL_CAP = 4096    # BC_PREF_SPILL_CAP
TILE = 256
BAND = 'the order-dependent band'


def bits(u):
    return int(np.float32(u).view(np.uint32))


def per_block(ul8, blk_of_tile, grid):
    """[(done rows, best, want)] per block; want: the set of (U8 bits, row)."""
    ul8 = np.asarray(ul8, dtype=np.float32)
    done = ~np.isnan(ul8[:, 0])
    rb = np.repeat(np.asarray(blk_of_tile), TILE)
    assert len(rb) == len(ul8)
    out = []
    for b in range(grid):
        rows_b = np.nonzero(done & (rb == b))[0]
        best = np.max(ul8[rows_b, 1]) if len(rows_b) else np.float32(-np.inf)
        umax = np.max(ul8[rows_b, 0]) if len(rows_b) else np.float32(-np.inf)
        want = set((bits(ul8[r, 0]), int(r)) for r in rows_b if ul8[r, 0] >= best)
        out.append((rows_b, best, umax, want))
    return out


def check_handover(ul8, blk_nc, blk_cand, blk_l, blk_u, spill, count, blk_of_tile, grid, allow_give_up=True):
    """ul8 [rows][2] float32; blk_nc [grid]; blk_cand [grid][8][2] int32 (U bits, row); blk_l [grid] float64; blk_u [grid] float32;
    spill [4096][2] int32; count: BC_PCTL_SPILL_N as the sweep left it; blk_of_tile [tiles] -> block.
    Returns {block: (|want_b|, |done_b|, code)} for the blocks that re-bounded anything."""
    blk_nc = np.asarray(blk_nc)
    blk_cand = np.asarray(blk_cand).reshape(grid, BLK_NC, 2)
    spill = np.asarray(spill).reshape(-1, 2)
    count = int(count)
    assert len(spill) == SPILL_CAP and len(blk_nc) == grid
    assert count >= 0, 'spill count %d' % count
    held = spill[:min(count, SPILL_CAP)]
    have = collections.Counter((int(u) & 0xffffffff, int(r)) for u, r in held)
    need = collections.Counter()
    owner = {}
    report = {}
    gave_up = [b for b in range(grid) if blk_nc[b] == -2]
    for b, (rows_b, best, umax, want) in enumerate(per_block(ul8, blk_of_tile, grid)):
        nw, nd, code = len(want), len(rows_b), int(blk_nc[b])
        tag = 'block %d (code %d, %d pairs in play, %d rows re-bounded)' % (b, code, nw, nd)
        assert blk_l[b] == np.float64(best), tag + ': blk_l'                    # maxima of floats are exact
        assert blk_u[b] == umax, tag + ': blk_u'
        assert -2 <= code <= BLK_NC, tag + ': no such code'
        assert not (nw <= L2_LCAP < nd), tag + ' lies in %s: its code depends on the order of the atomics' % BAND
        if nd:
            report[b] = (nw, nd, code)
        if nw <= BLK_NC:
            assert code == nw, tag + ': %d pairs fit the list of %d' % (nw, BLK_NC)
            got = [(int(u) & 0xffffffff, int(r)) for u, r in blk_cand[b, :code]]
            assert len(set(got)) == len(got) and set(got) == want, tag + ': the list is not the pairs in play'
            continue
        assert code < 0, tag + ': a list of %d cannot hold %d pairs' % (BLK_NC, nw)
        if nw > L2_LCAP:
            assert code == -2, tag + ': more than %d pairs cannot be held' % L2_LCAP
        if code == -2:
            assert allow_give_up, tag + ' gave up'
            # (outside the band nd > 512 means nw > 512: the block could not hold its pairs whatever the order)
            assert nd > L2_LCAP or count > SPILL_CAP, tag + ': gave up with %d rows re-bounded and a spill count of %d' % (nd, count)
            continue
        assert count <= SPILL_CAP or gave_up, tag + ': spill count %d above the cap and no block gave up' % count
        for pr in want:
            owner[pr] = b
        need.update(want)
        missing = [pr for pr in want if have[pr] == 0]
        assert not missing, tag + ': %d of its pairs are not in spill[0:%d], first (U bits %#x, row %d)' % ((len(missing), count) + missing[0])
    total = sum(need.values())
    if gave_up:
        assert count >= total, 'the -1 blocks hand over %d pairs, the spill count is %d' % (total, count)
    else:
        extra = have - need
        spilled = ', '.join('block %d' % b for b in sorted(set(owner.values()))) or 'no block'
        whose = sorted(set(owner.get(pr, -1) for pr in extra))
        assert not extra, '%s spilled %d pairs; spill[0:%d] also holds %d that are stale or repeated (of blocks %s; -1: of no block), first ' \
            '(U bits %#x, row %d)' % ((spilled, total, count, sum(extra.values()), whose) + next(iter(extra)))
        assert count == total, '%s spilled %d pairs, the spill count is %d' % (spilled, total, count)
    return report
