"""The batched BatchPSVI run on the device at the edges of its tiles and at its limits (tests/psvi_many_edge_cases.py): every
stage of the last step through the seam at the shapes of the two tables; a ragged batch whose largest problem has 17 point tiles;
the evaluation drivers' shape (sizes 1 .. 200 in one run); the problem count at its limit; the cases whose result is exact; and
float32 rows of a whole wave instruction and more.  The bounds are those of tests/psvi_many_cases.py and
tests/psvi_many_gauss_cases.py, unchanged; the matrix-core and cross-lane branches of bc_pm_tile, bc_pm_post_products and
bc_vil_gram, which no host build compiles, run here.  The worst error / bound per stage is printed (lines that begin with EDGE;
profiles/psvi_many_notes.md and profiles/psvi_many_gauss_notes.md keep the figures of one MI355X)."""
import numpy as np
import pytest

import psvi_many_edge_cases as ec

pytestmark = pytest.mark.gpu
KINDS = [ec.LOGISTIC, ec.GAUSS]
RAGGED = [1, 16, 17, 32, 33, 64, 65, 255, 256, 257]


@pytest.fixture(scope='module')
def bc():
    import beta_cores_amd as bc
    bc.default_context()
    return bc


def _steps(H, row):
    """two steps, so that the moments are not zero before the checked one; one where the host's long-double work is the longest"""
    d, m, s, n_sub = row[:4]
    return 1 if n_sub == H['BC_PSVI_MANY_MAX_SUB'] or (d, m) == (H['BC_VI_MAX_DIM'], H['BC_PSVI_MANY_MAX_POINTS']) else 2


# ---------------------------------------------------------------- a. the stages at the table shapes
@pytest.mark.parametrize('kind,row', [(k, r) for k in KINDS for r in ec.TABLES[k]], ids=lambda v: v if isinstance(v, str) else ec.row_id(v))
def test_stages_at_the_table_shapes(bc, kind, row):
    d, m, s, n_sub, diag, n_rows = row
    r = ec.Run(bc, kind, d, s, n_sub, _steps(ec.header_constants(), row), diag=diag, sizes=[m], n_rows=n_rows)
    ec.check_last_step(r)


# ---------------------------------------------------------------- b. a ragged batch
@pytest.mark.parametrize('kind', KINDS)
def test_a_ragged_batch(bc, kind):
    """17 point tiles in the grid of k_pm_ll, of which problem 0 uses one: every problem's stages, and the bits of each problem
    alone and of the batch in reverse order."""
    whole = ec.Run(bc, kind, 5, 17, 17, 2, sizes=RAGGED)
    assert whole.res['marked'] == []
    ec.check_last_step(whole)
    for m in (1, 16, 257):
        assert ec.Run(bc, kind, 5, 17, 17, 2, sizes=[m]).same_bits(whole, [0], [RAGGED.index(m)]), m
    back = ec.Run(bc, kind, 5, 17, 17, 2, sizes=RAGGED[::-1])
    assert back.res['marked'] == [] and back.same_bits(whole, range(10), range(9, -1, -1))


# ---------------------------------------------------------------- c. the drivers' shape
@pytest.mark.parametrize('kind', KINDS)
def test_the_drivers_shape(bc, kind):
    """sizes 1 .. 200 in one run (P = 200, R = 20100): seven problems against long double, the bits of three alone"""
    sizes = list(range(1, 201))
    whole = ec.Run(bc, kind, 5, 16, 37, 2, sizes=sizes)
    assert len(whole.sizes) == 200 and int(whole.last['row_ptr'][-1]) == 20100 and whole.res['marked'] == []
    ec.check_last_step(whole, problems=[0, 15, 16, 63, 64, 127, 199])
    for m in (1, 64, 200):
        assert ec.Run(bc, kind, 5, 16, 37, 2, sizes=[m]).same_bits(whole, [0], [m - 1]), m


# ---------------------------------------------------------------- d. the problem count at its limit
def test_the_problem_count_at_its_limit(bc):
    P = ec.header_constants()['BC_PSVI_MANY_MAX_PROBLEMS']
    perm = np.random.RandomState(9).permutation(ec.N_ROWS)
    starts = [perm[p % ec.N_ROWS:p % ec.N_ROWS + 1] for p in range(P)]
    whole = ec.Run(bc, ec.LOGISTIC, 3, 7, 37, 2, starts=starts)
    assert whole.sizes == [1] * P and whole.res['marked'] == []
    ec.check_last_step(whole, problems=[0, P // 2 - 1, P - 1])
    for p in (0, P // 2 - 1, P - 1):
        assert ec.Run(bc, ec.LOGISTIC, 3, 7, 37, 2, starts=[starts[p]]).same_bits(whole, [0], [p]), p


# ---------------------------------------------------------------- e. exact cases, no tolerance
@pytest.mark.parametrize('kind', KINDS)
def test_one_sample_leaves_the_state_where_it_was(bc, kind):
    """S = 1: a row minus its own mean is exactly zero, so target, resid and both gradients are zero (of either sign), both
    moments stay zero and ADAM moves nothing -- after every chunk."""
    d, m, s, n_sub, diag, n_rows = ec.TABLES[kind][0]
    assert s == 1
    r = ec.Run(bc, kind, d, s, n_sub, 3, diag=diag, sizes=[m], n_rows=n_rows, chunk=1)
    assert [done for done, _ in r.seams] == [1, 2, 3] and r.res['marked'] == []
    for done, L in r.seams:
        for k in ('target', 'resid', 'gw', 'gp', 'mom1_w', 'mom1_p', 'mom2_w', 'mom2_p'):
            assert not L[k].any(), (done, k)
        assert np.array_equal(L['w'], r.w0[0]) and np.array_equal(L['pts'], r.pts0[0]), done
        assert np.array_equal(L['w_before'], r.w0[0]) and np.array_equal(L['pts_before'], r.pts0[0]), done
        assert not L['flag'].any()
    assert np.array_equal(r.res['w'][0], r.w0[0]) and np.array_equal(r.res['pts'][0], r.pts0[0])
    last = ec.Run(bc, kind, d, s, n_sub, 3, diag=diag, sizes=[m], n_rows=n_rows)      # (chunks of 2 and 1: the seam before the last step)
    ec.check_last_step(last)                                   # mode (or mean) and draw within their bounds; zero bounds hold the zeros
    assert last.same_bits(r)


@pytest.mark.parametrize('kind', KINDS)
def test_one_coordinate_leaves_the_points_where_they_were(bc, kind):
    """D = 1: the point-gradient is centred over its only coordinate, so g_p is exactly zero and the points never move, while
    the weights do."""
    r = ec.Run(bc, kind, 1, 16, 16, 3, sizes=[1, 17])
    ec.check_last_step(r)
    for done, L in r.seams:
        assert not L['gp'].any() and not L['mom1_p'].any() and not L['mom2_p'].any(), done
    for p in range(2):
        assert np.array_equal(r.res['pts'][p], r.pts0[p])
        assert np.all(r.res['w'][p] != r.w0[p])


# ---------------------------------------------------------------- f. float32 rows of a wave instruction and more
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('d', [64, 128])
def test_wide_float32_rows_give_the_bits_of_their_widened_copy(bc, kind, d):
    """rows of 256 and 512 bytes: k_take_rows moves them with its second lane mapping"""
    narrow = ec.Run(bc, kind, d, 17, 37, 2, sizes=[1, 17, 40], f32=True)
    wide = ec.Run(bc, kind, d, 17, 37, 2, sizes=[1, 17, 40])
    assert narrow.res['marked'] == [] == wide.res['marked'] and narrow.same_bits(wide)
    assert not np.array_equal(wide.res['w'][2], wide.w0[2])    # (the run did move something)
