"""The batched BatchPSVI run at the edges of its tiles and at its limits, without a GPU (tests/psvi_many_edge_cases.py): the two
tables of shapes hold what they must, and every row of both, as one step from the run's initial state through the matching host
harness (tests/psvi_many_harness.cpp, tests/psvi_many_gauss_harness.cpp), stays inside the bounds of tests/psvi_many_cases.py and
tests/psvi_many_gauss_cases.py with ADAM bit for bit.  This pins that the long-double references and their bounds take these
shapes as they are; the device's own branches (matrix cores, cross-lane sums, strided loops) run in
tests/test_gpu_psvi_many_edges.py.

Worst error / bound over the rows, as measured on the host: 0.071 for the logistic kind (the draw at D = 1 with m = 4096; 0.0041,
g_p, without the draw), 0.058 for the Gaussian kind (mean and draw at D = 1; 0.0035, the target, without them); per stage in
profiles/psvi_many_notes.md and profiles/psvi_many_gauss_notes.md."""
import numpy as np
import pytest

import psvi_many_cases as pm
import psvi_many_edge_cases as ec
import psvi_many_gauss_cases as pg


@pytest.fixture(scope='module')
def harnesses(tmp_path_factory):
    return {ec.LOGISTIC: pm.build_harness(tmp_path_factory.mktemp('psvi_many_edges')),
            ec.GAUSS: pg.build_harness(tmp_path_factory.mktemp('psvi_many_gauss_edges'))}


def test_the_tables_hold_every_edge():
    ec.check_tables()


def _one_step(kind, row, harnesses, tmp_path):
    st = ec.first_step(kind, row)
    r = (pm if kind == ec.LOGISTIC else pg).run_step(harnesses[kind], st, tmp_path)
    worst = ec.check_host_step(kind, '%s %s' % (kind, ec.row_id(row)), st, r)
    ec.print_worst('host %s %s' % (kind, ec.row_id(row)), worst)
    d, m, s = row[:3]
    if s == 1:          # a row minus its own mean: the step is exactly empty (either sign of zero)
        assert not r['target'].any() and not r['resid'].any() and not r['gw'].any() and not r['gp'].any()
        assert np.array_equal(r['w'], st['w']) and np.array_equal(r['pts'], st['pts'])
        assert not any(r[k].any() for k in ('m1w', 'm1p', 'm2w', 'm2p'))
    if d == 1:          # the point-gradient is centred over its one coordinate
        assert not r['gp'].any() and np.array_equal(r['pts'], st['pts'])
    if d == 1 and s > 1:
        assert not np.array_equal(r['w'], st['w'])
    return worst


@pytest.mark.parametrize('row', ec.LOGISTIC_TABLE, ids=ec.row_id)
def test_logistic_row_as_one_host_step(harnesses, tmp_path, row):
    _one_step(ec.LOGISTIC, row, harnesses, tmp_path)


@pytest.mark.parametrize('row', ec.GAUSS_TABLE, ids=ec.row_id)
def test_gaussian_row_as_one_host_step(harnesses, tmp_path, row):
    _one_step(ec.GAUSS, row, harnesses, tmp_path)
