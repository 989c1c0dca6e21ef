"""tests/diag_harness.cpp -- the host build of beta_cores_amd/csrc/bc_diag_dev.h, the chain summary's own block functions with one
thread -- against the long-double restatement of tests/diag_cases.py, within the derived bounds, on the shapes and planted
coordinates the device tests use; ESS and R-hat as functions of the rho and moments that build returns.  CPU only."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import diag_cases as DC                                                          # noqa: E402

pytestmark = pytest.mark.skipif(not DC.LONGDOUBLE_OK, reason=DC.LONGDOUBLE_WHY)


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    return DC.build_harness(tmp_path_factory.mktemp('diag_harness'))


def _check(exe, tmp, p, n, c, d, max_lag, staged):
    x = DC.make_problem(p, n, c, d)
    got = DC.run_harness(exe, x, max_lag, tmp, staged=staged)
    what = 'host build %dx%dx%d problem %d max_lag %r %s' % (n, c, d, p, max_lag, 'staged' if staged else 'in place')
    assert got['status'] == 0
    DC.check_against_reference(got, x, max_lag, what)
    DC.check_own(got, n, c, what)
    for j, kind in DC.planted_kinds(p, d).items():
        if kind == 'const':
            assert np.isnan(got['rhat'][j]) and np.isnan(got['ess'][j]) and not got['cov'][j].any() and not got['cov'][:, j].any()
            assert got['mean'][j] == x[0, 0, j]
    assert np.array_equal(got['cov'], got['cov'].T)
    return got


@pytest.mark.parametrize('shape', DC.SHAPES, ids=lambda s: 'x'.join(str(k) for k in s))
def test_host_build_follows_the_restatement(harness, tmp_path, shape):
    P, n, c, d = shape
    for p in range(P):
        a = _check(harness, tmp_path, p, n, c, d, None, True)
        if p == 0:                                             # the sequences read where they lie: the same bits as the staged ones
            b = _check(harness, tmp_path, p, n, c, d, None, False)
            for k in ('mean', 'cov', 'W', 'varplus', 'rhat', 'ess', 'rho', 'truncated'):
                assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_host_build_clips_max_lag(harness, tmp_path):
    for lag in (1, 2, 31, 40):
        got = _check(harness, tmp_path, 0, 64, 4, 9, lag, True)
        assert got['rho'].shape[0] == min(lag, 31) + 1
