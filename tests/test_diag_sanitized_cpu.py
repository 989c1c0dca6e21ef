"""tests/diag_harness.cpp -- the chain summary's block functions (beta_cores_amd/csrc/bc_diag_dev.h) on the host -- compiled
stand-alone with -fsanitize=address,undefined and run on the smallest shape, an odd one and the chain limit, with the sequences
staged and read in place, within the same bounds as the plain build, and on a sample that is not finite.  It must end clean.  A
stand-alone program with its own main: nothing is preloaded and nothing is loaded into Python.  CPU only."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import diag_cases as DC                                                          # noqa: E402
import test_diag_harness_cpu as H                                                # noqa: E402

pytestmark = pytest.mark.skipif(not DC.LONGDOUBLE_OK, reason=DC.LONGDOUBLE_WHY)


@pytest.fixture(scope='module')
def sanitized(tmp_path_factory):
    return DC.build_harness(tmp_path_factory.mktemp('diag_san'), extra=['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'])


@pytest.mark.parametrize('n,c,d', [(4, 1, 1), (37, 3, 17), (12, 64, 33)])
def test_sanitized_build_ends_clean(sanitized, tmp_path, n, c, d):
    for staged in (True, False):
        H._check(sanitized, tmp_path, 1, n, c, d, None, staged)  # (run_harness asserts exit status 0 and an empty stderr)
    x = DC.make_problem(0, n, c, d)
    x[n // 2, c - 1, d - 1] = np.nan
    assert DC.run_harness(sanitized, x, None, tmp_path)['status'] == 1
