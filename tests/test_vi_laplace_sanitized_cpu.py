"""tests/vi_laplace_harness.cpp -- the host build of csrc/bc_vi_laplace_dev.h -- compiled stand-alone with
-fsanitize=address,undefined and run on the smallest and the largest D of tests/test_vi_laplace_cpu.py: every shape, the diagonal
form, a far start and the failure exit.  It must end clean.  CPU only; nothing here touches a GPU."""
import numpy as np
import pytest

import vi_laplace_cases as lc


@pytest.fixture(scope='module')
def sanitized(tmp_path_factory):
    return lc.build_harness(tmp_path_factory.mktemp('vi_laplace_san'), extra=['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'])


@pytest.mark.parametrize('d', [lc.DIMS[0], lc.DIMS[-1]])
def test_sanitized_build_ends_clean(sanitized, tmp_path, d):
    for i, (m, s) in enumerate(lc.SHAPES):
        c = lc.make_case(d, m, s, variant=i + d)
        r = lc.run_laplace(sanitized, c, tmp_path)      # (asserts exit status 0 and an empty stderr)
        assert r['status'] == 0 and np.all(r['pad'] == 7.0)
        lc.check_mode_and_draw(c, r['mode'], r['theta'], 'sanitized')
    c = lc.make_case(d, 7, 5, diag=True)
    assert lc.run_laplace(sanitized, c, tmp_path)['status'] == 0
    c['start'] = 50. * np.ones(d)
    assert lc.run_laplace(sanitized, c, tmp_path)['status'] == 0
    c['w'] = c['w'].copy()
    c['w'][3] = np.nan
    r = lc.run_laplace(sanitized, c, tmp_path)
    assert r['status'] == 1 and r['untouched']
