"""tests/psvi_many_harness.cpp -- one full step of the batched BatchPSVI run on the host -- compiled stand-alone with
-fsanitize=address,undefined and run on the smallest and the largest D, a ragged last row tile and more than one, both forms of
the covariance, and the three ways a problem gets marked.  It must end clean.  A stand-alone program: nothing is preloaded and
nothing is loaded into Python.  CPU only; nothing here touches a GPU."""
import numpy as np
import pytest

import psvi_many_cases as pm
import vi_laplace_cases as lc


@pytest.fixture(scope='module')
def sanitized(tmp_path_factory):
    return pm.build_harness(tmp_path_factory.mktemp('psvi_many_san'), extra=['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'])


@pytest.mark.parametrize('d', [1, 128])
def test_sanitized_build_ends_clean(sanitized, tmp_path, d):
    for shape, n_sub, diag in ((0, 1, False), (1, 37, True), (2, 200, False)):
        m, s = lc.SHAPES[shape]
        st = pm.make_step(d, m, s, n_sub, diag=diag, variant=shape + d)
        r = pm.run_step(sanitized, st, tmp_path)             # (asserts exit status 0 and an empty stderr)
        assert r['status'] == 0
        pm.check_stage34('sanitized', st['rows'], st['scale'], st['pts'], st['w'], r['theta'], r['target'], r['resid'], r['gw'])
    st = pm.make_step(d, 7, 5, 37, variant=1 + d)
    bad = dict(st, w=np.full(7, np.nan))
    assert pm.run_step(sanitized, bad, tmp_path)['status'] == 1
    bad = dict(st, rows=np.full_like(st['rows'], np.inf))
    assert pm.run_step(sanitized, bad, tmp_path)['status'] == 2
    bad = dict(st, m2w=np.full(7, -1e300))                # (sqrt of a negative moment: NaN after the step)
    assert pm.run_step(sanitized, bad, tmp_path)['status'] == 3
