"""tests/psvi_many_gauss_harness.cpp -- one full step of the Gaussian-location kind of the batched BatchPSVI run on the host --
compiled stand-alone with -fsanitize=address,undefined and run on the smallest and the largest D with ragged tiles of rows and of
points, and on the three ways a problem gets marked.  It must end clean.  A stand-alone program with its own main: nothing is
preloaded and nothing is loaded into Python.  CPU only; nothing here touches a GPU."""
import numpy as np
import pytest

import psvi_many_gauss_cases as pg


@pytest.fixture(scope='module')
def sanitized(tmp_path_factory):
    return pg.build_harness(tmp_path_factory.mktemp('psvi_many_gauss_san'), extra=['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'])


@pytest.mark.parametrize('d,m,s,n_sub', [(3, 1, 7, 37), (128, 17, 100, 64)])
def test_sanitized_build_ends_clean(sanitized, tmp_path, d, m, s, n_sub):
    st = pg.make_step(d, m, s, n_sub)
    r = pg.run_step(sanitized, st, tmp_path)                 # (asserts exit status 0 and an empty stderr)
    assert r['status'] == 0
    pg.check_stage34('sanitized', st['rows'], st['scale'], st['pts'], st['w'], r['theta'], st, r['target'], r['resid'], r['gw'])
    bad = dict(st, w=np.full(m, np.nan))
    assert pg.run_step(sanitized, bad, tmp_path)['status'] == 1
    bad = dict(st, rows=np.full_like(st['rows'], np.inf))
    assert pg.run_step(sanitized, bad, tmp_path)['status'] == 2
    bad = dict(st, m2w=np.full(m, -1e300))                   # (sqrt of a negative moment: NaN after the step)
    assert pg.run_step(sanitized, bad, tmp_path)['status'] == 3
