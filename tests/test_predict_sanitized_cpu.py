"""tests/predict_harness.cpp -- the host build of csrc/bc_predict_dev.h -- compiled stand-alone with -fsanitize=address,undefined
and run as its own program on the case table of tests/predict_cases.py and the limits (one row, D = 1 and D = 512, rows on both
sides of a block): it must end clean.  CPU only; nothing here touches a GPU, nothing is loaded into Python."""
import numpy as np
import pytest

import predict_cases as pc


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    return pc.build_harness(tmp_path_factory.mktemp('predict_san'), extra=['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'])


@pytest.mark.parametrize('name', pc.NAMES)
def test_sanitized_case_ends_clean(harness, tmp_path, name):
    c = pc.make_case(name)
    got = pc.run_harness(harness, c['Z'], c['mu'], c['F'], c['noise'], c['scale'], tmp_path)      # (asserts exit status 0, empty stderr)
    assert np.all(np.isfinite(got['ll'])) and np.all(got['sse'] >= 0) and np.all(got['var'] > 0)


@pytest.mark.parametrize('nt,d,t', [(1, 1, 1), (1, 512, 1), (pc.R + 1, 1, 2), (33, 511, 1), (2 * pc.R, 129, 1)])
def test_sanitized_limits_end_clean(harness, tmp_path, nt, d, t):
    rng = np.random.RandomState(5)
    Z, mu, F = rng.randn(nt, d + 1), rng.randn(t, d), rng.randn(t, d, d)
    got = pc.run_harness(harness, Z, mu, F, 0.5, 1., tmp_path)
    assert got['ll'].shape == (t,) and np.all(np.isfinite(got['ll']))
    bad = Z.copy()
    bad[0, 0] = np.inf                                           # a non-finite feature: non-finite sums, no trap, no bad index
    got = pc.run_harness(harness, bad, mu, F, 0.5, 1., tmp_path)
    assert not np.any(np.isfinite(got['ll']))
    pc.run_harness(harness, np.zeros((1, 514)), np.zeros((1, 513)), np.zeros((1, 513, 513)), 1., 1., tmp_path, expect=2)
