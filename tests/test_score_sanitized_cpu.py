"""tests/score_harness.cpp -- the host build of csrc/bc_score_dev.h -- compiled stand-alone with -fsanitize=address,undefined and
run on the case table of tests/score_cases.py and the limits (one row, one theta, D = 1 and D = 256, T past a block's 128): it
must end clean.  CPU only; nothing here touches a GPU, nothing is loaded into Python."""
import numpy as np
import pytest

import score_cases as sc


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    return sc.build_harness(tmp_path_factory.mktemp('score_san'), extra=['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'])


@pytest.mark.parametrize('name', sc.NAMES)
def test_sanitized_case_ends_clean(harness, tmp_path, name):
    c = sc.make_case(name)
    cor, ll = sc.run_harness(harness, c['X'], c['Y'], c['thetas'], tmp_path)      # (asserts exit status 0 and an empty stderr)
    assert np.all(np.isfinite(ll)) and np.all((cor >= 0) & (cor <= c['X'].shape[0]))


@pytest.mark.parametrize('nt,d,t', [(1, 1, 1), (1, 256, 1), (17, 256, 2), (1, 1, 129), (33, 255, 3)])
def test_sanitized_limits_end_clean(harness, tmp_path, nt, d, t):
    rng = np.random.RandomState(5)
    X, Y, th = rng.randn(nt, d), np.where(rng.rand(nt) < 0.5, 1., -1.), rng.randn(t, d) * 1e3
    cor, ll = sc.run_harness(harness, X, Y, th, tmp_path)
    assert cor.shape == (t,) and np.all(np.isfinite(ll))
    sc.run_harness(harness, X, Y, th * np.inf, tmp_path)                            # non-finite margins: no trap, no bad index
    sc.run_harness(harness, np.zeros((1, 257)), np.ones(1), np.zeros((1, 257)), tmp_path, expect=2)
