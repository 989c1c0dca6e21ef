"""The arithmetic of the held-out scorer without a GPU: tests/score_harness.cpp -- the host build of csrc/bc_score_dev.h, walked
lane by lane as k_lr_score walks it -- against the long-double restatement of tests/score_cases.py (counts equal, ll within the
derived tolerance), against the reference's own compute_accuracy and log_likelihood sums (tests/golden/score_f20.npz, recorded
by tests/golden/make_golden_score.py), and the Python layer's argument checks that need no device."""
import os

import numpy as np
import pytest

import score_cases as sc
from beta_cores_amd import samplers

GOLDEN = os.path.join(sc.ROOT, 'tests', 'golden', 'score_f20.npz')
pytestmark = pytest.mark.skipif(not sc.LONGDOUBLE_OK, reason='np.longdouble is no wider than float64 on this platform')


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    return sc.build_harness(tmp_path_factory.mktemp('score'))


def test_the_table_meets_its_conditions():
    sc.check_table()
    for n in sc.NAMES:
        c = sc.make_case(n)
        if c['X'].shape[0] >= 3:
            assert not c['X'][:2].any() and c['Y'][0] == 1. and c['Y'][1] == -1.


@pytest.mark.parametrize('name', sc.NAMES)
def test_harness_against_long_double(harness, tmp_path, name):
    c, ref = sc.make_case(name), sc.reference(name)
    sc.check_condition(ref)
    cor, ll = sc.run_harness(harness, c['X'], c['Y'], c['thetas'], tmp_path)
    sc.compare(cor, ll, ref, name)


def test_tie_rule_and_extremes(harness, tmp_path):
    """One row, one column: s = y x theta.  Zeros of either sign are ties (predicted +1); beyond +-100 and +-745 the sign decides."""
    rows = []
    for x in (0., -0., 1e-300, 1., 101., 746., 1e300):
        for y in (1., -1.):
            for th in (1., -1.):
                rows.append((x, y, th))
    for x, y, th in rows:
        cor, ll = sc.run_harness(harness, np.array([[x]]), np.array([y]), np.array([[th]]), tmp_path)
        s = y * x * th
        want = 1 if (y > 0 and s >= 0) or (y < 0 and s > 0) else 0
        assert cor[0] == want, (x, y, th)
        m = np.longdouble(-s)
        exact = -(max(m, 0) + np.log1p(np.exp(-abs(m))))
        assert abs(np.longdouble(ll[0]) - exact) <= 8 * sc.U * abs(exact) + 3.8e-44, (x, y, th)


def test_harness_against_the_reference_fixture(harness, tmp_path):
    g = np.load(GOLDEN)
    Xt, Yt, th = g['Xt'], g['Yt'], g['thetas']
    ref = sc.restate(Xt, Yt, th)
    sc.check_condition(ref)
    cor, ll = sc.run_harness(harness, Xt, Yt, th, tmp_path)
    nt = Xt.shape[0]
    # the reference's accuracies are means of 0 / 1 over Nt (and T Nt) entries: the counts are recovered exactly
    assert np.array_equal(cor, np.rint(g['accuracy_each'] * nt).astype(np.int64))
    assert abs(cor.sum() / (th.shape[0] * nt) - float(g['accuracy'])) <= 1e-15
    # the reference's sums are float64 NumPy: they carry the same count of roundings, so twice the tolerance separates the two
    assert np.all(np.abs(ll - g['ll_sum']) <= 2. * ref['tol'])
    sc.compare(cor, ll, ref, 'score_f20')


def test_harness_refuses_shapes_outside_the_limits(harness, tmp_path):
    sc.run_harness(harness, np.zeros((1, 257)), np.ones(1), np.zeros((1, 257)), tmp_path, expect=2)
    sc.run_harness(harness, np.zeros((1, 3)), np.ones(1), np.zeros((0, 3)), tmp_path, expect=2)


def test_heldout_checks_need_no_device():
    with pytest.raises(ValueError, match='-1 and \\+1'):
        samplers.HeldOut(np.zeros((3, 2)), [1., 0., -1.])
    with pytest.raises(ValueError, match='one label per row'):
        samplers.HeldOut(np.zeros((3, 2)), [1., -1.])
    with pytest.raises(ValueError, match='float32 Xt'):
        samplers.HeldOut(np.zeros((3, 2)), [1., -1., 1.], dtype=np.float32)
    with pytest.raises(ValueError, match='columns'):
        samplers.HeldOut(np.zeros((3, 257)), [1., -1., 1.])
    with pytest.raises(ValueError, match='keep_samples=False needs score'):
        samplers.logistic_hmc_many([(np.zeros((1, 2)), None)], keep_samples=False)
    assert samplers.HMCResult.correct is None and samplers.HMCResult.test_ll is None and samplers.HMCResult.accuracy is None
