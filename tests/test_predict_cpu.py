"""The arithmetic of the linear-regression held-out scorer without a GPU: tests/predict_harness.cpp -- the host build of
csrc/bc_predict_dev.h, walked lane by lane, chunk by chunk and through the combine stage as k_linreg_predict walks it -- against
the long-double restatement of tests/predict_cases.py (sums and per-row outputs within the derived tolerance), the exact cases bit
for bit, batch independence of the sums, the reference's own figures (tests/golden/predict_f24.npz, recorded by
tests/golden/make_golden_predict.py), and the Python layer's argument checks that need no device."""
import os

import numpy as np
import pytest

import predict_cases as pc
from beta_cores_amd import samplers

GOLDEN = os.path.join(pc.ROOT, 'tests', 'golden', 'predict_f24.npz')
pytestmark = pytest.mark.skipif(not pc.LONGDOUBLE_OK, reason='np.longdouble is no wider than float64 on this platform')


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    return pc.build_harness(tmp_path_factory.mktemp('predict'))


def test_the_table_meets_its_conditions():
    pc.check_table()


@pytest.mark.parametrize('name', pc.NAMES)
def test_harness_against_long_double(harness, tmp_path, name):
    c, ref = pc.make_case(name), pc.reference(name)
    got = pc.run_harness(harness, c['Z'], c['mu'], c['F'], c['noise'], c['scale'], tmp_path)
    pc.compare(got['ll'], got['sse'], ref, name, mean=got['mean'], var=got['var'])
    lean = pc.run_harness(harness, c['Z'], c['mu'], c['F'], c['noise'], c['scale'], tmp_path, per_row=False)
    assert np.array_equal(lean['ll'], got['ll']) and np.array_equal(lean['sse'], got['sse'])


def test_exact_zero_factor(harness, tmp_path):
    Z, mu, F, noise, scale = pc.exact_zero_factor()
    got = pc.run_harness(harness, Z, mu, F, noise, scale, tmp_path)
    assert np.array_equal(got['var'], np.repeat(noise[:, None], Z.shape[0], axis=1))


@pytest.mark.parametrize('d', [1, 5, 16, 17, 128, 129, 300])
def test_exact_unit_rows(harness, tmp_path, d):
    Z, mu, F, noise, scale, want_mean, want_var = pc.exact_unit_rows(d)
    got = pc.run_harness(harness, Z, mu, F, noise, scale, tmp_path)
    assert np.array_equal(got['mean'][0], want_mean) and np.array_equal(got['var'][0], want_var)
    if d > 1:
        wrong = pc.run_harness(harness, Z, mu, np.ascontiguousarray(F.transpose(0, 2, 1)), noise, scale, tmp_path)
        assert not np.array_equal(wrong['var'][0], want_var)


def test_exact_single_row(harness, tmp_path):
    Z, mu, F, noise, scale, want_ll = pc.exact_single_row()
    got = pc.run_harness(harness, Z, mu, F, noise, scale, tmp_path)
    assert got['sse'][0] == 0. and got['var'][0, 0] == 1. and got['mean'][0, 0] == Z[0, -1] and got['ll'][0] == want_ll


def test_a_posteriors_sums_do_not_depend_on_its_batch(harness, tmp_path):
    c = pc.make_case('n65_d16_t17')
    full = pc.run_harness(harness, c['Z'], c['mu'], c['F'], c['noise'], c['scale'], tmp_path, per_row=False)
    for t in (0, 1, 9, 16):
        for sel in ([t], [t, 3], [5, 2, t]):
            one = pc.run_harness(harness, c['Z'], c['mu'][sel], c['F'][sel], c['noise'][sel], c['scale'][sel], tmp_path, per_row=False)
            at = sel.index(t)
            assert one['ll'][at] == full['ll'][t] and one['sse'][at] == full['sse'][t], (t, sel)


def test_harness_against_the_reference_fixture(harness, tmp_path):
    g = np.load(GOLDEN)
    Z = np.hstack((g['Xt'], g['yt'][:, None]))
    nt = Z.shape[0]
    host_gap = float(g['host_gap'])
    assert host_gap <= 1e-12
    for i in range(g['theta_mean'].shape[0]):
        F = np.linalg.cholesky(g['theta_cov'][i])
        noise = float(g['sigmasq'][i])
        ref = pc.restate(Z, g['theta_mean'][i], F, noise, 1.)
        got = pc.run_harness(harness, Z, g['theta_mean'][i], F[None], noise, 1., tmp_path)
        pc.compare(got['ll'], got['sse'], ref, 'predict_f24[%d]' % i, mean=got['mean'], var=got['var'])
        # the golden tolerance: the derived bound plus 8 host_gap (|golden| + 1) (a different LAPACK Cholesky on this host)
        assert np.all(np.abs(got['mean'][0] - g['pred_mean'][i]) <= ref['tol_mean'][0] + 8. * host_gap * (np.abs(g['pred_mean'][i]) + 1.))
        assert np.all(np.abs(got['var'][0] - g['pred_var'][i]) <= ref['tol_var'][0] + 8. * host_gap * (np.abs(g['pred_var'][i]) + 1.))
        scores = samplers.PredictiveScores(got['ll'], got['sse'], nt)
        nll_tol = ref['tol_ll'][0] / nt + 8. * host_gap * (abs(float(g['nll'][i])) + 1.)
        assert abs(scores.nll()[0] - float(g['nll'][i])) <= nll_tol
        assert abs(-got['ll'][0] / nt - float(-g['log_density'][i].mean())) <= nll_tol
        rmse = float(g['rmse'][i])
        std = float(g['output_std'])
        # d sqrt(x) = dx / (2 sqrt(x)): the sse tolerance carried through output_std sqrt(sse / Nt), plus the host gap
        rmse_tol = std * ref['tol_sse'][0] / nt / (2. * rmse / std) * 1.01 + 8. * host_gap * (rmse + 1.)
        assert abs(scores.rmse(std)[0] - rmse) <= rmse_tol


def test_harness_refuses_shapes_outside_the_limits(harness, tmp_path):
    pc.run_harness(harness, np.zeros((1, pc.MAX_DIM + 2)), np.zeros((1, pc.MAX_DIM + 1)), np.zeros((1, pc.MAX_DIM + 1, pc.MAX_DIM + 1)), 1., 1., tmp_path,
                   expect=2)


def test_python_checks_need_no_device():
    with pytest.raises(ValueError, match='Nt x \\(D \\+ 1\\)'):
        samplers.RegressionHeldOut(np.zeros((3, 1)))
    with pytest.raises(ValueError, match='1 .. 512 features'):
        samplers.RegressionHeldOut(np.zeros((3, 514)))
    with pytest.raises(TypeError, match='RegressionHeldOut'):
        samplers.linreg_predictive(np.zeros((3, 3)), np.zeros(2), np.eye(2), 1.)
    s = samplers.PredictiveScores(np.array([-8., -2.]), np.array([16., 4.]), 4)
    assert np.array_equal(s.nll(), [2., 0.5]) and np.array_equal(s.rmse(3.), [6., 3.]) and s.mean is None and s.var is None
