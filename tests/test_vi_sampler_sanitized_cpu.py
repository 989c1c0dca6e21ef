"""tests/vi_sampler_harness.cpp -- the host build of csrc/bc_vi_sampler_dev.h -- compiled stand-alone with
-fsanitize=address,undefined and run on the largest and the smallest shapes of tests/test_vi_sampler_cpu.py, both kinds, the
not-positive-definite exit and the ADAM body: it must end clean.  CPU only; nothing here touches a GPU."""
import numpy as np
import pytest

import vi_sampler_cases as vc
from beta_cores_amd.util.opt import adam_step_arrays


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    return vc.build_harness(tmp_path_factory.mktemp('vi_sampler_san'), extra=['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'])


@pytest.mark.parametrize('kind', [vc.LINREG, vc.GAUSS])
@pytest.mark.parametrize('d,m,s', [(1, 1, 1), (3, 7, 5), (33, 130, 5), (128, 130, 100)])
def test_sanitized_draw_ends_clean(harness, tmp_path, kind, d, m, s):
    c = vc.make_case(kind, d, m, s)
    status, theta, pad, _, _ = vc.run_sampler(harness, c, tmp_path)      # (asserts exit status 0 and an empty stderr)
    assert status == 0 and np.all(pad == 7.0) and np.all(np.isfinite(theta))
    bad = vc.make_case(kind, d, m, s, sig0_sign=-1.)
    bad['w'] = bad['w'] * 0.
    assert vc.run_sampler(harness, bad, tmp_path)[0] == 1


@pytest.mark.parametrize('kind', [vc.LINREG, vc.GAUSS])
def test_sanitized_general_prior_draw_ends_clean(harness, tmp_path, kind):
    """A dense Sig0inv and th0 != 0 (bc_vi_prior_rhs runs in the harness), scaled weights, nearly collinear columns."""
    c = vc.make_general_case(kind, 33, 130, 5, variant=4)
    status, theta, pad, _, raw = vc.run_sampler(harness, c, tmp_path)
    ref, kappa = vc.high_precision_reference(c)
    assert status == 0 and np.all(pad == 7.0)
    assert np.abs((theta if kind == vc.LINREG else raw) - ref).max() <= vc.draw_bound(33, kappa, ref)


def test_sanitized_adam_ends_clean(harness, tmp_path):
    rng = np.random.RandomState(2)
    out = vc.run_adam(harness, rng.rand(9) + .1, rng.randn(9), rng.rand(9), adam_step_arrays(12, lambda i: 1. / (1. + i)), tmp_path)
    assert out.shape == (12, 9) and np.all(out >= 0.)
