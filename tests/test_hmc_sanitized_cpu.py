"""tests/hmc_harness.cpp -- the host build of csrc/bc_hmc_dev.h -- compiled stand-alone with -fsanitize=address,undefined and
run on the trace cases of tests/hmc_cases.py, the limits of the chain count and the dimension, the everything-rejected run and
the non-finite start: it must end clean.  CPU only; nothing here touches a GPU, nothing is loaded into Python."""
import numpy as np
import pytest

import hmc_cases as hc


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    return hc.build_harness(tmp_path_factory.mktemp('hmc_san'), extra=['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'])


@pytest.mark.parametrize('name', ['small', 'wide'])
def test_sanitized_trace_ends_clean(harness, tmp_path, name):
    case = hc.make_trace_case(name)
    got = hc.run_harness(harness, case, tmp_path)      # (asserts exit status 0 and an empty stderr)
    assert got['status'] == 0 and got['accept'].any() and not got['accept'].all() and np.all(np.isfinite(got['samples']))


@pytest.mark.parametrize('n,d,c', [(1, 1, 1), (17, 256, 2), (9, 3, 64)])
def test_sanitized_limits_end_clean(harness, tmp_path, n, d, c):
    Z, w = hc.make_data(n, d, 7)
    rng = np.random.RandomState(8)
    case = dict(Z=Z, w=w, start=rng.randn(c, d) * 0.1, inv_mass=0.5 + rng.rand(d), eps=0.05, L=3, E=rng.randn(2, c, d),
                logU=np.log(rng.rand(2, c)))
    got = hc.run_harness(harness, case, tmp_path)
    assert got['status'] == 0 and got['samples'].shape == (2, c, d) and np.all(np.isfinite(got['logjoint']))
    case['eps'] = 1e6
    got = hc.run_harness(harness, case, tmp_path)
    assert got['status'] == 0 and not got['accept'].any()
    case['start'][0, 0] = np.inf
    assert hc.run_harness(harness, case, tmp_path)['status'] == 1
