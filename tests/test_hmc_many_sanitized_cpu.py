"""tests/hmc_small_harness.cpp -- the host build of csrc/bc_hmc_small_dev.h + csrc/bc_hmc_dev.h -- compiled stand-alone with
-fsanitize=address,undefined and run on the batch cases of tests/hmc_many_cases.py, the limits (1 x 1 x 1, one row at D = 256,
64 chains), the everything-rejected run and the non-finite start: it must end clean.  CPU only; nothing here touches a GPU,
nothing is loaded into Python."""
import numpy as np
import pytest

import hmc_cases as hc
import hmc_many_cases as mc


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    return mc.build_harness(tmp_path_factory.mktemp('hmc_small_san'), extra=['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'])


@pytest.mark.parametrize('name', mc.BATCH_NAMES)
def test_sanitized_batch_ends_clean(harness, tmp_path, name):
    case = mc.make_batch_case(name)
    got = mc.run_harness(harness, case['problems'], tmp_path)      # (asserts exit status 0 and an empty stderr)
    acc = np.concatenate([g['accept'].ravel() for g in got])
    assert all(g['status'] == 0 for g in got) and acc.any() and not acc.all()
    assert all(np.all(np.isfinite(g['samples'])) for g in got)


@pytest.mark.parametrize('ns,d,c', [((1,), 1, 1), ((1, 3), 256, 2), ((9, 64, 129), 3, 64)])
def test_sanitized_limits_end_clean(harness, tmp_path, ns, d, c):
    rng = np.random.RandomState(8)
    E, logU = rng.randn(2, c, d), np.log(rng.rand(2, c))
    probs = []
    for p, n in enumerate(ns):
        Z, w = hc.make_data(n, d, 7 + p)
        probs.append(dict(Z=Z, w=w, start=rng.randn(c, d) * 0.1, inv_mass=0.5 + rng.rand(d), eps=0.05, L=3, E=E, logU=logU))
    got = mc.run_harness(harness, probs, tmp_path)
    assert all(g['status'] == 0 and g['samples'].shape == (2, c, d) and np.all(np.isfinite(g['logjoint'])) for g in got)
    for pr in probs:
        pr['eps'] = 1e6
    got = mc.run_harness(harness, probs, tmp_path)
    assert all(g['status'] == 0 and not g['accept'].any() for g in got)
    probs[-1]['start'][0, 0] = np.inf
    got = mc.run_harness(harness, probs, tmp_path)
    assert [g['status'] for g in got] == [0] * (len(ns) - 1) + [1]
