"""tests/psvi_grad_harness.cpp -- the host build of csrc/bc_psvi_dev.h -- compiled stand-alone with
-fsanitize=address,undefined and run on the three smallest shapes, one odd one and the two largest of tests/test_psvi_grad_cpu.py, all three
models: it must end clean (every input and the work space live in allocations of exactly their size).  CPU only; nothing here
touches a GPU."""
import numpy as np
import pytest

import psvi_cases as pc


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    return pc.build_harness(tmp_path_factory.mktemp('psvi_grad_san'), extra=['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'])


@pytest.mark.parametrize('kind,sigsq', pc.MODELS)
@pytest.mark.parametrize('m,s,d', [(1, 1, 1), (1, 1, 2), (1, 1, 3), (7, 5, 3), (130, 100, 300), (40, 256, 300)])
def test_sanitized_point_gradient_ends_clean(harness, tmp_path, kind, sigsq, m, s, d):
    c = pc.make_case(kind, m, s, d, sigsq)
    got = pc.run_harness(harness, c, tmp_path)      # (asserts exit status 0 and an empty stderr)
    ref, bound = pc.reference(c)
    assert np.all(np.isfinite(got)) and np.all(np.abs(got - ref) <= bound)
