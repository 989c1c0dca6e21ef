"""tests/laplace_many_harness.cpp -- the four stages of csrc/bc_vi_laplace_dev.h run over a packed batch on the host -- compiled
stand-alone with -fsanitize=address,undefined and run on the smallest and the largest D of tests/test_laplace_many_cpu.py: a
batch with shared and with per-problem normals, the diagonal form, no draws at all, and a batch with refused problems.  It must
end clean.  A stand-alone program: nothing is preloaded and nothing is loaded into Python.  CPU only; nothing here touches a
GPU."""
import numpy as np
import pytest

import laplace_many_cases as lm
import vi_laplace_cases as lc


@pytest.fixture(scope='module')
def sanitized(tmp_path_factory):
    return lm.build_harness(tmp_path_factory.mktemp('laplace_many_san'), extra=['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'])


@pytest.mark.parametrize('d', [1, 128])
def test_sanitized_build_ends_clean(sanitized, tmp_path, d):
    rng = np.random.RandomState(900 + d)
    base = lm.cases_of_dim(d) + [lc.make_case(d, 300, 256, variant=3 + d)]
    E = rng.randn(17, d)
    cases = [lm.with_normals(c, E) for c in base]
    for c, r in zip(cases, lm.run_harness(sanitized, cases, E, tmp_path)):      # (asserts exit status 0 and an empty stderr)
        assert r['status'] == 0
        lc.check_mode_and_draw(c, r['mu'], r['draws'], 'sanitized')
        lm.check_factors(c, r['mu'], r['hdiag'], r['chol'], r['inv'], 'sanitized')
    Ep = rng.randn(len(base), 3, d)
    assert all(r['status'] == 0 for r in lm.run_harness(sanitized, base, Ep, tmp_path))
    assert all(r['status'] == 0 for r in lm.run_harness(sanitized, base, Ep, tmp_path, diag=True))
    none = lm.run_harness(sanitized, base, np.zeros((0, d)), tmp_path)
    assert all(r['status'] == 0 and r['draws'].shape == (0, d) for r in none)
    bad = [dict(c) for c in base]
    bad[1]['w'] = bad[1]['w'].copy()
    bad[1]['w'][3] = np.nan
    bad[-1]['start'] = np.full(d, np.nan)
    outs = lm.run_harness(sanitized, bad, E, tmp_path)
    assert [r['status'] for r in outs] == [0, 1] + [0] * (len(base) - 3) + [1] and outs[1]['untouched'] and outs[-1]['untouched']
