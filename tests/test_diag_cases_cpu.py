"""The cases of tests/diag_cases.py held on the CPU, before tests/test_gpu_diag.py runs them on the device.  Conditions, not
measurements: NumPy's float64 evaluation of the formulas lies inside every derived bound, no bound exceeds 1e-9 of its quantity's
scale (so that none is vacuous), every planted coordinate is what its kind says in the long-double restatement, and the
restatement itself behaves like an ESS and an R-hat on chains whose answer is known."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import diag_cases as DC                                                          # noqa: E402

pytestmark = pytest.mark.skipif(not DC.LONGDOUBLE_OK, reason=DC.LONGDOUBLE_WHY)
CAP = 1e-9


@pytest.mark.parametrize('shape', DC.SHAPES, ids=lambda s: 'x'.join(str(k) for k in s))
def test_float64_numpy_lies_inside_bounds_that_are_not_vacuous(shape):
    P, n, c, d = shape
    seen = set()
    for p in range(P):
        x = DC.make_problem(p, n, c, d)
        ref, f64, b = DC.summary(x), DC.summary(x, dtype=np.float64), DC.bounds(x)
        sc = DC.scales(ref)
        for k in ('mean', 'cov', 'W', 'varplus', 'rho'):
            what = '%r problem %d %s' % (shape, p, k)
            assert DC.inside(f64[k], ref[k], b[k]), '%s: float64 NumPy is %.3g bounds from the reference' % (what, DC.worst(f64[k], ref[k], b[k]))
            live = ~np.isnan(np.asarray(ref[k])) & (np.asarray(sc[k]) > 0)
            assert np.all(np.asarray(b[k])[live] <= CAP * np.asarray(sc[k])[live]), \
                '%s: bound %.3g of the scale' % (what, float((np.asarray(b[k])[live] / np.asarray(sc[k])[live]).max()))
            dead = ~np.isnan(np.asarray(ref[k])) & (np.asarray(sc[k]) == 0)
            assert np.all(np.asarray(b[k])[dead] == 0), what
        for j, kind in DC.planted_kinds(p, d).items():
            seen.add((kind, j % 16))
            if kind == 'const':
                assert np.isnan(ref['rhat'][j]) and np.isnan(ref['ess'][j]) and not ref['cov'][j].any() and not ref['cov'][:, j].any()
                assert ref['mean'][j] == DC.LD(x[0, 0, j])
            elif kind == 'big':
                assert abs(ref['mean'][j] - 1e8) < 1. and 0.3 < ref['cov'][j, j] < 3.
            elif kind == 'anti':
                assert ref['K'][j] == 0 and np.isnan(ref['ess'][j]) and ref['truncated'][j] == 0
            elif kind == 'ar9' and n == 64:
                assert ref['truncated'][j] == 1 and ref['K'][j] == (ref['L'] + 1) // 2 and np.isfinite(ref['ess'][j])
            elif kind == 'shift' and 2 <= c <= 16:
                # (one of C chains 5 sd away: Bh is about 25 (C - 1) / C^2 and rhat^2 about 1 + Bh, above 2.25 up to C = 17; among
                # 64 chains one stray chain moves rhat to 1.13 only, by the definition)
                assert ref['rhat'][j] > 1.5
            elif kind == 'shift' and c > 16:
                assert 1.05 < ref['rhat'][j] < 1.5
    if d >= 128:
        assert seen == {(k, s) for k in DC.KINDS for s in (0, 7, 15)}     # every kind in the first, a middle and the last place of a tile
    if shape == (5, 64, 16, 9):
        assert any(k == 'ar9' for p in range(P) for k in DC.planted_kinds(p, d).values())


def test_the_restatement_on_chains_whose_answer_is_known():
    rng = np.random.RandomState(5)
    n, c = 1000, 16
    ar = DC._ar1(rng, n, c, 0.5)[:, :, None]
    r = DC.summary(ar)
    ratio = float(r['ess'][0]) / (n * c)
    assert abs(ratio / (1. / 3.) - 1.) < 0.25, ratio
    iid = rng.randn(n, c, 1)
    r = DC.summary(iid)
    assert abs(float(r['rhat'][0]) - 1.) < 0.01 and 0.8 < float(r['ess'][0]) / (n * c) < 1.2
    small = DC.summary(rng.randn(4, 1, 1))
    assert np.isfinite(small['rhat'][0]) and small['L'] == 1
    const = DC.summary(np.full((8, 2, 1), 0.3))
    assert np.isnan(const['rhat'][0]) and np.isnan(const['ess'][0])


def test_max_lag_clips_and_flags():
    x = DC.make_problem(0, 64, 4, 3, plant=False)
    h = 32
    for lag, L in ((1, 1), (2, 2), (h - 1, h - 1), (h + 5, h - 1), (None, h - 1)):
        r = DC.summary(x, lag)
        assert r['L'] == L and r['rho'].shape[0] == L + 1
        assert np.all((r['K'] == (L + 1) // 2) == (r['truncated'] == 1))
    assert np.all(DC.summary(x, 1)['truncated'] == 1) and np.all(DC.summary(x, 1)['K'] == 1)      # (P_0 = 1 + rho_1 > 0 on these chains)


def test_ess_from_rho_follows_the_rule_on_a_handmade_sequence():
    rho = np.array([1., 0.5, 0.2, 0.4, 0.1, 0.05, -0.3, 0.1, 0.9])          # pairs: 1.5, 0.6, 0.15, -0.2 | L = 8: rho_8 is never used
    ess, full, K, tau, tot = DC.ess_from_rho(rho, 100)
    assert K == 3 and full == 0 and abs(float(tau) - (-1 + 2 * (1.5 + 0.6 + 0.15))) < 1e-15 and abs(float(ess) - 100 / float(tau)) < 1e-12
    rho = np.array([1., 0.5, 0.2, 0.6, np.nan, np.nan])                      # monotone: min(0.8, 1.5) = 0.8; a NaN pair ends the sum
    ess, full, K, tau, tot = DC.ess_from_rho(rho, 10)
    assert K == 2 and full == 0 and abs(float(tau) - (-1 + 2 * (1.5 + 0.8))) < 1e-15
    assert DC.ess_from_rho(np.array([1., 0.5]), 10)[1:3] == (1, 1)
    assert np.isnan(DC.ess_from_rho(np.array([1., -1.2, 0.3]), 10)[0])
