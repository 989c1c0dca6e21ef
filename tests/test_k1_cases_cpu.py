"""The bound of K1's element-wise GPU tests (tests/k1_cases.py), on the CPU: it is not too tight -- the float64 oracle
(oracle/models_ref.py, likelihoods.*.beta_gradient_host, NumPy's centring), as it is and with the contraction summed in reversed
order, lies inside it on every listed case -- and not blind: six wrong projections each leave it; the lists reach what they
say; and, in numbers, what the bar the suite began with (1e-11 * (1 + max|f| over the matrix)) would have let through."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import k1_cases as K                                                             # noqa: E402


def need_longdouble():
    if not K.LONGDOUBLE_OK:
        pytest.skip(K.LONGDOUBLE_WHY)


def centred(raw):
    return raw - raw.mean(axis=1)[:, None]


def results(phi):
    """(Phi, norms, column sums) as NumPy forms them from a float64 Phi"""
    return phi, np.sqrt((phi ** 2).sum(axis=1)), phi.sum(axis=0)


def reversed_inputs(family, inp):
    """the same case with the features in reversed order: the same sums, added up from the other end"""
    out = dict(inp)
    Z = inp['Z']
    d = inp['th'].shape[1]
    out['Z'] = np.ascontiguousarray(np.hstack((Z[:, :d][:, ::-1], Z[:, d:])))
    out['th'] = np.ascontiguousarray(inp['th'][:, ::-1])
    if family == 'gauss':
        out['Siginv'] = np.ascontiguousarray(inp['Siginv'][::-1, ::-1])
    return out


# ------------------------------------------------------------------ the lists
def test_lists_reach_every_instance_and_edge():
    S_all = set(c[3] for c in K.STAGED)
    assert S_all == {1, 16, 64, 97, 100, 65, 101, 112, 113, 208, 209, 256, 257, 300, 513}
    assert set(c[1] for c in K.STAGED) == {1, 15, 16, 17, 127, 128, 129, 300}
    small_kc = set(c[2] for c in K.STAGED if K.instance(c[3])[3] == 32)
    big_kc = set(c[2] for c in K.STAGED if K.instance(c[3])[3] == 16)
    assert {1, 31, 32, 33} <= small_kc and {15, 16, 17} <= big_kc and max(small_kc | big_kc) > 128
    for fam in K.FAMILIES:
        mine = [c for c in K.STAGED if c[0] == fam]
        assert set(K.instance(c[3])[0] for c in mine) == {'4', '6+4', '7', '13', '16', 'RAW'}, fam
        assert any(96 < c[3] <= 100 and c[1] % 16 != 0 for c in mine), fam        # a ragged n in the S = 97 .. 100 path
        assert set(c[4] for c in mine) == set(K.KINDS)
    assert len(set(K.STAGED)) == len(K.STAGED)
    assert sorted(sum(K.IDS.values(), ())) == list(range(9))
    assert set(K.RESIDENT) == set((d, S) for d in (13, 37) for S in (16, 100, 112))
    assert [K.instance(S)[0] for S in (16, 100, 112)] == ['4', '6+4', '7']
    for b in (K.RESIDENT_BETA,) + tuple(K.BETA.values()):
        assert b in K.PT_BODY_ERR and b <= 32.


def test_instance_restates_theta_layout():
    src = open(os.path.join(ROOT, 'beta_cores_amd', 'csrc', 'bc_project.hip')).read()
    assert 'const int NTsel = raw ? 16 : tail ? 6 : nt <= 4 ? 4 : nt <= 7 ? 7 : nt <= 13 ? 13 : 16;' in src
    assert 'const bool tail = !raw && s > 96 && s <= 100 && !no_tail;' in src
    assert 'const int KC = NTsel <= 7 ? 32 : 16;' in src
    assert [K.instance(S)[:2] for S in (1, 64, 65, 96, 97, 100, 101, 112, 113, 208, 209, 256, 257)] == \
        [('4', 4), ('4', 4), ('7', 7), ('7', 7), ('6+4', 6), ('6+4', 6), ('7', 7), ('7', 7), ('13', 13), ('13', 13), ('16', 16), ('16', 16),
         ('RAW', 16)]


def test_inputs_are_what_the_docstring_says():
    for fam, n, d, S, kind in (('linreg', 129, 33, 64, 'wide'), ('logistic', 300, 17, 208, 'plain'), ('gauss', 17, 32, 65, 'wide')):
        a, b = K.inputs(fam, n, d, S, kind), K.inputs(fam, n, d, S, kind)
        assert np.array_equal(a['Z'], b['Z']) and np.array_equal(a['th'], b['th'])
        assert a['Z'].shape == (n, d + (fam == 'linreg')) and a['th'].shape == (S, d)
        assert np.isfinite(a['Z']).all() and np.isfinite(a['th']).all()
        zr = K.zero_rows(n)
        assert len(zr) == 2 and zr[-1] == n - 1
        assert not a['Z'][zr, :d].any() and a['Z'][np.setdiff1d(np.arange(n), zr), :d].any(axis=1).all()
    assert K.zero_rows(1) == [0]


# ------------------------------------------------------------------ not too tight
def test_float64_oracle_lies_inside_the_bound():
    """The float64 oracle and the same oracle with the features reversed, on every staged case and every model id: Phi, norms and
    column sums inside the bound (and using a part of it that shows the bound is no orders of magnitude off)."""
    need_longdouble()
    worst = (0., None)
    for c in K.STAGED:
        fam = c[0]
        inp, refs = K.case(*c)
        for src in (inp, reversed_inputs(fam, inp)):
            for mid in K.IDS[fam]:
                phi = centred(K.oracle_raw(mid, src['Z'], src['th'], src, K.BETA[fam]))
                r = K.ratios(refs[mid], *results(phi))
                assert max(r) <= 1., (c, mid, r)
                if max(r) > worst[0]:
                    worst = (max(r), (c, K.NAMES[mid]))
    print('worst error / bound of the float64 oracle: %.3f at %r' % worst)
    assert worst[0] > 0.02


def test_resident_inputs_meet_the_conditions_and_the_oracle_lies_inside():
    """The resident cases' inputs at 256 compute units, on the picked rows: the conditions, and the oracle inside the bound."""
    need_longdouble()
    n = K.resident_rows(256)
    assert n == 262_144 + 77
    worst = 0.
    for fam in K.FAMILIES:
        d, S = 37, 100
        inp = K.resident_inputs(fam, n, d, S)
        pick = K.resident_pick(n, np.random.RandomState(d + S))
        assert pick.size >= 300 and set([0, 1, 31, 32, 127, 128, n - 33, n - 32, n - 1] + K.zero_rows(n)) <= set(pick)
        for mid in K.IDS[fam]:
            ref = K.reference(fam, mid, inp, rows=pick)
            K.check_conditions(fam, ref, 'wide')
            phi = centred(K.oracle_raw(mid, inp['Z'][pick], inp['th'], inp, K.RESIDENT_BETA))
            r = K.ratios(ref, phi, results(phi)[1])
            assert max(r) <= 1., (fam, mid, r)
            worst = max(worst, max(r))
    print('worst error / bound of the float64 oracle on the resident inputs: %.3f' % worst)


# ------------------------------------------------------------------ not blind
class NumpyWith:
    """the numpy module with some functions replaced (handed to the oracle's modules in place of `np`)"""
    def __init__(self, **over):
        self._over = over

    def __getattr__(self, name):
        return self._over[name] if name in self._over else getattr(np, name)


def mutant_theta_float32(fam, mid, inp, beta):
    return centred(K.oracle_raw(mid, inp['Z'], inp['th'].astype(np.float32).astype(np.float64), inp, beta))


def mutant_last_feature_dropped(fam, mid, inp, beta):
    d = inp['th'].shape[1]
    if fam == 'gauss':                       # (the oracle contracts x with Siginv . theta: the feature is dropped from x)
        Z = inp['Z'].copy()
        Z[:, d - 1] = 0.
        return centred(K.oracle_raw(mid, Z, inp['th'], inp, beta))
    th = inp['th'].copy()
    th[:, d - 1] = 0.
    return centred(K.oracle_raw(mid, inp['Z'], th, inp, beta))


def mutant_padded_mean(fam, mid, inp, beta):
    raw = K.oracle_raw(mid, inp['Z'], inp['th'], inp, beta)
    return raw - (raw.sum(axis=1) / K.instance(raw.shape[1])[2])[:, None]


def mutant_exp_off_by_2_to_minus_40(fam, mid, inp, beta, monkeypatch):
    fake = NumpyWith(exp=lambda x: np.exp(x) * (1. + 2. ** -40))
    with monkeypatch.context() as mp:
        mp.setattr(K.M, 'np', fake)
        mp.setattr(K.L, 'np', fake)
        return centred(K.oracle_raw(mid, inp['Z'], inp['th'], inp, beta))


def mutant_last_row_duplicated(fam, mid, inp, beta):
    phi = centred(K.oracle_raw(mid, inp['Z'], inp['th'], inp, beta))
    phi[-1] = phi[-2]
    return phi


def mutant_matrix_mean(fam, mid, inp, beta):
    raw = K.oracle_raw(mid, inp['Z'], inp['th'], inp, beta)
    return raw - raw.mean()


MUTANTS = {
    'Theta rounded to float32': mutant_theta_float32,
    'the last feature dropped from the contraction': mutant_last_feature_dropped,
    'the mean divided by the padded sample count': mutant_padded_mean,
    'exp replaced by exp * (1 + 2^-40)': mutant_exp_off_by_2_to_minus_40,
    'the last row duplicated from the row before': mutant_last_row_duplicated,
    'centred with the matrix\'s mean': mutant_matrix_mean,
}
NO_EXP = (0, 4)        # the linear-regression and Gaussian log-likelihoods hold no exp


def old_bar_passes(phi, raw):
    """check_phi of tests/test_gpu_project.py on a float64 Phi (its column-sum and norm checks compare the result with itself)"""
    return bool(np.abs(phi - centred(raw)).max() <= 1e-11 * (1. + np.abs(raw).max()))


def test_six_mutants_leave_the_bound(monkeypatch):
    """Each wrong projection exceeds the bound on at least one listed case of every model id it can touch (staged cases with two
    rows and two samples or more).  Printed, for the 'wide' cases: how many (case, model id) results of each mutant the bar
    1e-11 * (1 + max|f| over the matrix) passes, and how many stay inside the derived bound (those the mutation leaves as they
    were: S equal to the padded count, a model without an exp)."""
    need_longdouble()
    caught = dict(((name, mid), 0) for name in MUTANTS for mid in range(9))
    tried = dict.fromkeys(MUTANTS, 0)
    old_passed = dict.fromkeys(MUTANTS, 0)
    new_passed = dict.fromkeys(MUTANTS, 0)
    for c in K.STAGED:
        fam, n, d, S, kind = c
        if n < 2 or S < 2:
            continue
        inp, refs = K.case(*c)
        for mid in K.IDS[fam]:
            raw = K.oracle_raw(mid, inp['Z'], inp['th'], inp, K.BETA[fam])
            for name, mutate in MUTANTS.items():
                phi = mutate(fam, mid, inp, K.BETA[fam], monkeypatch) if 'exp' in name else mutate(fam, mid, inp, K.BETA[fam])
                outside = max(K.ratios(refs[mid], *results(phi))) > 1.
                caught[(name, mid)] += outside
                if kind == 'wide':
                    tried[name] += 1
                    old_passed[name] += old_bar_passes(phi, raw)
                    new_passed[name] += not outside
    for name in MUTANTS:
        print('%-48s wide cases x ids: %3d; passed by 1e-11 * (1 + max|f|): %3d; inside the derived bound: %3d; caught per id %r'
              % (name, tried[name], old_passed[name], new_passed[name], [caught[(name, mid)] for mid in range(9)]))
    for (name, mid), k in caught.items():
        if 'exp' in name and mid in NO_EXP:
            assert k == 0, (name, mid)            # nothing to mutate: the same projection, still inside
            continue
        assert k >= 1, (name, K.NAMES[mid])


def test_ratios_see_a_nan():
    need_longdouble()
    inp, refs = K.case('linreg', 17, 32, 100, 'plain')
    phi = centred(K.oracle_raw(0, inp['Z'], inp['th'], inp, None))
    assert max(K.ratios(refs[0], *results(phi))) <= 1.
    phi[3, 4] = np.nan
    assert K.ratios(refs[0], *results(phi))[0] == float('inf')
