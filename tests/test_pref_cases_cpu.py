"""The checker of tests/pref_cases.py is neither too tight nor blind, shown without a GPU on the NumPy model of
tests/pref_model.py (the builders, the vector quantisers and the interval formulas, float64 / float32 where the device is):

  * the faithful model passes the checker on every case (matrix, vector, both levels);
  * every doctored model -- one deliberate defect each, of the kind the argmax-only GPU tests cannot see -- is rejected on the
    committed cases, by the check that is meant to see it (the failure names it);
  * the adversarial vectors do their job: the model attains at least 0.9 (S >= 37) and 0.8 (S = 8) of the half-width on the
    targeted row for each of the bound's three terms, and with the mirror and record checks switched off the CONTAINMENT check
    alone still rejects an understated delta, fev0 and fev1;
  * the layout formulas restated in Python are those of csrc/bc_layout.h compiled for the host."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import pref_cases as P            # noqa: E402
import pref_model as M            # noqa: E402

CASES = P.case_list()


def run_case(S, n, doctor=None, names=None, skip=()):
    """The model on every vector of one case matrix; returns {vector name: stats per level}."""
    phi = P.case_phi(S, n)
    prev, seeds = P.previous_vector(S, n)
    cache, memo, out = {}, {}, {}
    for name, mode, v, pd, term, row in P.case_vectors(S, n):
        if names is not None and name.split(':')[0] not in names:
            continue
        s = M.run_model(phi, mode, v, pd, seeds=seeds, v_prev=prev, doctor=doctor, mirrors=cache)
        out[name] = (P.check_all(s, skip=skip, memo=memo), term, row)
    return out


@pytest.mark.parametrize('S,n', CASES, ids=lambda x: str(x))
def test_model_passes_the_checker(S, n):
    res = run_case(S, n)
    assert res
    if n >= 64 and S >= 8:
        # the special rows did what they are for: uncertain rows on the slope vectors at both levels, finite ones beside them
        st = res['slope'][0]
        assert st['i8']['uncertain'] >= 2 and st['i8']['rows'] > st['i8']['uncertain']
        if S <= 256:
            assert st['i4']['uncertain'] > st['i8']['uncertain']


# doctored model -> (the check that must reject it, matrices on which it must, vectors that suffice)
DOCTORS = {
    'delta_nearest': ('int8 delta below the measured error', None),
    'delta_x095': ('int8 delta below the measured error', None),
    'scale_nearest': ('int8 scale', None),
    'fev0_x09': ('fev0', ['vec']),
    'fev1_x09': ('fev1', ['slope']),
    'no_slope': ('int8 interval', ['slope']),
    'l2_next_row': ('level 2 interval', ['random', 'vec']),
    'r8_shifted': ('r8 record', None),
    'i4_clip6': ('4-bit digit', None),
    'theta0_stale': ('theta0', ['scaled']),
}
DOCTOR_CASES = [(37, 3001), (99, 3001), (8, 300), (203, 3001)]


@pytest.mark.parametrize('S,n', DOCTOR_CASES, ids=lambda x: str(x))
@pytest.mark.parametrize('doctor', sorted(DOCTORS))
def test_doctored_models_are_rejected(doctor, S, n):
    want, names = DOCTORS[doctor]
    with pytest.raises(AssertionError) as err:
        run_case(S, n, doctor=doctor, names=names)
    assert str(err.value).startswith(want), str(err.value)


@pytest.mark.parametrize('S,n', [c for c in DOCTOR_CASES if c[0] >= 37], ids=lambda x: str(x))      # (S = 8 attains 0.83 < 1 / 0.9)
@pytest.mark.parametrize('doctor,names', [('delta_x095', ['row8']), ('fev0_x09', ['vec']), ('fev1_x09', ['slope'])])
def test_containment_alone_sees_an_understated_bound(doctor, names, S, n):
    """Without the direct checks of the mirror and of the record, the adversarial vector still exposes the defect: the exact
    score leaves [L, U].  (On the random vectors of the same matrix it does not: that is why the cases exist.)"""
    with pytest.raises(AssertionError) as err:
        run_case(S, n, doctor=doctor, names=names, skip=('mirror', 'record'))
    assert 'is outside [L, U]' in str(err.value), str(err.value)
    run_case(S, n, doctor=doctor, names=['random', 'random-giga'], skip=('mirror', 'record'))


def test_attainment_of_every_term():
    worst = {}
    for S, n in CASES:
        if n < 64 or S < 8:
            continue
        best = {}
        for name, (st, term, row) in run_case(S, n, names=['row8', 'row4', 'vec', 'slope']).items():
            level = 'i4' if term == 'row4' else 'i8'
            a = float(st[level]['attain_rows'][row])
            best[term] = max(best.get(term, 0.), a)
        print('S %3d n %4d  ' % (S, n) + '  '.join('%s %.4f' % kv for kv in sorted(best.items())))
        for term in ('row', 'vec', 'slope'):
            assert best[term] >= (0.9 if S >= 37 else 0.8), (S, n, term, best[term])
        if 'row4' in best:
            assert best['row4'] >= 0.8, (S, n, best['row4'])
        for term, a in best.items():
            key = (term, S >= 37)
            worst[key] = min(worst.get(key, 1.), a)
    print('worst model attainment (term, S >= 37):', sorted(worst.items()))


def test_layout_formulas_are_the_headers(tmp_path):
    exe = str(tmp_path / 'pref_layout_harness')
    cmd = ['gcc', '-O2', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'beta_cores_amd', 'csrc'),
           os.path.join(ROOT, 'tests', 'pref_layout_harness.c'), '-o', exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    res = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout + res.stderr
    seen = 0
    for line in res.stdout.splitlines():
        w = line.split()
        x = [int(t) for t in w[1:]]
        if w[0] == 'S':
            S = x[0]
            assert x[1:] == [M.lay_i8_sp4(S), M.lay_i4_batch(S), M.lay_i4_sp8(S, M.lay_i4_batch(S)), M.lay_r8_bytes(S)], line
        elif w[0] == 'w8':
            assert M.lay_i8_word(*x[:4]) == x[4], line
        elif w[0] == 'w4':
            assert M.lay_i4_word(*x[:4]) == x[4], line
        elif w[0] == 'phi':
            assert M.lay_phi_elem(*x[:3]) == x[3], line
        elif w[0] == 'tiles':
            assert x == [M.lay_i8_tiles(0), M.lay_i8_tiles(256), M.lay_i8_tiles(257)]
        seen += 1
    assert seen == 300 + 81 + 1


def test_the_packers_and_the_decoders_agree():
    """pref_model packs by reshaping, pref_cases decodes through the index formulas: a round trip through both."""
    rng = np.random.RandomState(5)
    for S in (5, 37, 104, 253):
        ptiles, sp4 = 3, M.lay_i8_sp4(S)
        sp8 = M.lay_i4_sp8(S, M.lay_i4_batch(S))
        q8 = rng.randint(-127, 128, size=(ptiles * 256, 4 * sp4)).astype(np.int32)
        q4 = rng.randint(-7, 8, size=(ptiles * 256, 8 * sp8)).astype(np.int32)
        s = M.Snap(ptiles=ptiles, sp4=sp4, sp8=sp8, u8=M.pack_i8(q8, ptiles, sp4), u4=M.pack_i4(q4, ptiles, sp8))
        assert np.array_equal(P.decode_i8(s), q8) and np.array_equal(P.decode_i4(s), q4)
