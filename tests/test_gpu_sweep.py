"""K3, the fp64 score + argmax sweep, held to planted winners at every position of its structure (tests/sweep_cases.py; the lists
are checked on the CPU by tests/test_sweep_cases_cpu.py), through every route that ends in a K3 argmax:

  DevicePhi.argmax      k_sweep<MODE> + k_local_winner (256 threads): every case -- the index, the value inside the derived
                        bound (the error / bound ratios are printed), the same bits on a second call
  a solver's first step b = v given explicitly, BC_PREFILTER=0: the fused finish kernel (dev_pick_blocks: the second strided
                        reducer of the per-block candidates, 512 threads), its BC_FINISH_NOFUSE and BC_FINISH_NOPF forms, and
                        the step-wise select() -- on one rank k_local_winner again, whose single record k_pick then reads;
                        BC_PREFILTER=8 (one-level int8) and 4 (two-level), whose rescoring stage repeats the sweep's chain,
                        must select the same row and cache the same column bytes

The winner's row is the only one that scores 1; runners-up at 0.999 sit where an indexing error would land, so a wrong index
is a lost row, not noise."""
import sys
import os

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sweep_cases as SC                                                         # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def bc():
    import beta_cores_amd as bc
    bc.default_context()
    return bc


@pytest.fixture(scope='module')
def bcv(bc):
    """for the tests that hold a value to the derived bound: they need the np.longdouble reference"""
    if not SC.LONGDOUBLE_OK:
        pytest.skip(SC.LONGDOUBLE_WHY)
    return bc


def n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count      # what bc_sweep_grid sizes the grid by (ctx->n_cu)


def argmax_checked(d, phi, v, mode, want, post_divs=(1.,), off=0, label=''):
    """argmax on the resident d = phi: index off + want, value inside the bound, a second call gives the same bits.
    Returns the worst error / bound ratio."""
    worst = 0.
    for pd in post_divs:
        f, val = d.argmax(v, mode=mode, post_div=pd)
        assert f == off + want, '%s: mode %d post_div %g offset %d: row %d for %d' % (label, mode, pd, off, f - off, want)
        r = SC.ratio(val, phi[want], v, mode, pd if mode == 1 else 1.)
        assert r <= 1., '%s: post_div %g: value %r is %.3g bounds from the reference' % (label, pd, val, r)
        f2, val2 = d.argmax(v, mode=mode, post_div=pd)
        assert f2 == f and np.array_equal(np.float64(val2).view(np.int64), np.float64(val).view(np.int64)), label
        worst = max(worst, r)
    return worst


def run_planted(bc, cases, S, mode):
    worst = (0., None)
    for label, n, winners in cases:
        phi, v, _ = SC.planted(n, S, mode, winners)
        d = bc.DevicePhi.from_host(phi)
        r = argmax_checked(d, phi, v, mode, min(winners), post_divs=(1., float(S)) if mode == 1 else (1.,), label=label)
        print('  K3 mode %d S %3d %s: error / bound %.3f' % (mode, S, label, r))
        worst = max(worst, (r, label))
    return worst


# ------------------------------------------------------------------ DevicePhi.argmax: planted positions and ties
@pytest.mark.parametrize('S,mode', [(S, m) for S in SC.S_ALL for m in SC.modes_of(S)])
def test_argmax_planted_positions(bcv, S, mode):
    bc = bcv
    cases = SC.small_cases(S, mode) + SC.small_ties()
    worst = run_planted(bc, cases, S, mode)
    # the runner-up's value: the winner's row replaced by one more runner-up, the lowest of the equal rows wins
    pos = SC.small_positions(SC.N_ODD)
    second = 0.
    for key in ('last row', 'block 1 first tile'):
        phi, v, want = SC.runners_alone(SC.N_ODD, S, mode, pos[key])
        assert want == pos[key] - SC.TILE
        second = max(second, argmax_checked(bc.DevicePhi.from_host(phi), phi, v, mode, want, post_divs=(1., float(S)) if mode == 1 else (1.,),
                                            label='runners-up alone, %s' % key))
    print('K3 mode %d S %3d: %3d cases, worst error / bound %.3f (the winner, 1) and %.3f (a runner-up alone, 0.999)'
          % (mode, S, len(cases), worst[0], second))


@pytest.mark.parametrize('mode', [0, 1])
def test_argmax_row_offsets(bcv, mode):
    bc = bcv
    """the shard's global indices cross 2^31 and 2^32 inside the Phi, and carry a high word above 2^33"""
    worst = 0.
    for p in SC.OFFSET_POSITIONS:
        phi, v, _ = SC.planted(SC.N_ODD, 4, mode, (p,))
        for off in SC.OFFSETS:
            d = bc.DevicePhi.from_host(phi, row_offset=off)
            assert d.row_offset == off
            worst = max(worst, argmax_checked(d, phi, v, mode, p, post_divs=(1., 4.) if mode == 1 else (1.,), off=off, label='row %d' % p))
    print('K3 mode %d S 4 row offsets: worst error / bound %.3f' % (mode, worst))


@pytest.mark.parametrize('S', [1, 2])
def test_argmax_first_positive_row_among_exact_signs(bc, S):
    phi, v1, v0, first = SC.sign_case(S)
    d = bc.DevicePhi.from_host(phi)
    for pd in (1., 4.):
        assert d.argmax(v1, mode=1, post_div=pd) == (first, 1. / pd)
    assert d.argmax(v0, mode=0) == (first, 1.)


def test_argmax_nan_rule(bc):
    """bc_better: NaN beats everything and the first NaN wins, as np.argmax has it"""
    for label, phi, v, mode, want in SC.nan_cases():
        sc = SC.numpy_scores(phi, v, mode)
        assert (int(np.argmax(sc)) if want >= 0 else -1) == want
        for off in (0, 2 ** 32 - 64):
            f, val = bc.DevicePhi.from_host(phi, row_offset=off).argmax(v, mode=mode)
            if want < 0:
                assert f == -1, label
            else:
                assert f == off + want and np.isnan(val), (label, f, val)


def test_argmax_giga_mask(bcv):
    bc = bcv
    """s1 = +-1 exactly: masked, scoring +-0 with the sign of s0 however large s0 is; s1 on either side of -1 + 1e-14"""
    for label, phi, v, want in SC.mask_cases():
        sc = SC.numpy_scores(phi, v, 0)
        assert int(np.argmax(sc)) == want
        d = bc.DevicePhi.from_host(phi)
        f, val = d.argmax(v, mode=0)
        assert f == want, (label, f, val)
        if sc[want] == 0.:
            assert val == 0. and np.signbit(val) == np.signbit(sc[want]), (label, val)
        else:
            r = SC.ratio(val, phi[want], v, 0)
            print('K3 mask case "%s": value %r, error / bound %.3f (bound %.3g relative)'
                  % (label, val, r, float(SC.bound(phi[want], v, 0)[0] / abs(SC.ref_score(phi[want], v, 0)[0]))))
            assert r <= 1., (label, val, r)
        f2, val2 = d.argmax(v, mode=0)
        assert f2 == f and np.float64(val2).view(np.int64) == np.float64(val).view(np.int64), label


# ------------------------------------------------------------------ grid strides and more candidates than a reducer has threads
def device_sized(case, mode):
    return [('n %d %s' % (case['n'], label), case['n'], (p,)) for label, p in case['positions'].items()] \
        + [('n %d tie: %s' % (case['n'], label), case['n'], w) for label, w in case['ties']]


@pytest.mark.parametrize('mode', [0, 1])
def test_argmax_three_grid_strides(bcv, monkeypatch, mode):
    bc = bcv
    """BC_SWEEP_BLOCKS_PER_CU=1 (read when the Phi is created): every block walks three tiles per wave"""
    monkeypatch.setenv('BC_SWEEP_BLOCKS_PER_CU', '1')
    for case in (SC.stride_case(n_cu()), SC.second_stride_case(n_cu())):
        worst = run_planted(bc, device_sized(case, mode), case['S'], mode)
        print('K3 mode %d S %3d n %d, grid %d: worst error / bound %.3f at %s' % ((mode, case['S'], case['n'], case['grid']) + worst))
    if mode == 1:
        c = SC.nan_stride_case(n_cu())
        f, val = bc.DevicePhi.from_host(c['phi']).argmax(c['v'], mode=1)
        assert f == c['expect'] and np.isnan(val)


@pytest.mark.parametrize('mode', [0, 1])
def test_argmax_more_blocks_than_reducer_threads(bcv, monkeypatch, mode):
    bc = bcv
    """4 blocks per CU (1024 on 256 CUs): candidates on the second, third and last trip of k_local_winner's 256 threads"""
    monkeypatch.delenv('BC_SWEEP_BLOCKS_PER_CU', raising=False)
    case = SC.wide_case(n_cu())
    worst = run_planted(bc, device_sized(case, mode), case['S'], mode)
    print('K3 mode %d S %3d n %d, grid %d: worst error / bound %.3f at %s' % ((mode, case['S'], case['n'], case['grid']) + worst))


# ------------------------------------------------------------------ a solver's first step
KNOBS = (None, 'BC_FINISH_NOFUSE', 'BC_FINISH_NOPF')
PREFILTER_FORM = {0: 0, 8: 1, 4: 3}        # bc_snnls_prefilter_form: fp64 sweeps, the one-level int8 sweep, the two-level form


def first_step_checked(bc, monkeypatch, alg, phi, v, want, label):
    """b = v: GIGA's first step scores phi . bn / |phi| with xw = 0, FrankWolfe's scores against b.  Every form selects `want`
    and caches the bytes of its row."""
    cls = dict(giga=bc.snnls.GIGA, fw=bc.snnls.FrankWolfe)[alg]
    d = bc.DevicePhi.from_host(phi)
    S = phi.shape[1]
    monkeypatch.delenv('BC_I8_BB', raising=False)
    forms = []
    for pref in (0, 8) + ((4,) if S <= 256 else ()):
        for knob in (KNOBS if pref == 0 else KNOBS[:1]):
            monkeypatch.setenv('BC_PREFILTER', str(pref))
            for k in KNOBS[1:]:
                monkeypatch.delenv(k, raising=False)
            if knob:
                monkeypatch.setenv(knob, '1')
            sv = cls(d.T, v)
            what = '%s %s BC_PREFILTER=%d %s' % (label, alg, pref, knob or 'default')
            assert sv._eng.prefilter == (8 if pref else 0) and sv._eng.prefilter_form == PREFILTER_FORM[pref], \
                '%s: pre-filter %d in form %d' % (what, sv._eng.prefilter, sv._eng.prefilter_form)
            sv.build(1)
            f, st, _ = sv._eng.trace()
            assert len(f) == 1 and f[0] == want, '%s: trace %r (status %r) for %d' % (what, f, st, want)
            forms.append((pref, knob, sv._eng.prefilter_form, sv._eng.finish_form()))
            idx, val = sv.sparse_weights()
            assert list(idx) == [want], what
            cols = sv._eng.columns()
            assert cols.shape == (1, S) and np.array_equal(cols[0].view(np.int64), phi[want].view(np.int64)), what
    for k in KNOBS[1:]:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('BC_PREFILTER', '0')
    sv = cls(d.T, v)
    f = sv._eng.select()                       # the step-wise protocol: k_sweep + k_local_winner, the record read by k_pick
    assert f == want, '%s %s select(): %d for %d' % (label, alg, f, want)
    sv._eng.reweight(f)
    assert list(sv.sparse_weights()[0]) == [want]
    assert np.array_equal(sv._eng.columns()[0].view(np.int64), phi[want].view(np.int64))
    return forms


@pytest.mark.parametrize('S', [4, 11, 257, 600])
@pytest.mark.parametrize('alg', ['giga', 'fw'])
def test_first_step_planted_positions(bc, monkeypatch, alg, S):
    """every planted position the argmax route runs at this S (at S = 4 and 11: all 14 at both n, and n = 1 ... 129) and every
    tie pair.  The pre-filters' tiles are 256 rows, so the positions fall differently there."""
    cases = SC.small_cases(S, 1) + SC.small_ties()
    forms = set()
    for label, n, winners in cases:
        phi, v, _ = SC.planted(n, S, 1, winners)
        forms |= set(first_step_checked(bc, monkeypatch, alg, phi, v, min(winners), 'S %d %s' % (S, label)))
    print('first step %s S %d: %d cases; (BC_PREFILTER, knob, pre-filter form, finish form): %s' % (alg, S, len(cases), sorted(forms, key=repr)))
    assert len(set(f for _, _, _, f in forms)) >= (2 if S <= 512 else 1)


@pytest.mark.parametrize('alg', ['giga', 'fw'])
def test_first_step_second_grid_stride(bc, monkeypatch, alg):
    """the fused step under BC_SWEEP_BLOCKS_PER_CU=1: winners on a second stride, a tie whose lower index lives in the higher block"""
    monkeypatch.setenv('BC_SWEEP_BLOCKS_PER_CU', '1')
    case = SC.second_stride_case(n_cu())
    for label, n, winners in device_sized(case, 1):
        phi, v, _ = SC.planted(n, case['S'], 1, winners)
        first_step_checked(bc, monkeypatch, alg, phi, v, min(winners), label)


@pytest.mark.parametrize('alg', ['giga', 'fw'])
def test_first_step_more_blocks_than_reducer_threads(bc, monkeypatch, alg):
    """4 blocks per CU: candidates beyond the 512 threads of dev_pick_blocks (the default form) and beyond the 256 of
    k_local_winner (BC_FINISH_NOFUSE, BC_FINISH_NOPF, select()), and ties across their trips"""
    monkeypatch.delenv('BC_SWEEP_BLOCKS_PER_CU', raising=False)
    case = SC.wide_case(n_cu())
    for label, n, winners in device_sized(case, 1):
        phi, v, _ = SC.planted(n, case['S'], 1, winners)
        first_step_checked(bc, monkeypatch, alg, phi, v, min(winners), label)
