"""The cases of tests/step_cases.py held on the CPU, before tests/test_gpu_step.py runs them on the device.  Conditions, not
measurements: every case's reference step succeeds with room to spare, its winner is decided by 1e-6 or more, its derived bound is
tight enough to be worth holding a kernel to (1e-9 of a weight) and loose enough for honest float64 (NumPy's own evaluation lies
inside it), the list lengths walk every loop of dev_xw_err_t (xw_walk, written from the kernel text), and three mutants of the xw
rebuild are caught -- in the cases xw_walk names and in no other."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import step_cases as SC                                                          # noqa: E402

pytestmark = pytest.mark.skipif(not SC.LONGDOUBLE_OK, reason=SC.LONGDOUBLE_WHY)
LD = SC.LD

WEIGHT_CAP = 1e-9          # bound on a new weight / |weight|
ERROR_CAP = 1e-9           # bound on the new error / max(error, 1e-3 |b|)
MARGIN = 1e-6              # the winner's score above the runner-up's


def one_round(S, nnz0):
    """the step from a list of nnz0 entries runs dev_xw_err_t<true> in the one-round forms"""
    return S <= SC.FIN_THREADS and nnz0 + 1 <= SC.PF_MAXNNZ


# ------------------------------------------------------------------ the lists against the loop model
def test_walk_partitions_the_list():
    for S in (2, 3, 65, 100, 257, 512, 513):
        for nnz in (0, 1, 79, 80, 81, 183, 1025):
            for pf in (False, True):
                w = SC.xw_walk(S, nnz, pf)
                entries = sorted(j for lst in w.values() for _, j in lst)
                assert entries == list(range(nnz)), (S, nnz, pf)
                G = SC.groups(S)
                assert all(j % G == g for lst in w.values() for g, j in lst)
                assert all(j < SC.PF_NC * G for _, j in w['c16']) and (pf or not w['c16'])


@pytest.mark.parametrize('alg', SC.ALGS)
def test_lengths_enter_every_loop(alg):
    """Per S: every loop of dev_xw_err_t is entered, in the template that runs it, and the appended entry falls on both sides of
    the up-front loads.  Where the one-round kernel hands over to the plain kernel (1024 entries) before its list can leave the
    up-front loads (S < 16: 31 G >= 1023), the loops behind them are walked by the plain kernel's template alone -- stated
    here as what the model says, not skipped."""
    for S in SC.S_of(alg):
        G = SC.groups(S)
        seen = {False: set(), True: set()}
        new_in = set()
        for nnz0, kind in SC.cases(S, alg):
            nnz1 = nnz0 + (1 if kind in ('fresh', 'zeros', 'all_zero') else 0)
            for nnz, pf in ((nnz0, False), (nnz1, False)) + (((nnz1, True),) if one_round(S, nnz0) else ()):
                seen[pf] |= set(k for k, lst in SC.xw_walk(S, nnz, pf).items() if lst)
            if one_round(S, nnz0) and nnz1 == nnz0 + 1:
                new_in.add(SC.loop_of(S, nnz1, True, nnz0))
        if S > SC.FIN_THREADS:
            assert seen[False] == {'serial'} and not seen[True], S
            continue
        assert seen[False] >= {'x16', 'x4', 'tail'}, (S, seen)
        assert 'c16' in seen[True]
        longest = SC.xw_walk(S, SC.PF_MAXNNZ, True)
        if longest['x16']:
            assert seen[True] >= {'c16', 'x16', 'x4', 'tail'}, (S, seen)
        else:
            assert 31 * G >= SC.PF_MAXNNZ - 1 and S < 17
        if 16 * G + 1 <= SC.PF_MAXNNZ - 1:
            assert 'c16' in new_in and len(new_in - {'c16'}) >= 1, (S, new_in)
        else:
            assert new_in == {'c16'}, (S, new_in)
        # both sides of the hand-over, and a revisit on either side of the up-front loads
        lens = [L for L, _ in SC.cases(S, alg)]
        assert 1023 in lens and 1024 in lens and 16 * G in lens and 16 * G - 1 in lens and 16 * G + 1 in lens
        assert SC.form_of(S, 1023, 'BC_PREFILTER=0 default') == SC.ONE_ROUND and SC.form_of(S, 1024, 'BC_PREFILTER=0 default') == SC.PLAIN
        for kind, head in (('revisit_head', True), ('revisit_behind', False)):
            c = SC.planted(S, 36 * G + 3, alg, kind)
            slot = int(np.flatnonzero(c['idx'] == c['f'])[0])
            assert (slot < SC.PF_NC * G) == head and c['val'][slot] > 0


def test_full_lengths_at_s_100():
    G = 5
    assert SC.all_lengths(100) == sorted({0, 1, G - 1, G, G + 1, 79, 80, 81, 99, 100, 159, 160, 161, 183, 1022, 1023, 1024, 1025})
    for S in SC.S_ONE_ROUND + SC.S_PLAIN:
        assert set(SC.edge_lengths(S)) <= set(SC.all_lengths(S))


# ------------------------------------------------------------------ every case: conditions on the reference step
@pytest.mark.parametrize('alg,S', [(a, S) for a in SC.ALGS for S in SC.S_of(a)])
def test_cases_hold_their_conditions(alg, S):
    worst = dict(weight=0., error=0., f64=0., margin=np.inf)
    for nnz, kind in SC.cases(S, alg):
        what = '%s S %d nnz %d %s' % (alg, S, nnz, kind)
        c = SC.planted(S, nnz, alg, kind)
        assert len(set(c['idx'].tolist())) == nnz and (nnz < 3 or (np.diff(c['idx']) < 0).any()), what
        listed = c['f'] in c['idx']
        assert listed == kind.startswith('revisit'), what
        npos = int((c['val'] > 0).sum())
        assert npos == (0 if kind == 'all_zero' else nnz) or (kind == 'zeros' and 0 < npos < nnz), what
        r = SC.ref_step(alg, c['phi'], c['b'], c['idx'], c['val'], c['f'])
        assert r['ok'] and r['safe'], '%s: the reference step fails or its own bound lets it fail: %r' % (what, r['g'] and [float(x.v) for x in r['g']])
        assert r['at_new'] == (-1 if listed else nnz), what
        pre, post = r['pre']['err'], r['post']['err']
        if r['pre']['npos'] > 0:                          # (the guard is off for an empty set: snnls.py:44-45)
            assert pre.v - pre.bound() > post.v + post.bound(), '%s: the guard could trip by rounding' % what
        m = SC.margin(SC.scores(alg, c['phi'], c['b'], c['idx'], c['val']), c['f'])
        assert m >= MARGIN, '%s: the winner leads by %.3g' % (what, m)
        w1 = r['w1']
        nz = w1.v != 0
        assert np.all(w1.bound()[~nz] == 0), what
        wrel = float((w1.bound()[nz] / np.abs(w1.v[nz])).max())
        assert wrel <= WEIGHT_CAP, '%s: weight bound %.3g of the weight' % (what, wrel)
        bnorm = float(np.sqrt((c['b'] ** 2).sum()))
        erel = float(post.bound() / max(float(post.v), 1e-3 * bnorm))
        assert erel <= ERROR_CAP, '%s: error bound %.3g' % (what, erel)
        r64 = SC.ref_step(alg, c['phi'], c['b'], c['idx'], c['val'], c['f'], dtype=np.float64)
        assert r64['ok'] and np.array_equal(r64['idx1'], r['idx1'])
        q = max(SC.ratio(r64['w1'].v, w1), SC.ratio(r64['post']['err'].v, post), SC.ratio(r64['pre']['err'].v, pre),
                SC.ratio(r64['post']['xw'].v, r['post']['xw']))
        assert q <= 1., '%s: float64 NumPy is %.3g bounds from the reference' % (what, q)
        worst = dict(weight=max(worst['weight'], wrel), error=max(worst['error'], erel), f64=max(worst['f64'], q), margin=min(worst['margin'], m))
    print('step cases %s S %4d: %2d cases; bound / weight <= %.2g, error bound <= %.2g, float64 NumPy / bound <= %.3f, margin >= %.3g'
          % (alg, S, len(SC.cases(S, alg)), worst['weight'], worst['error'], worst['f64'], worst['margin']))


# ------------------------------------------------------------------ mutants of the xw rebuild
MUTANT_S = (65, 100, 257, 512)


def mutated_error(c, r, mutant):
    """(||xw - b|| with the mutant's xw after the step, whether xw_walk says this case meets the mutant)"""
    S, nnz0 = c['S'], c['nnz']
    P = np.asarray(c['phi'], dtype=LD)
    cols = P[r['idx1']].copy()
    w = r['w1'].v
    nnz1, at_new = cols.shape[0], r['at_new']
    pf = one_round(S, nnz0)
    G = SC.groups(S)
    if mutant == 'drop':                                  # the last entry the tail loop serves (else the last of the list)
        tail = SC.xw_walk(S, nnz1, pf)['tail']
        j = max(j for _, j in tail) if tail else nnz1 - 1
        xw = SC.xw_model(S, w, cols, drop=j)
        meets = nnz1 > 0 and w[j] != 0
    elif mutant == 'no_xf':                               # the slot of the up-front loads as it was loaded: clamped to nnz0 - 1
        meets = pf and at_new >= 0 and SC.loop_of(S, nnz1, True, at_new) == 'c16'
        if meets:
            cols[at_new] = cols[nnz0 - 1] if nnz0 > 0 else 0
        xw = SC.xw_model(S, w, cols)
    else:                                                 # G rounded up: the last group is short of threads
        Gup = -(-SC.FIN_THREADS // S)
        xw = SC.xw_model(S, w, cols, G=Gup)
        meets = Gup != G and nnz1 >= Gup and bool(np.any(w[Gup - 1::Gup] != 0))
    d = xw - np.asarray(c['b'], dtype=LD)
    return np.sqrt((d * d).sum()), bool(meets)


@pytest.mark.parametrize('mutant', ['drop', 'no_xf', 'G_up'])
def test_mutants_are_caught_where_the_walk_says(mutant):
    caught, named, total = [], [], 0
    for alg in SC.ALGS:
        for S in MUTANT_S:
            for nnz, kind in SC.cases(S, alg):
                c = SC.planted(S, nnz, alg, kind)
                r = SC.ref_step(alg, c['phi'], c['b'], c['idx'], c['val'], c['f'])
                post = r['post']['err']
                P = np.asarray(c['phi'], dtype=LD)
                honest = SC.xw_model(S, r['w1'].v, P[r['idx1']])
                assert SC.ratio(honest.astype(np.float64), r['post']['xw']) <= 1., 'the model itself'
                err, meets = mutated_error(c, r, mutant)
                total += 1
                key = (alg, S, nnz, kind)
                if meets:
                    named.append(key)
                if abs(err - post.v) > 10 * post.bound():
                    caught.append(key)
    print('mutant %s: caught in %d of %d cases, xw_walk names %d' % (mutant, len(caught), total, len(named)))
    assert caught, 'no case catches the mutant %s' % mutant
    assert set(caught) <= set(named), sorted(set(caught) - set(named))
    assert set(caught) == set(named), 'cases that meet the mutant and let it pass: %r' % sorted(set(named) - set(caught))[:5]
    if mutant == 'G_up':
        assert not any(S in (256, 512) for _, S, _, _ in named) and any(S == 100 for _, S, _, _ in caught)
    if mutant == 'no_xf':
        assert all(nnz < SC.PF_NC * SC.groups(S) for _, S, nnz, _ in named)
