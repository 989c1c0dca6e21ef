"""The greedy step -- k_step_finish_pf<alg, RS>, k_step_finish<alg>, k_reweight<alg>, k_set_weights and their stages in
bc_snnls_dev.h -- held to the np.longdouble reference step of tests/step_cases.py from PLANTED list states, inside a derived
running error bound (1e-11 of a weight or so: tests/test_step_cases_cpu.py holds the cases and the bound), in every form of the
finish kernel the environment offers:

  BC_PREFILTER=0                      one round of loads, the winner from the sweep's block candidates
  BC_PREFILTER=8 BC_FINISH_NOFUSE     one round of loads, the winner from k_rescore's record
  BC_PREFILTER=0 BC_FINISH_NOPF       the plain kernel (also: S > 512 and lists of 1024 entries and more, in every form)
  BC_PREFILTER=8 / 4                  one round with the rescoring inside (int8 one-level / two-level, S <= 256)
  BC_PREFILTER=8 BC_I8_BB=1           one round behind the branch-and-bound sweep (S <= 256)
  select() + reweight(f)              the step-wise protocol: k_pick and k_reweight

Per form: set_sparse_weights(idx, val) (the columns come from the shard), the state read back, build(1), build(1) again, and on a
second solver build(2) in one call, whose list-length hint takes both lengths.  The list lengths sit at the edges of
dev_xw_err_t's loops (16 G, 20 G, 32 G, 36 G + 3 for G = 512 / S thread groups) and at the hand-over to the plain kernel (1023 /
1024); the second step is bounded from the list the device returned after the first, so bounds do not compound."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import step_cases as SC                                                          # noqa: E402
from test_gpu_snnls import _build_in_every_form                                  # noqa: E402

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


def forms_of(S):
    """[(BC_PREFILTER, knob, BC_I8_BB)]; above 512 columns every form runs the plain kernel and the knobs choose nothing"""
    if S > SC.FIN_THREADS:
        return [(0, None, False), (8, None, False)]
    out = [(0, None, False), (8, 'BC_FINISH_NOFUSE', False), (0, 'BC_FINISH_NOPF', False), (8, None, False)]
    if S <= 256:
        out += [(4, None, False), (8, None, True)]
    return out


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


class Step(object):
    """what a solver shows after a step"""

    def __init__(self, sv):
        self.idx, self.val = sv._eng.sparse_weights()
        self.err = sv._eng.error()

    def same(self, o):
        return np.array_equal(self.idx, o.idx) and same_bits(self.val, o.val) and same_bits(np.float64(self.err), np.float64(o.err))


def held(step, ref, what):
    """the list, every weight and the error against a reference step; returns the worst error / bound ratio"""
    assert np.array_equal(step.idx, ref['idx1']), '%s: the list %r for %r' % (what, step.idx[-3:], ref['idx1'][-3:])
    rw = SC.ratio(step.val, ref['w1'])
    re = SC.ratio(step.err, ref['post']['err'])
    assert rw <= 1., '%s: a weight is %.3g bounds from the reference' % (what, rw)
    assert re <= 1., '%s: error() %r is %.3g bounds from the reference %r' % (what, step.err, re, float(ref['post']['err'].v))
    return max(rw, re)


def run_case(bc, monkeypatch, c):
    """one planted case in every form; returns (worst ratio, the forms seen)"""
    alg, S, nnz0 = c['alg'], c['S'], c['nnz']
    phi, b = c['phi'], c['b']
    tag = '%s S %d nnz %d %s' % (alg, S, nnz0, c['kind'])
    ref1 = SC.ref_step(alg, phi, b, c['idx'], c['val'], c['f'])
    assert ref1['ok']
    d = bc.DevicePhi.from_host(phi)
    first = {}                  # what the first form left: the other forms must leave the same bits
    worst = [0.]
    seen = set()

    def second_reference(s1, f2):
        if 'ref2' not in first:
            sc = SC.scores(alg, phi, b, s1.idx, s1.val)
            assert float(sc.max() - sc[f2]) <= 1e-9 * float(np.abs(sc).max()), '%s: the second pick %d scores %r, the best row %r' % (tag, f2, sc[f2], sc.max())
            first['ref2'] = SC.ref_step(alg, phi, b, s1.idx, s1.val, f2)
            assert first['ref2']['ok'], tag
        return first['ref2']

    def failed_second(s1, f2, what):
        if f2 < 0:
            cn = ref1['nxt']['cn']
            assert alg == 'giga' and float(cn.v - cn.bound()) < 1e-12, '%s: _select failed with |cdir| = %r' % (what, float(cn.v))
            return
        if 'ref2' not in first:
            first['ref2'] = SC.ref_step(alg, phi, b, s1.idx, s1.val, f2)
        r2 = first['ref2']
        guard = r2['ok'] and float(r2['post']['err'].v + r2['post']['err'].bound()) >= float(r2['pre']['err'].v - r2['pre']['err'].bound())
        assert not (r2['ok'] and r2['safe']) or guard, '%s: the second step failed where the reference succeeds: %r' % (
            what, [float(x.v) for x in r2['g']])

    def agree(key, got, what):
        if key not in first:
            first[key] = got
        elif isinstance(got, Step):
            assert got.same(first[key]), '%s: %s differs from the first form\'s bits' % (what, key)
        else:
            assert same_bits(got, first[key]), '%s: %s differs from the first form\'s bits' % (what, key)

    def run(label, sv):
        what = '%s [%s]' % (tag, label)
        eng = sv._eng
        # the planted state as k_set_weights and the non-prefetching dev_xw_err left it
        i0, v0 = eng.sparse_weights()
        assert np.array_equal(i0, c['idx']) and same_bits(v0, c['val']), what
        assert same_bits(eng.columns(), phi[c['idx']]), what
        r0 = SC.ratio(eng.error(), ref1['pre']['err'])
        assert r0 <= 1., '%s: error() of the planted state is %.3g bounds from the reference' % (what, r0)
        worst[0] = max(worst[0], r0)
        assert sv.size() == ref1['pre']['npos']
        if label == 'step-wise':
            f = eng.select()
            assert f == c['f'], '%s: select() %d for %d' % (what, f, c['f'])
            eng.reweight(f)
            s1 = Step(sv)
            agree('step 1', s1, what)
            if first['st2'] == 1:
                # the fused forms' second step failed: k_reweight refuses the same step sizes and moves nothing -- or the
                # fused guard reverted a step that raised the error, which the protocol leaves to its host loop
                try:
                    eng.reweight(eng.select())
                except bc.NumericalPrecisionError:
                    agree('step 2', Step(sv), what)
                else:
                    assert eng.error() > s1.err, what
                return
            f2 = eng.select()
            assert f2 == first['f2'], what
            eng.reweight(f2)
            agree('step 2', Step(sv), what)
            return
        redone = eng.prefilter_fallbacks()
        sv.build(1)
        f, st, er = eng.trace()
        assert len(f) == 1 and f[0] == c['f'] and st[0] == 0, '%s: trace %r status %r for %d' % (what, f, st, c['f'])
        form = eng.finish_form()
        assert form == SC.form_of(S, nnz0, label, eng.prefilter_fallbacks() > redone), '%s: finish form %d' % (what, form)
        seen.add(form)
        s1 = Step(sv)
        worst[0] = max(worst[0], held(s1, ref1, what + ' step 1'))
        assert same_bits(np.float64(er[0]), np.float64(s1.err))
        agree('step 1', s1, what)
        assert same_bits(eng.columns(), phi[s1.idx]), what
        redone = eng.prefilter_fallbacks()
        sv.build(1)
        f, st, er = eng.trace()
        assert len(f) == 2, what
        assert eng.finish_form() == SC.form_of(S, len(s1.idx), label, eng.prefilter_fallbacks() > redone), \
            '%s: second step: finish form %d' % (what, eng.finish_form())
        first.setdefault('f2', int(f[1]))
        first.setdefault('st2', int(st[1]))
        assert f[1] == first['f2'] and st[1] == first['st2'], what
        s2 = Step(sv)
        if st[1] == 0:
            worst[0] = max(worst[0], held(s2, second_reference(s1, int(f[1])), what + ' step 2'))
        else:
            # a failed second step: the reference fails too, or its own bound lets it fail, and nothing moved
            failed_second(s1, int(f[1]), what)
            assert s2.same(s1), '%s: the second step failed (f = %d) and moved the state' % (what, f[1])
        agree('step 2', s2, what)
        agree('trace errors', er, what)
        # build(2) in one call on a sibling (the environment is still this form's)
        sib = type(sv)(d.T, b)
        sib._eng.set_sparse_weights(c['idx'], c['val'])
        sib.build(2)
        f_, st_, er_ = sib._eng.trace()
        assert np.array_equal(f_, f) and np.array_equal(st_, st) and same_bits(er_, er), what + ' build(2)'
        assert Step(sib).same(s2), '%s: build(2) differs from build(1) + build(1)' % what
        assert sib._eng.finish_form() == eng.finish_form()

    _build_in_every_form(bc, monkeypatch, alg, phi, None, b=b, A=d.T, state=(c['idx'], c['val']), forms=forms_of(S), run=run)
    return worst[0], seen


@pytest.mark.parametrize('alg,S', [(a, S) for a in SC.ALGS for S in SC.S_of(a)])
def test_step_planted_states(bcv, monkeypatch, alg, S):
    bc = bcv
    worst, forms, at = 0., set(), None
    for nnz, kind in SC.cases(S, alg):
        r, seen = run_case(bc, monkeypatch, SC.planted(S, nnz, alg, kind))
        forms |= seen
        if r >= worst:
            worst, at = r, (nnz, kind)
    print('step %s S %4d: %2d cases in %d forms, finish forms %s; worst error / bound %.3f at %r'
          % (alg, S, len(SC.cases(S, alg)), len(forms_of(S)) + 1, sorted(forms), worst, at))
    want = {SC.PLAIN} if S > SC.FIN_THREADS else {SC.PLAIN, SC.ONE_ROUND, SC.ONE_ROUND_RESCORE} | ({SC.ONE_ROUND_BB} if S <= 256 else set())
    assert forms == want


@pytest.mark.parametrize('S', [9, 600])
@pytest.mark.parametrize('alg', SC.ALGS)
def test_failed_step_leaves_the_planted_state(bc, monkeypatch, alg, S):
    """The colinear design of test_finish_kernels_agree_on_failure_branches from a planted list of 1 and of 16 G + 1 entries: a
    step that ends with status 1 (GIGA's _select raises; FrankWolfe's line search or the guard refuses) leaves indices, weights
    and error() bit-equal to what they were, in every form, and the forms agree step by step."""
    for nnz0 in SC.colinear_lengths(S):
        c = SC.colinear(S, nnz0, alg)
        tag = '%s S %d nnz %d colinear' % (alg, S, nnz0)
        d = bc.DevicePhi.from_host(c['phi'])
        first = {}
        failed = []

        def run(label, sv):
            if label == 'step-wise':
                return
            what = '%s [%s]' % (tag, label)
            steps = []
            for m in range(3):
                before = Step(sv)
                if m == 0:
                    assert np.array_equal(before.idx, c['idx']) and same_bits(before.val, c['val']), what
                sv.build(1)
                f, st, er = sv._eng.trace()
                assert len(f) == m + 1
                after = Step(sv)
                if st[m] == 1:
                    failed.append(label)
                    assert after.same(before), '%s: step %d failed (f = %d) and moved the state' % (what, m, f[m])
                steps.append((int(f[m]), int(st[m]), after))
                if sv.reached_numeric_limit:
                    break
            if 'steps' not in first:
                first['steps'] = steps
                print('%s: (f, status) %r' % (tag, [(a, s_) for a, s_, _ in steps]))
            else:
                assert len(steps) == len(first['steps']), what
                for (fa, sa, xa), (fb, sb, xb) in zip(steps, first['steps']):
                    assert fa == fb and sa == sb and xa.same(xb), what

        runs = _build_in_every_form(bc, monkeypatch, alg, c['phi'], None, b=c['b'], A=d.T, state=(c['idx'], c['val']), forms=forms_of(S), run=run)
        assert set(failed) == set(r[0] for r in runs[:-1]), '%s: no step ended with status 1 in %r' % (tag, sorted(set(r[0] for r in runs[:-1]) - set(failed)))
