"""How the chain summary is threaded through the samplers, without a GPU: a recording stand-in for the batched engine (the calls
of _DeviceHMCMany that _run_hmc_group makes), the stand-in engine and scorer of tests/test_valuation_cpu.py for the route that
returns its samples, and a stand-in summarizer written with NumPy.  Warm-up chunks are never folded in, kept chunks are folded in
order, summary=False performs exactly the calls of a run without the option, stream positions are unchanged,
keep_samples=False with summary=True returns no samples and a summary, and tmc_shapley(summary=True) fills its two arrays and
changes no value of phi."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import diag_cases as DC                                                          # noqa: E402
import test_valuation_cpu as tv                                                  # noqa: E402
from beta_cores_amd import samplers, valuation                                   # noqa: E402


def numpy_summarizer(samples, max_lag=None):
    """chain_summary's stand-in: the restatement of tests/diag_cases.py in float64"""
    r = DC.summary(np.asarray(samples), max_lag, dtype=np.float64)
    return samplers.ChainSummary(r['mean'], r['cov'], r['rhat'], r['ess'], r['truncated'] != 0, 0)


class RecordingMany:
    """The batched engine's protocol as _run_hmc_group drives it, every call written down.  Samples: the chunk's normals plus the
    problem's number; every draw is accepted."""

    def __init__(self, P, with_fold=True):
        self.P, self.calls, self.kept = P, [], []
        if not with_fold:                                      # an engine from before the option: it takes no fold argument
            self.chunk = self._chunk_plain
            self.chunk_scored = self._chunk_scored_plain

    def begin(self, starts, inv_mass, n_leapfrog, n_iter):
        self.calls.append(('begin', n_iter))
        self.c, self.d = starts.shape[1:]

    def auto_chunk(self, c, d):
        return 3

    def attach_summary(self, n_keep, max_lag):
        self.calls.append(('attach', n_keep, max_lag))

    def _run(self, normals):
        k = normals.shape[0]
        s = normals[None] + np.arange(self.P)[:, None, None, None]
        return k, s, s.sum(axis=3), np.ones((self.P, k, self.c), dtype=np.int32), np.zeros(self.P, dtype=np.int32)

    def chunk(self, normals, log_u, steps, shared, fold=False):
        k, s, lj, acc, st = self._run(normals)
        self.calls.append(('chunk', k, fold))
        if fold:
            self.kept.append(s)
        return s, lj, acc, st

    def chunk_scored(self, normals, log_u, steps, shared, held, keep_samples, fold=False):
        k, s, lj, acc, st = self._run(normals)
        self.calls.append(('chunk_scored', k, held is not None, keep_samples, fold))
        if fold:
            self.kept.append(s)
        cor = np.full((self.P, k, self.c), 7, dtype=np.int32) if held is not None else None
        return (s if keep_samples and held is not None else None), lj, acc, st, cor, (lj * 2. if held is not None else None)

    def _chunk_plain(self, normals, log_u, steps, shared):
        return RecordingMany.chunk(self, normals, log_u, steps, shared)

    def _chunk_scored_plain(self, normals, log_u, steps, shared, held, keep_samples):
        return RecordingMany.chunk_scored(self, normals, log_u, steps, shared, held, keep_samples)

    def summary_end(self):
        self.calls.append(('summary_end',))
        x = np.concatenate(self.kept, axis=1)                  # P x n x C x D, the kept chunks in the order they were folded
        each = [numpy_summarizer(x[p]) for p in range(self.P)]
        return samplers.ChainSummary(*[np.array([getattr(e, k) for e in each]) for k in ('mean', 'cov', 'rhat', 'ess', 'ess_truncated', 'status')])

    def end(self):
        self.calls.append(('end',))
        return None


def _group(eng, seed=4, n=8, warmup=5, held=None, keep=True, **extra):
    P, c, d = eng.P, 2, 3
    rng = np.random.RandomState(seed)
    draws = samplers._ManyDraws(rng, True, P, c, d, keep=False)
    res = samplers._run_hmc_group(eng, list(range(P)), np.zeros((P, c, d)), np.ones((P, d)), np.full(P, 0.1), draws, c, d, n, 2, warmup, 2, 1.0, 3,
                                  held=held, keep_samples=keep, **extra)
    return res, rng.randn()                                    # (and where the stream stands after the run)


def test_warm_up_is_never_folded_and_kept_chunks_are_folded_in_order():
    for held, keep in ((None, True), (None, False), (object(), True), (object(), False)):
        eng, sums = RecordingMany(3), {}
        (res, bad, _), pos = _group(eng, held=held, keep=keep, summaries=sums, max_lag=2)
        calls = eng.calls
        assert calls[0] == ('begin', 13) and calls[1] == ('attach', 8, 2) and calls[-2:] == [('summary_end',), ('end',)]
        chunks = [c for c in calls if c[0].startswith('chunk')]
        assert [c[1] for c in chunks] == [2, 2, 1, 3, 3, 2]     # warm-up in chunks of adapt_every, kept ones in chunks of `chunk`
        assert [c[-1] for c in chunks] == [False] * 3 + [True] * 3
        assert not bad and sorted(sums) == [0, 1, 2]
        # the summary is that of the kept iterations, in order: the stream's draws 5 .. 12 (warm-up took the first five)
        rng = np.random.RandomState(4)
        tape = [(rng.randn(k, 2, 3), rng.rand(k, 2))[0] for k in (2, 2, 1, 3, 3, 2)]
        kept = np.concatenate(tape[3:])
        for p in range(3):
            want = numpy_summarizer(kept + p)
            assert np.array_equal(sums[p].mean, want.mean) and np.array_equal(sums[p].rhat, want.rhat, equal_nan=True)
            s = res[p][0]
            assert (s is None) == (not keep) and (keep is False or np.array_equal(s, kept + p))
        # the run without the option: the same calls less the summary's, the same results, the same stream position
        plain = RecordingMany(3, with_fold=False)
        (res0, _, _), pos0 = _group(plain, held=held, keep=keep or held is None)
        if keep or held is not None:
            assert [c[:-1] if c[0].startswith('chunk') else c for c in calls if c[0] not in ('attach', 'summary_end')] == \
                [c[:-1] if c[0].startswith('chunk') else c for c in plain.calls]
        assert pos == pos0
        for p in range(3):
            assert np.array_equal(res[p][1], res0[p][1]) and np.array_equal(res[p][2], res0[p][2]) and len(res[p]) == len(res0[p])


def test_summary_off_performs_exactly_the_calls_of_before():
    for held in (None, object()):
        a, b = RecordingMany(2, with_fold=False), RecordingMany(2, with_fold=False)
        _group(a, held=held)
        _group(b, held=held, summaries=None)
        assert a.calls == b.calls and not any(c[0] in ('attach', 'summary_end') for c in a.calls)


def _many(summary, keep=True, score=None, seed=9, **kw):
    Z, groups, held = tv.make()
    probs = [(Z[np.concatenate(groups[:j + 1])], None) for j in range(3)]
    rng = np.random.RandomState(seed)
    res = samplers.logistic_hmc_many(probs, n_samples=8, n_chains=2, warmup=4, adapt_every=2, step_size=0.2, start=np.zeros((2, 3)), rng=rng,
                                     engine=tv.ToyEngine, scorer=tv.numpy_scorer, score=held if score else None, keep_samples=keep,
                                     summary=summary, summarizer=numpy_summarizer if summary else None, **kw)
    return res, rng.randn()


def test_the_route_that_returns_its_samples_is_summarised_from_them():
    (plain, pos0), (full, pos1) = _many(False), _many(True, max_lag=2)
    assert pos0 == pos1
    for a, b in zip(plain, full):
        assert a.summary is None and np.array_equal(a.samples, b.samples) and np.array_equal(a.accept, b.accept)
        want = numpy_summarizer(b.samples, 2)
        assert np.array_equal(b.summary.mean, want.mean) and np.array_equal(b.summary.ess, want.ess, equal_nan=True)
    (lean, pos2), (both, pos3) = _many(True, keep=False), _many(True, keep=False, score=True)
    (scored, _) = _many(False, keep=False, score=True)
    assert pos2 == pos0 and pos3 == pos0
    for a, b, c, s in zip(full, lean, both, scored):
        assert b.samples is None and c.samples is None
        assert np.array_equal(b.summary.cov, numpy_summarizer(a.samples).cov)
        assert np.array_equal(c.correct, s.correct) and np.array_equal(c.test_ll, s.test_ll) and c.accuracy == s.accuracy
    with pytest.raises(ValueError, match='keep_samples=False needs score'):
        _many(False, keep=False)
    with pytest.raises(ValueError, match='at least 4'):
        samplers.logistic_hmc_many([(np.ones((2, 3)), None)], n_samples=3, n_chains=2, start=np.zeros((2, 3)), engine=tv.ToyEngine, summary=True,
                                   summarizer=numpy_summarizer)


def test_logistic_hmc_takes_the_stand_in_summarizer():
    import hmc_cases as hc
    Z, w = hc.make_data(12, 3, 5)

    class Rows:
        shape = Z.shape

    kw = dict(n_samples=6, n_chains=2, start=np.zeros((2, 3)), inv_mass=np.ones(3), engine=lambda z, wts: tv.ToyEngine(Z, wts))
    a = samplers.logistic_hmc(Rows(), w, rng=np.random.RandomState(2), **kw)
    b = samplers.logistic_hmc(Rows(), w, rng=np.random.RandomState(2), summary=True, summarizer=numpy_summarizer, **kw)
    assert a.summary is None and np.array_equal(a.samples, b.samples)
    assert np.array_equal(b.summary.mean, numpy_summarizer(b.samples).mean)


def test_tmc_shapley_fills_its_arrays_and_changes_no_value():
    Z, groups, held = tv.make()
    kw = dict(group_cap=5, engine=tv.ToyEngine, scorer=tv.numpy_scorer, **tv.KW)
    plain = valuation.tmc_shapley(Z, groups, held, 5, 3, rng=np.random.RandomState(11), **kw)
    got = valuation.tmc_shapley(Z, groups, held, 5, 3, rng=np.random.RandomState(11), summary=True, summarizer=numpy_summarizer,
                                perms_per_batch=2, **kw)
    assert plain.max_rhat is None and plain.min_ess is None
    assert got.max_rhat.shape == (5, 3) and got.min_ess.shape == (5, 3) and np.isfinite(got.max_rhat).all() and np.isfinite(got.min_ess).all()
    assert np.array_equal(got.phi, plain.phi) and np.array_equal(got.values, plain.values) and np.array_equal(got.perms, plain.perms)
    assert np.array_equal(got.occurrences, plain.occurrences)
