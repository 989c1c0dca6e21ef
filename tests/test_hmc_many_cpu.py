"""The batched small-problem HMC run without a GPU: the host build of csrc/bc_hmc_small_dev.h + csrc/bc_hmc_dev.h
(tests/hmc_small_harness.cpp) on the batch cases of tests/hmc_many_cases.py against the long-double restatement, and
samplers.logistic_hmc_many's host logic -- the shared and the independent draws, the per-problem warm-up, the per-problem
arguments and the argument checks -- through the NumPy stand-in engine of tests/hmc_cases.py."""
import numpy as np
import pytest

import hmc_cases as hc
import hmc_many_cases as mc
from beta_cores_amd import samplers


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    return mc.build_harness(tmp_path_factory.mktemp('hmc_small_harness'))


@pytest.mark.parametrize('name', mc.BATCH_NAMES)
def test_host_build_follows_the_long_double_restatement(harness, tmp_path, name):
    """Every problem of the batch: decisions equal, positions and log-joints within hc.trace_tolerance of that problem, a
    rejected chain's bits unchanged.  The conditions on the inputs are asserted on the restatement."""
    case, refs = mc.make_batch_case(name), mc.batch_reference(name)
    mc.check_batch_condition(refs)
    got = mc.run_harness(harness, case['problems'], tmp_path)
    for pr, g, (ref, tol_s, tol_l) in zip(case['problems'], got, refs):
        assert g['status'] == 0
        mc.compare_with_reference(g, ref, tol_s, tol_l, pr['start'], pr['name'])


def test_the_table_of_the_batch_cases_holds():
    """The accepted counts the cases were chosen for (float64 restatement = long-double restatement: asserted by trace_tolerance)."""
    want = dict(ragged5=(56, 90), wide128=(228, 256), d256=(15, 16), d1=(6, 12), pack128=(43, 48))
    for name in mc.BATCH_NAMES:
        acc = np.concatenate([ref['accept'].ravel() for ref, _, _ in mc.batch_reference(name)])
        assert (int(acc.sum()), acc.size) == want[name], (name, acc.sum(), acc.size)
    d1 = mc.batch_reference('d1')
    assert d1[0][0]['accept'].all() and not d1[1][0]['accept'].any()      # one accepts everything beside one that rejects everything


def test_host_build_marks_one_problem_only_and_rejects_at_a_huge_step(harness, tmp_path):
    case = mc.make_batch_case('ragged5')
    probs = [dict(pr) for pr in case['problems'][:3]]
    clean = mc.run_harness(harness, probs, tmp_path)
    probs[1]['start'] = probs[1]['start'].copy()
    probs[1]['start'][2, 0] = np.inf
    probs[2]['eps'] = 1e6
    got = mc.run_harness(harness, probs, tmp_path)
    assert [g['status'] for g in got] == [0, 1, 0]
    assert not got[1]['samples'].any() and not got[1]['accept'].any()
    assert np.array_equal(got[0]['samples'], clean[0]['samples']) and np.array_equal(got[0]['logjoint'], clean[0]['logjoint'])
    assert not got[2]['accept'].any() and np.array_equal(got[2]['samples'], np.broadcast_to(probs[2]['start'], got[2]['samples'].shape))


# ------------------------------------------------------------------ samplers.logistic_hmc_many through the stand-in engine
class _Rows:
    """Stands in for a DeviceData in logistic_hmc: a shape, a context, and the rows for the stand-in engine."""

    def __init__(self, Z):
        self._z, self.shape, self.ctx = Z, Z.shape, None

    def __array__(self, dtype=None, copy=None):
        return self._z if dtype is None else self._z.astype(dtype)


def _problems(ns=(12, 1, 40, 7), d=3, seed=31):
    return [hc.make_data(n, d, seed + p) for p, n in enumerate(ns)]


class _Recording:
    """An engine factory that keeps the engines it made, in order."""

    def __init__(self):
        self.made = []

    def __call__(self, Z, wts):
        self.made.append(hc.NumpyHMCEngine(Z, wts))
        return self.made[-1]


def test_shared_draws_equal_the_equally_seeded_loop():
    """draws='shared': entry p is logistic_hmc(Z_p, wts_p, ..., rng=RandomState(seed)) EXACTLY on the stand-in engine -- samples,
    log-joints, decisions, the warm-up steps (which diverge per problem), the frozen step and the chunk sizes."""
    probs = _problems()
    rng = np.random.RandomState(4)
    start, im = rng.randn(4, 3) * 0.1, 0.5 + rng.rand(3)
    kw = dict(n_samples=9, n_chains=4, step_size=0.4, n_leapfrog=3, inv_mass=im, start=start, warmup=11, adapt_every=4, adapt_rate=1.5)
    for chunk in (None, 4):
        rec_many, rec_one = _Recording(), _Recording()
        many = samplers.logistic_hmc_many(probs, rng=np.random.RandomState(9), engine=rec_many, chunk=chunk, **kw)
        assert isinstance(many, list) and len(many) == len(probs) and many.fallback == [] and many.marked == []
        for p, (Z, w) in enumerate(probs):
            one = samplers.logistic_hmc(_Rows(Z), w, rng=np.random.RandomState(9), engine=rec_one, chunk=chunk, **kw)
            r = many[p]
            assert np.array_equal(r.samples, one.samples) and np.array_equal(r.logjoint, one.logjoint) and np.array_equal(r.accept, one.accept)
            assert r.step_size == one.step_size and np.array_equal(r.warmup_steps, one.warmup_steps) and r.warmup_steps.shape == (3,)
            assert np.array_equal(r.start, one.start) and np.array_equal(r.inv_mass, one.inv_mass) and r.route == 'small'
            assert rec_many.made[p].sizes == rec_one.made[p].sizes and rec_many.made[p].steps == rec_one.made[p].steps
            assert rec_many.made[p].ended and rec_many.made[p].n_iter == 20
        assert rec_many.made[0].sizes == ([4, 4, 3, 7, 2] if chunk is None else [4, 4, 3, 4, 4, 1])
        steps = [r.step_size for r in many]
        assert len(set(steps)) > 1                                       # the steps diverged per problem


def test_independent_draws_consume_the_stream_in_the_documented_order():
    """draws='independent': per chunk, for p = 0 .. P - 1 in order, randn(k, C, D) then log(rand(k, C)); the automatic chunk is
    the engine's divided by P."""
    probs = _problems(ns=(5, 9, 3))
    rng = np.random.RandomState(4)
    start, im = rng.randn(2, 3) * 0.1, 0.5 + rng.rand(3)
    rec = _Recording()
    many = samplers.logistic_hmc_many(probs, n_samples=5, n_chains=2, step_size=0.2, n_leapfrog=2, inv_mass=im, start=start,
                                      rng=np.random.RandomState(6), draws='independent', engine=rec)
    assert rec.made[0].sizes == [2, 2, 1]                                # 7 // 3 = 2 iterations per chunk
    r = np.random.RandomState(6)
    E, U = [[] for _ in probs], [[] for _ in probs]
    for k in (2, 2, 1):
        for p in range(3):
            E[p].append(r.randn(k, 2, 3))
            U[p].append(np.log(r.rand(k, 2)))
    for p, (Z, w) in enumerate(probs):
        ref = hc.hmc_run(Z, w, start, im, 0.2, 2, np.concatenate(E[p]), np.concatenate(U[p]), dtype=np.float64)
        assert np.array_equal(many[p].samples, ref['samples']) and np.array_equal(many[p].accept, ref['accept'])
    assert not np.array_equal(many[0].samples[:, :, 0], many[1].samples[:, :, 0])


def test_per_problem_arguments_and_the_empty_coreset():
    probs = _problems(ns=(6, 10))
    probs.append((np.zeros((0, 3)), None))                               # an empty coreset: one zero row with weight 0, the prior
    probs.append((probs[0][0].astype(np.float32), None))                 # float32 rows are widened; wts None = all ones
    P = len(probs)
    rng = np.random.RandomState(8)
    starts, ims, steps = rng.randn(P, 2, 3) * 0.1, 0.5 + rng.rand(P, 3), 0.1 * (1. + np.arange(P))
    rec = _Recording()
    many = samplers.logistic_hmc_many(probs, n_samples=4, n_chains=2, step_size=steps, n_leapfrog=2, inv_mass=ims, start=starts,
                                      rng=np.random.RandomState(2), engine=rec)
    assert rec.made[2].Z.shape == (1, 3) and not rec.made[2].Z.any() and np.array_equal(rec.made[2].w, np.zeros(1))
    assert rec.made[3].Z.dtype == np.float64 and np.array_equal(rec.made[3].Z, probs[3][0].astype(np.float64)) and np.array_equal(rec.made[3].w, np.ones(6))
    r = np.random.RandomState(2)
    E, U = r.randn(4, 2, 3), np.log(r.rand(4, 2))
    for p in range(P):
        assert rec.made[p].steps == [steps[p]] and np.array_equal(many[p].start, starts[p]) and np.array_equal(many[p].inv_mass, ims[p])
        ref = hc.hmc_run(rec.made[p].Z, rec.made[p].w, starts[p], ims[p], steps[p], 2, E, U, dtype=np.float64)
        assert np.array_equal(many[p].samples, ref['samples'])
    # the prior alone: the one zero row has weight 0 and adds nothing, the log-joint is -D/2 log 2 pi - |theta|^2 / 2
    th = many[2].samples[-1]
    assert np.allclose(many[2].logjoint[-1], -1.5 * np.log(2. * np.pi) - 0.5 * (th * th).sum(axis=1), rtol=1e-13)


def test_argument_checks():
    probs = _problems(ns=(6, 10))
    rng = np.random.RandomState(8)
    start, im = rng.randn(2, 3) * 0.1, 0.5 + rng.rand(3)
    kw = dict(n_samples=2, n_chains=2, inv_mass=im, start=start, engine=hc.NumpyHMCEngine)

    def run(pr=probs, **over):
        a = dict(kw)
        a.update(over)
        return samplers.logistic_hmc_many(pr, **a)
    assert len(run()) == 2
    with pytest.raises(ValueError, match='draws'):
        run(draws='common')
    with pytest.raises(ValueError, match='at least one'):
        run(pr=[])
    with pytest.raises(ValueError, match='columns'):
        run(pr=[probs[0], (np.zeros((4, 2)), None)])
    with pytest.raises(ValueError, match='n x D'):
        run(pr=[(np.zeros(3), None)])
    with pytest.raises(ValueError, match='wts'):
        run(pr=[(probs[0][0], probs[0][1][:-1])])
    for bad in (0, 65):
        with pytest.raises(ValueError, match='chains'):
            run(n_chains=bad, start=np.zeros((bad, 3)))
    with pytest.raises(ValueError, match='256'):
        run(pr=[(np.zeros((4, 257)), None)], start=np.zeros((2, 257)), inv_mass=np.ones(257))
    with pytest.raises(ValueError, match='start'):
        run(start=start[:1])
    with pytest.raises(ValueError, match='start'):
        run(start=np.zeros((3, 2, 3)))                                    # neither C x D nor P x C x D
    with pytest.raises(ValueError, match='inv_mass'):
        run(inv_mass=np.ones((3, 3)))
    with pytest.raises(ValueError, match='inv_mass'):
        run(inv_mass=im * 0.)
    with pytest.raises(ValueError, match='inv_mass'):
        run(inv_mass='stan')
    with pytest.raises(ValueError, match='step_size'):
        run(step_size=[0.1, 0.2, 0.3])
    with pytest.raises(ValueError, match='step_size'):
        run(step_size=[0.1, 0.])
    with pytest.raises(ValueError, match='step_size'):
        run(step_size=np.inf)
    with pytest.raises(ValueError):
        run(n_samples=0)
    with pytest.raises(ValueError):
        run(n_leapfrog=0)
    with pytest.raises(ValueError, match='chunk'):
        run(chunk=0)
    with pytest.raises(ValueError, match='Laplace'):
        run(start=None)
    with pytest.raises(ValueError, match='Laplace'):
        run(inv_mass='laplace')


def test_the_restatement_stays_inside_the_statistical_guard():
    """The condition of the GPU suite's statistical guard, on the stand-in engine: with the problems, the seed, the step and the
    start rule the GPU test uses (start = mode + randn(C, D) . LSig^T, mass from the Laplace diagonal), the float64 restatement
    itself is inside the bars, with either kind of draws -- 0.12 sd and 0.92 .. 1.07 with shared draws against 0.25 sd and
    [0.8, 1.25]."""
    g = mc.GUARD
    probs, fits = mc.guard_problems()
    ims = []
    for (Z, w), (mode, _, _) in zip(probs, fits):
        m = -Z.dot(mode)
        p = 0.5 * (1. + np.tanh(0.5 * m))
        ims.append(1. / (1. + ((w * p * (1. - p))[:, None] * Z * Z).sum(axis=0)))
    for draws in ('shared', 'independent'):
        rng = np.random.RandomState(g['rng_seed'])
        if draws == 'shared':
            e0 = rng.randn(g['c'], g['d'])
            starts = np.array([mode + e0.dot(LSig.T) for mode, _, LSig in fits])
        else:
            starts = np.array([mode + rng.randn(g['c'], g['d']).dot(LSig.T) for mode, _, LSig in fits])
        res = samplers.logistic_hmc_many(probs, n_samples=g['n_samples'], n_chains=g['c'], step_size=g['step'], n_leapfrog=g['L'],
                                         inv_mass=np.array(ims), start=starts, rng=rng, draws=draws, engine=hc.NumpyHMCEngine)
        mc.check_guard(res, fits, 'restatement, %s draws' % draws)
