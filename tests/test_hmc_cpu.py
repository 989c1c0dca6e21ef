"""The multi-chain HMC sampler without a GPU: the host build of csrc/bc_hmc_dev.h (tests/hmc_harness.cpp) against the
long-double restatement of tests/hmc_cases.py, and samplers.logistic_hmc's host logic -- the warm-up rule, the chunking, the
order of the draws and the argument checks -- through a stand-in engine."""
import numpy as np
import pytest

import hmc_cases as hc
from beta_cores_amd import samplers


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    return hc.build_harness(tmp_path_factory.mktemp('hmc_harness'))


@pytest.mark.parametrize('name', ['small', 'wide'])
def test_host_build_follows_the_long_double_restatement(harness, tmp_path, name):
    """One run whose trajectories end in accepted and in rejected proposals: positions and log-joints within 64 x the float64
    restatement's own deviation (floor 1e-13, relative), the decisions equal, a rejected chain's bits unchanged."""
    case = hc.make_trace_case(name)
    ref, tol_s, tol_l = hc.trace_tolerance(case)
    hc.check_trace_condition(ref)
    got = hc.run_harness(harness, case, tmp_path)
    assert got['status'] == 0
    assert np.array_equal(got['accept'], ref['accept'])
    ds, dl = hc.rel_dev(got['samples'], ref['samples']), hc.rel_dev(got['logjoint'], ref['logjoint'])
    print('%s: samples %.3g (tol %.3g), logjoint %.3g (tol %.3g)' % (name, ds, tol_s, dl, tol_l))
    assert ds <= tol_s and dl <= tol_l
    prev_s, prev_l = np.vstack((case['start'][None], got['samples'][:-1])), got['logjoint'][:-1]
    rej = ~got['accept']
    assert np.array_equal(got['samples'][rej], prev_s[rej])
    assert np.array_equal(got['logjoint'][1:][rej[1:]], prev_l[rej[1:]])


def test_host_build_rejects_everything_at_a_huge_step_and_flags_a_bad_weight(harness, tmp_path):
    case = hc.make_trace_case('small')
    case['eps'] = 1e6
    got = hc.run_harness(harness, case, tmp_path)
    assert got['status'] == 0 and not got['accept'].any()
    assert np.array_equal(got['samples'], np.broadcast_to(case['start'], got['samples'].shape))
    case = hc.make_trace_case('small')
    case['w'][3] = np.nan
    assert hc.run_harness(harness, case, tmp_path)['status'] == 1


# ------------------------------------------------------------------ samplers.logistic_hmc through the stand-in engine
class _Rows:
    """Stands in for a DeviceData: a shape, a context, and the rows for the stand-in engine."""

    def __init__(self, Z, ctx='ctx-a'):
        self._z, self.shape, self.ctx = Z, Z.shape, ctx

    def __array__(self, dtype=None, copy=None):
        return self._z if dtype is None else self._z.astype(dtype)


def _problem(n=60, d=3, c=4, seed=5):
    Z, w = hc.make_data(n, d, seed)
    rng = np.random.RandomState(seed)
    return _Rows(Z), w, rng.randn(c, d) * 0.1, 0.5 + rng.rand(d)


def test_warmup_rule_and_chunking():
    """Warm-up in chunks of adapt_every (the last one shorter), step <- step * exp(rate (acc - 0.8)) after each with acc the
    accepted fraction of that chunk; the step frozen afterwards; the kept iterations chunked as asked; warm-up discarded."""
    rows, w, start, im = _problem()
    fractions = [1.0, 0.5, 0.0, 0.9, 0.9, 0.9]
    engines = []

    def engine(Z, wts):
        engines.append(hc.NumpyHMCEngine(Z, wts, forced_accept=fractions))
        return engines[-1]
    res = samplers.logistic_hmc(rows, w, n_samples=9, n_chains=4, step_size=0.05, n_leapfrog=3, inv_mass=im, start=start, warmup=25,
                                rng=np.random.RandomState(1), adapt_every=10, adapt_rate=1.5, chunk=4, engine=engine)
    eng = engines[0]
    assert eng.ended and eng.n_iter == 34
    assert eng.sizes == [10, 10, 5, 4, 4, 1]
    want, step = [], 0.05
    for i in range(3):
        want.append(step)
        acc = np.mean(np.random.RandomState(i + 1).rand(eng.sizes[i], 4) < fractions[i])
        step = step * float(np.exp(1.5 * (acc - 0.8)))
    assert eng.steps[:3] == want and eng.steps[3:] == [step] * 3 and res.step_size == step
    assert np.array_equal(res.warmup_steps, np.array(want))
    assert want[1] > want[0] and want[3 - 1] < want[1]          # all accepted: longer; half accepted: shorter
    assert res.samples.shape == (9, 4, 3) and res.logjoint.shape == (9, 4) and res.accept_rate.shape == (4,)
    assert samplers.hmc_warmup_step(0.2, 0.8) == 0.2 and samplers.hmc_warmup_step(0.2, 1.0, rate=2.) == 0.2 * float(np.exp(2. * (1.0 - 0.8)))


def test_draw_order_and_result_against_the_restatement():
    """Per chunk randn(k, C, D) then log(rand(k, C)), from the given stream; without warm-up the samples are hmc_run's."""
    rows, w, start, im = _problem()
    res = samplers.logistic_hmc(rows, w, n_samples=5, n_chains=4, step_size=0.07, n_leapfrog=2, inv_mass=im, start=start,
                                rng=np.random.RandomState(3), chunk=3, engine=hc.NumpyHMCEngine)
    rng = np.random.RandomState(3)
    e1, u1 = rng.randn(3, 4, 3), np.log(rng.rand(3, 4))
    e2, u2 = rng.randn(2, 4, 3), np.log(rng.rand(2, 4))
    ref = hc.hmc_run(np.asarray(rows), w, start, im, 0.07, 2, np.concatenate((e1, e2)), np.concatenate((u1, u2)), dtype=np.float64)
    assert np.array_equal(res.samples, ref['samples']) and np.array_equal(res.logjoint, ref['logjoint'])
    assert np.array_equal(res.accept, ref['accept']) and np.array_equal(res.accept_rate, ref['accept'].mean(axis=0))
    assert res.pooled().shape == (20, 3) and res.step_size == 0.07 and res.warmup_steps.size == 0


class _Comm:
    world = 2


def test_argument_checks():
    rows, w, start, im = _problem()
    kw = dict(n_samples=2, n_chains=4, inv_mass=im, start=start, engine=hc.NumpyHMCEngine)

    def run(Z=rows, wts=w, **over):
        a = dict(kw)
        a.update(over)
        return samplers.logistic_hmc(Z, wts, **a)
    run()
    for bad in (0, 65):
        with pytest.raises(ValueError, match='chains'):
            run(n_chains=bad, start=np.zeros((bad, 3)))
    wide = _Rows(np.zeros((4, 257)))
    with pytest.raises(ValueError, match='256'):
        run(Z=wide, wts=None, start=np.zeros((4, 257)), inv_mass=np.ones(257))
    with pytest.raises(NotImplementedError):
        run(comm=_Comm())
    with pytest.raises(ValueError, match='context'):
        run(ctx='ctx-b')
    run(ctx='ctx-a')
    with pytest.raises(ValueError, match='start'):
        run(start=start[:3])
    with pytest.raises(ValueError, match='start'):
        run(start=start[:, :2])
    with pytest.raises(ValueError, match='wts'):
        run(wts=w[:-1])
    with pytest.raises(ValueError, match='inv_mass'):
        run(inv_mass=im[:-1])
    with pytest.raises(ValueError, match='inv_mass'):
        run(inv_mass=im * 0.)
    with pytest.raises(ValueError, match='inv_mass'):
        run(inv_mass='stan')
    with pytest.raises(ValueError, match='step_size'):
        run(step_size=0.)
    with pytest.raises(ValueError, match='step_size'):
        run(step_size=np.inf)
    with pytest.raises(ValueError):
        run(n_samples=0)
    with pytest.raises(ValueError):
        run(n_leapfrog=0)
    with pytest.raises(ValueError, match='Laplace'):
        run(start=None)
    with pytest.raises(ValueError, match='Laplace'):
        run(inv_mass='laplace')
