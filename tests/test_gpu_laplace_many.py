"""The batched Laplace fit on the device (k_laplace_many; include/beta_cores_laplace_small.h; samplers.logistic_laplace_many):
every problem of a batch against the formulas in long double -- the mode and the draw under the bounds of
tests/vi_laplace_cases.py, hdiag and the two factors under the bounds of tests/laplace_many_cases.py --, the bits of the
verified single-problem kernel k_vi_laplace, independence of the batch, the exact cases, per-problem marking, the scores
computed where the draws lie, today's loop of logistic_laplace, and the refusals of the entry point.

The batches of test 1 share one S per call (the call has one): every case of dimension D is drawn with S = 100 normals of a
seeded stream, whatever s its lc.make_case names; S = 1 and S = 5 are drawn in the test against k_vi_laplace."""
import numpy as np
import pytest

import laplace_many_cases as lm
import test_gpu_vi_laplace as tvl
import test_gpu_vi_optimize as tvo
import test_laplace_many_cpu as tcpu
import vi_laplace_cases as lc

pytestmark = pytest.mark.gpu
FIELDS = ('mu', 'LSig', 'LSigInv', 'hdiag', 'value', 'newton', 'halvings', 'halvings_all', 'draws')


@pytest.fixture(scope='module')
def bc():
    import beta_cores_amd as bc
    bc.default_context()
    return bc


def same_fit(a, b, fields=FIELDS):
    return all(np.array_equal(getattr(a, k), getattr(b, k)) for k in fields)


def fit(bc, cases, seed, S, diag=False, **kw):
    """The cases (common D) as one call with S shared normals of RandomState(seed); the cases come back carrying those normals."""
    d = cases[0]['d']
    cs = [lm.with_normals(c, np.random.RandomState(seed).randn(S, d), diag=diag) for c in cases]
    probs, starts = lm.problems_of(cs)
    return cs, bc.samplers.logistic_laplace_many(probs, mu0=starts, diag=diag, n_draws=S, rng=np.random.RandomState(seed), **kw)


# ---------------------------------------------------------------- 1: against long double
@pytest.mark.parametrize('d', [1, 2, 3, 16, 33, 128])
def test_batch_against_long_double(bc, d):
    cases, res = fit(bc, lm.cases_of_dim(d), 40 + d, 100)
    assert len(res) == len(cases) and res.marked == [] and res.device_ms > 0.
    worst = {}
    for c, r in zip(cases, res):
        assert 1 <= r.newton <= 200 and 0 <= r.halvings <= 34 and r.halvings <= r.halvings_all
        rm, rd = lc.check_mode_and_draw(c, r.mu, r.draws, 'device')
        rf = lm.check_factors(c, r.mu, r.hdiag, r.LSigInv, r.LSig, 'device')
        assert np.all(np.triu(r.LSigInv, 1) == 0.) and np.all(np.triu(r.LSig, 1) == 0.)
        for k, v in dict(rf, mode=rm, draw=rd).items():
            worst[k] = max(worst.get(k, 0.), v)
    print('worst error / bound at D = %d: %s' % (d, ', '.join('%s %.3g' % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize('d', [3, 128])
def test_diagonal_batch_against_long_double(bc, d):
    cases, res = fit(bc, lm.cases_of_dim(d), 60 + d, 100, diag=True)
    for c, r in zip(cases, res):
        assert 1 <= r.newton <= 200 and 0 <= r.halvings <= 34
        lc.check_mode_and_draw(c, r.mu, r.draws, 'device, diag')
        lm.check_factors(c, r.mu, r.hdiag, label='device, diag')
        sq = np.sqrt(r.hdiag)
        assert np.array_equal(r.LSig, np.diag(1. / sq)) and np.array_equal(r.LSigInv, np.diag(sq))


# ---------------------------------------------------------------- 2: the bits of the verified kernel
def one_step(bc, c):
    """(vi_last_mode(), vi_last_draw()) after a one-step vi_optimize run on case c: start, weights, rows and normals are the
    case's (tests/test_gpu_vi_laplace.py's one_step, restated)."""
    sampler = bc.samplers.LogisticLaplaceSampler(np.zeros(c['d']), diag=c['diag'], rng=np.random.RandomState(0), solver='newton')
    prj = bc.DeviceProjector(sampler, c['s'], bc.likelihoods.LogisticRegression())
    sampler._rng, sampler._mode = tvo._FixedNormals(c['E']), c['start'].copy()
    assert prj.vi_optimize(tvl.data(bc, c['d'])[1], c['Z'], c['w'], 1, lambda i: 1.) is not None and prj.vi_optimize_calls == 1
    return prj.vi_last_mode(), prj.vi_last_draw()


@pytest.mark.parametrize('d,m,s', [(3, 7, 5), (33, 1, 1), (128, 130, 100)])
def test_same_bits_as_k_vi_laplace(bc, d, m, s):
    c = lc.make_case(d, m, s, variant=d)
    mode, draw = one_step(bc, c)
    r = bc.samplers.logistic_laplace_many([(c['Z'], c['w'])], mu0=c['start'], n_draws=s, rng=tvo._FixedNormals(c['E']))[0]
    assert np.array_equal(r.mu, mode['mode']) and np.array_equal(r.draws, draw['theta'])
    assert (r.newton, r.halvings) == (mode['newton'], mode['halvings'])


# ---------------------------------------------------------------- 3: batch independence
def test_a_problems_bits_do_not_depend_on_its_batch(bc):
    cases = [lc.make_case(33, m, 3, variant=m) for m in (1, 7, 64, 65, 300)]
    _, fwd = fit(bc, cases, 3, 3)
    _, rev = fit(bc, cases[::-1], 3, 3)
    _, again = fit(bc, cases, 3, 3)
    for p in range(5):
        _, alone = fit(bc, cases[p:p + 1], 3, 3)
        assert same_fit(fwd[p], rev[4 - p]) and same_fit(fwd[p], alone[0]) and same_fit(fwd[p], again[p]), p
    assert not np.array_equal(fwd[0].mu, fwd[1].mu)


# ---------------------------------------------------------------- 4: exact cases
def test_the_prior_comes_back_exactly(bc):
    d, S = 5, 4
    E = np.random.RandomState(8).randn(S, d)
    Z = lc.make_case(d, 7, S)['Z']
    res = bc.samplers.logistic_laplace_many([(Z, np.zeros(7)), (np.zeros((0, d)), None)], n_draws=S, rng=np.random.RandomState(8))
    for r in res:
        assert np.all(r.mu == 0.) and np.all(r.hdiag == 1.) and r.newton == 0
        assert np.array_equal(r.LSig, np.eye(d)) and np.array_equal(r.LSigInv, np.eye(d)) and np.array_equal(r.draws, E)
        assert abs(r.value + 0.5 * d * np.log(2. * np.pi)) <= np.spacing(0.5 * d * np.log(2. * np.pi))


def test_a_weight_that_is_not_positive_contributes_nothing(bc):
    """Rows with weight 0 or below are the reference's Z[wts > 0]: they enter no sum.  Their places in the sums remain, though:
    the value pass hands rows to lanes by position and the Gram product takes rows four at a time, so removing the rows moves
    the others and the SAME terms are added in another order.  The two fits therefore agree to rounding, not bit for bit: each
    is held to the long-double reference of the problem without those rows, and their modes to lc.mode_bound of each other."""
    d, S = 16, 5
    keep = lc.make_case(d, 130, S, variant=0)
    pos = keep['w'] > 0
    clean = dict(keep, Z=keep['Z'][pos], w=keep['w'][pos], m=int(pos.sum()), key=None)
    del clean['key']
    dirty_w = keep['w'].copy()
    dirty_w[~pos] = np.where(np.arange((~pos).sum()) % 2 == 0, 0., -1.5)
    E = np.random.RandomState(11).randn(S, d)
    res = bc.samplers.logistic_laplace_many([(keep['Z'], dirty_w), (clean['Z'], clean['w'])], n_draws=S, rng=np.random.RandomState(11))
    clean = lm.with_normals(clean, E)
    mu_ref = lc.reference_mode(clean).astype(np.float64)
    for r in res:
        lc.check_mode_and_draw(clean, r.mu, r.draws, 'device, rows of no weight')
        lm.check_factors(clean, r.mu, r.hdiag, r.LSigInv, r.LSig, 'device, rows of no weight')
    diff = np.abs(res[0].mu - res[1].mu).max()
    print('with / without the rows of no weight: same bits %s, max |mu - mu\'| %.3e (bound %.3e)'
          % (same_fit(res[0], res[1]), diff, lc.mode_bound(clean, mu_ref)))
    assert diff <= lc.mode_bound(clean, mu_ref)


# ---------------------------------------------------------------- 5: marking
@pytest.mark.parametrize('what', ['weight', 'start'])
def test_a_problem_that_is_not_finite_is_marked_alone(bc, what):
    cases = lm.cases_of_dim(16)
    assert len(cases) == 5
    bad = [dict(c) for c in cases]
    if what == 'weight':
        bad[2]['w'] = bad[2]['w'].copy()
        bad[2]['w'][5] = np.nan
    else:
        bad[2]['start'] = np.full(16, np.inf)
    _, res = fit(bc, bad, 5, 3, strict=False)
    _, rest = fit(bc, cases[:2] + cases[3:], 5, 3)
    assert res[2] is None and res.marked == [2] and len(res) == 5
    for r, ok in zip(res[:2] + res[3:], rest):
        assert same_fit(r, ok)
    with pytest.raises(bc.NumericalPrecisionError, match=r'problem\(s\) 2 '):
        fit(bc, bad, 5, 3)
    _, after = fit(bc, cases, 5, 3)                       # the context serves the next call
    assert after.marked == [] and same_fit(after[0], rest[0])


# ---------------------------------------------------------------- 6: scores where the draws lie
def test_scores_are_those_of_the_scorer_on_the_draws(bc):
    d, S = 16, 7
    rng = np.random.RandomState(21)
    Xt = rng.randn(200, d)
    held = bc.samplers.HeldOut(Xt, np.where(rng.rand(200) < 0.5, 1., -1.))
    probs, starts = lm.problems_of(lm.cases_of_dim(d))
    f = bc.samplers.logistic_laplace_many
    r1 = np.random.RandomState(22)
    res = f(probs, mu0=starts, n_draws=S, rng=r1, score=held)
    after = np.random.RandomState(22)
    after.randn(S, d)
    assert np.array_equal(r1.randn(3), after.randn(3))          # 'shared': one S x D block was drawn
    lean = f(probs, mu0=starts, n_draws=S, rng=np.random.RandomState(22), score=held, keep_draws=False)
    for r, l in zip(res, lean):
        cor, ll = bc.samplers.logistic_score(held, r.draws)
        assert r.correct.shape == (S,) and np.array_equal(r.correct, cor) and np.array_equal(r.test_ll, ll)
        assert r.accuracy == held.accuracy(cor)
        assert l.draws is None and np.array_equal(l.correct, cor) and np.array_equal(l.test_ll, ll) and np.array_equal(l.mu, r.mu)
    r2 = np.random.RandomState(22)
    ind = f(probs, mu0=starts, n_draws=S, rng=r2, draws='independent', score=held)
    after = np.random.RandomState(22)
    blocks = [after.randn(S, d) for _ in probs]
    assert np.array_equal(r2.randn(3), after.randn(3))          # 'independent': P blocks, p = 0 .. P - 1 in order
    for p, r in enumerate(ind):
        alone = f(probs[p:p + 1], mu0=starts[p], n_draws=S, rng=tvo._FixedNormals(blocks[p]))[0]
        assert np.array_equal(r.draws, alone.draws) and np.array_equal(r.mu, res[p].mu)
        cor, ll = bc.samplers.logistic_score(held, r.draws)
        assert np.array_equal(r.correct, cor) and np.array_equal(r.test_ll, ll)
    assert not np.array_equal(ind[1].draws, res[1].draws)


# ---------------------------------------------------------------- 7: against today's loop
def test_modes_agree_with_the_loop_of_logistic_laplace(bc):
    for d in (3, 33):
        cases = lm.cases_of_dim(d)
        for c in cases:
            c['start'] = np.zeros(d)
        probs, _ = lm.problems_of(cases)
        res = bc.samplers.logistic_laplace_many(probs)
        for c, r in zip(cases, res):
            assert r.draws is None
            mu = bc.samplers.logistic_laplace(c['w'], bc.DeviceData(c['Z']), np.zeros(d), solver='newton')[0]
            bound = 2. * lc.mode_bound(c, lc.reference_mode(c).astype(np.float64))      # (both sit within one bound of mu*)
            assert np.abs(r.mu - mu).max() <= bound, (c['key'], np.abs(r.mu - mu).max(), bound)


def test_hmc_many_takes_its_fits_from_one_batched_call(bc):
    d, c = 16, 4
    probs = [(cs['Z'], cs['w']) for cs in (lc.make_case(d, m, 1, variant=0) for m in (1, 7, 130))]
    kw = dict(n_samples=5, n_chains=c, step_size=0.01, n_leapfrog=3, warmup=4, adapt_every=2)
    f = bc.samplers.logistic_hmc_many
    got = f(probs, start=None, inv_mass='laplace', laplace='batched', rng=np.random.RandomState(7), **kw)
    many = bc.samplers.logistic_laplace_many(probs)
    r7 = np.random.RandomState(7)
    e0 = r7.randn(c, d)
    starts = np.array([r.mu + e0.dot(r.LSig.T) for r in many])
    ims = np.array([1. / r.hdiag for r in many])
    explicit = f(probs, start=starts, inv_mass=ims, rng=r7, **kw)
    for p in range(3):
        assert np.array_equal(got[p].start, starts[p]) and np.array_equal(got[p].inv_mass, ims[p])
        assert np.array_equal(got[p].samples, explicit[p].samples) and np.array_equal(got[p].accept, explicit[p].accept)
    each = f(probs, start=None, inv_mass='laplace', laplace='each', rng=np.random.RandomState(7), **kw)
    plain = f(probs, start=None, inv_mass='laplace', rng=np.random.RandomState(7), **kw)
    for p in range(3):
        assert np.array_equal(each[p].samples, plain[p].samples) and np.array_equal(each[p].start, plain[p].start)
        assert np.array_equal(each[p].inv_mass, plain[p].inv_mass)
        assert np.allclose(each[p].start, got[p].start, rtol=1e-6, atol=1e-6)


# ---------------------------------------------------------------- 8: refusals through ctypes
def test_refusals_leave_the_outputs_and_the_context_as_they_were(bc):
    from beta_cores_amd import _native as N
    from beta_cores_amd.device import _ptr
    ctx = bc.default_context()
    c = tcpu._Call()
    c.kw['ctx'] = ctx.h
    rng = np.random.RandomState(31)
    held = bc.samplers.HeldOut(rng.randn(200, 3), np.where(rng.rand(200) < 0.5, 1., -1.))
    cor, ll = np.full((2, 2), 7, dtype=np.int32), np.full((2, 2), 7.)
    assert c.refused(d=129, rows=_ptr(np.ones((3, 129))))
    assert c.refused(s=257)
    assert c.refused(row_ptr=_ptr(np.array([0, 2, 2], dtype=np.int64)))
    assert c.refused(inv=None)                                                         # out_chol without out_inv
    assert c.refused(diag=1)                                                           # factors with the diagonal form
    assert c.refused(zt=held.Z.h, cor=_ptr(cor), ll=_ptr(ll))                          # zt without yt
    assert c.refused(zt=held.Z.h, yt=held.Y.h, cor=_ptr(cor), ll=_ptr(ll), s=0, normals=None, th=None)      # scoring with s = 0
    wide = bc.samplers.HeldOut(rng.randn(200, 4), np.where(rng.rand(200) < 0.5, 1., -1.))
    assert c.refused(zt=wide.Z.h, yt=wide.Y.h, cor=_ptr(cor), ll=_ptr(ll))            # held-out rows of another width
    assert np.all(cor == 7) and np.all(ll == 7.)
    kw = c.kw
    args = [kw[k] for k in ('ctx', 'rows', 'w', 'row_ptr', 'P', 'd', 'start', 'diag', 'normals', 'stride', 's', 'zt', 'yt', 'mu', 'hd', 'val',
                            'cnt', 'st', 'chol', 'inv', 'th', 'cor', 'll')]
    assert N.load().bc_laplace_small(*args) == N.BC_OK and np.all(c.st == 0) and np.all(c.cnt[:, 0] >= 1)      # still usable
    ref = bc.samplers.logistic_laplace_many([(np.ones((1, 3)), None), (np.ones((2, 3)), None)], n_draws=2, rng=tvo._FixedNormals(np.ones((2, 3))))
    assert np.array_equal(c.mu, np.array([r.mu for r in ref])) and np.array_equal(c.th, np.array([r.draws for r in ref]))
