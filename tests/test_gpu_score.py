"""The held-out scorer (k_lr_score, include/beta_cores_score.h) and what is built on it, on the GPU.

1. samplers.logistic_score against the long-double restatement of tests/score_cases.py on every case of its table: counts equal
   (under the input condition, asserted here on the CPU), ll within the derived tolerance; float32 rows give the bits of the same
   values stored as float64.
2. Batch independence, bit for bit.
3. In-run scoring of logistic_hmc_many on two batch shapes of tests/hmc_many_cases.py, and the chunk protocol of the C ABI.
4. The fallback route.
5. valuation.tmc_shapley end to end against a host loop.
"""
import ctypes

import numpy as np
import pytest

import hmc_cases as hc
import hmc_many_cases as mc
import score_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def bc():
    import beta_cores_amd as bc
    bc.default_context()
    return bc


def _p(x):
    return None if x is None else x.ctypes.data_as(ctypes.c_void_p)


def _held_of(bc, case):
    return bc.samplers.HeldOut(case['X'], case['Y'], dtype=np.float32 if case['f32'] else None)


# ------------------------------------------------------------------ 1. the stand-alone scorer against the restatement
@pytest.mark.skipif(not sc.LONGDOUBLE_OK, reason='np.longdouble is no wider than float64 on this platform')
@pytest.mark.parametrize('name', sc.NAMES)
def test_scorer_follows_the_restatement(bc, name):
    case, ref = sc.make_case(name), sc.reference(name)
    sc.check_condition(ref)                                         # (on the CPU: rounding cannot flip a prediction)
    cor, ll = bc.samplers.logistic_score(_held_of(bc, case), case['thetas'])
    assert cor.shape == ll.shape == (case['thetas'].shape[0],)
    sc.compare(cor, ll, ref, 'device ' + name)
    if case['f32']:
        wide = bc.samplers.HeldOut(case['X'].astype(np.float64), case['Y'])
        cor64, ll64 = bc.samplers.logistic_score(wide, case['thetas'])
        assert np.array_equal(cor64, cor) and np.array_equal(ll64, ll)


def test_scorer_refusals(bc):
    from beta_cores_amd import _native as N
    case = sc.make_case('n17_d5_t17')
    held = _held_of(bc, case)
    th = case['thetas'].copy()
    with pytest.raises(ValueError, match='T x 5'):
        bc.samplers.logistic_score(held, th[:, :4])
    th[3, 2] = np.nan
    with pytest.raises(ValueError, match=r'theta\[3\]\[2\]'):
        bc.samplers.logistic_score(held, th)
    lib, h = N.load(), bc.default_context().h
    cor, ll = np.zeros(17, dtype=np.int32), np.zeros(17)
    good = np.ascontiguousarray(case['thetas'])
    assert lib.bc_lr_score(h, held.Z.h, held.Y.h, _p(good), 0, _p(cor), _p(ll)) == N.BC_INVALID_ARGUMENT          # T = 0
    assert lib.bc_lr_score(h, held.Z.h, held.Z.h, _p(good), 17, _p(cor), _p(ll)) == N.BC_INVALID_ARGUMENT         # labels of the wrong shape
    assert lib.bc_lr_score(h, held.Z.h, held.Y.h, _p(good), 17, None, _p(ll)) == N.BC_INVALID_ARGUMENT
    assert lib.bc_score_chunk(h, held.Z.h, held.Y.h) == N.BC_INVALID_ARGUMENT and 'pending' in N.last_error()       # no run is open
    assert lib.bc_lr_score(h, held.Z.h, held.Y.h, _p(good), 17, _p(cor), _p(ll)) == N.BC_OK
    assert np.array_equal(cor, bc.samplers.logistic_score(held, good)[0])


# ------------------------------------------------------------------ 2. batch independence
def test_a_thetas_bits_do_not_depend_on_its_batch(bc):
    case = sc.make_case('n300_d129_t1025')
    held, th = _held_of(bc, case), case['thetas']
    cor, ll = bc.samplers.logistic_score(held, th)
    for t in (0, 2, 517, 1024):
        for batch, at in ((th[t:t + 1], 0), (np.vstack((th[t:t + 1], th[:40])), 0), (np.vstack((th[:40], th[t:t + 1])), 40),
                          (np.vstack((th[100:230], th[t:t + 1], th[:7])), 130)):
            c1, l1 = bc.samplers.logistic_score(held, batch)
            assert c1[at] == cor[t] and np.array_equal(l1[at], ll[t]), (t, batch.shape)
    again = bc.samplers.logistic_score(held, th)
    assert np.array_equal(again[0], cor) and np.array_equal(again[1], ll)


# ------------------------------------------------------------------ 3. in-run scoring
def _many_args(case):
    pr = case['problems']
    return dict(problems=[(p['Z'], p['w']) for p in pr], start=np.array([p['start'] for p in pr]), inv_mass=np.array([p['inv_mass'] for p in pr]),
                step_size=np.array([p['eps'] for p in pr]), n_chains=case['c'], n_leapfrog=case['L'], n_samples=6, warmup=4, adapt_every=2, chunk=4)


def _held_for(bc, d, nt=37, seed=5):
    rng = np.random.RandomState(seed)
    return bc.samplers.HeldOut(rng.randn(nt, d), np.where(rng.rand(nt) < 0.5, 1., -1.))


@pytest.mark.parametrize('name', ['ragged5', 'pack128'])
def test_in_run_scores_are_the_stand_alone_scorers(bc, name):
    case = mc.make_batch_case(name)
    kw = _many_args(case)
    problems = kw.pop('problems')
    held = _held_for(bc, case['d'])
    plain = bc.samplers.logistic_hmc_many(problems, rng=np.random.RandomState(3), **kw)
    scored = bc.samplers.logistic_hmc_many(problems, rng=np.random.RandomState(3), score=held, **kw)
    lean = bc.samplers.logistic_hmc_many(problems, rng=np.random.RandomState(3), score=held, keep_samples=False, **kw)
    for a, b, c in zip(plain, scored, lean):
        assert a.correct is None and a.test_ll is None and a.accuracy is None
        assert b.route == 'small' and np.array_equal(a.samples, b.samples) and np.array_equal(a.logjoint, b.logjoint)
        assert np.array_equal(a.accept, b.accept) and a.step_size == b.step_size and np.array_equal(a.warmup_steps, b.warmup_steps)
        cor, ll = bc.samplers.logistic_score(held, b.pooled())
        assert b.correct.shape == b.test_ll.shape == b.logjoint.shape
        assert np.array_equal(b.correct.ravel(), cor) and np.array_equal(b.test_ll.ravel(), ll)
        assert b.accuracy == held.accuracy(cor)
        assert c.samples is None and np.array_equal(c.correct, b.correct) and np.array_equal(c.test_ll, b.test_ll) and c.accuracy == b.accuracy
        assert np.array_equal(c.logjoint, b.logjoint) and np.array_equal(c.accept, b.accept) and c.step_size == b.step_size
    # a problem whose start is not finite is marked; the others' scores are unaffected
    bad = dict(kw, start=kw['start'].copy())
    bad['start'][1, 0, 0] = np.inf
    res = bc.samplers.logistic_hmc_many(problems, rng=np.random.RandomState(3), score=held, keep_samples=False, strict=False, **bad)
    assert res.marked == [1] and res[1] is None
    for p, (r, b) in enumerate(zip(res, scored)):
        if p != 1:
            assert np.array_equal(r.correct, b.correct) and np.array_equal(r.test_ll, b.test_ll)


def test_chunk_protocol_of_the_scored_end(bc):
    from beta_cores_amd import _native as N
    lib, h = N.load(), bc.default_context().h
    case = mc.make_batch_case('ragged5')
    rows, w, row_ptr, start, im, eps = mc.pack(case['problems'])
    P, c, d = start.shape
    E, U, L, T = np.ascontiguousarray(case['E']), np.ascontiguousarray(case['logU']), case['L'], case['T']
    held, other = _held_for(bc, d), _held_for(bc, d + 1)
    bad = N.BC_INVALID_ARGUMENT

    def outs():
        return (np.full((P, T, c, d), 7.), np.full((P, T, c), 7.), np.full((P, T, c), 7, dtype=np.int32), np.zeros(P, dtype=np.int32),
                np.full((P, T, c), 7, dtype=np.int32), np.full((P, T, c), 7.))
    # run 1: the scored end without a score is refused and leaves the chunk pending; the plain end serves a scored chunk
    assert lib.bc_hmc_small_begin(h, _p(rows), _p(w), _p(row_ptr), P, d, _p(start), c, _p(im), L, T) == 0
    assert lib.bc_score_chunk(h, held.Z.h, held.Y.h) == bad                                                    # no chunk is pending
    assert lib.bc_hmc_small_chunk_begin(h, _p(E), _p(U), 0, T, _p(eps)) == 0
    s, lj, acc, st, cor, ll = outs()
    assert lib.bc_score_chunk_end(h, _p(s), _p(lj), _p(acc), _p(st), _p(cor), _p(ll)) == bad and 'bc_score_chunk' in N.last_error()
    assert lib.bc_score_chunk_end(h, _p(s), _p(lj), _p(acc), _p(st), _p(cor), None) == bad
    assert lib.bc_score_chunk_end(h, _p(s), None, _p(acc), _p(st), None, None) == bad
    assert np.all(s == 7.) and np.all(cor == 7)
    assert lib.bc_score_chunk(h, other.Z.h, other.Y.h) == bad and 'columns' in N.last_error()                  # held-out rows of another width
    th17 = np.zeros((1, d))
    assert lib.bc_lr_score(h, held.Z.h, held.Y.h, _p(th17), 1, _p(cor), _p(ll)) == bad and 'bc_hmc_small' in N.last_error()   # the busy table
    assert lib.bc_score_chunk(h, held.Z.h, held.Y.h) == 0
    assert lib.bc_hmc_small_chunk_end(h, _p(s), _p(lj), _p(acc), _p(st)) == 0                                  # the chunk could still be fetched
    assert lib.bc_hmc_small_end(h) == 0
    assert not st.any() and np.all(s != 7.)
    # run 2: scored, everything fetched
    assert lib.bc_hmc_small_begin(h, _p(rows), _p(w), _p(row_ptr), P, d, _p(start), c, _p(im), L, T) == 0
    assert lib.bc_hmc_small_chunk_begin(h, _p(E), _p(U), 0, T, _p(eps)) == 0
    assert lib.bc_score_chunk(h, held.Z.h, held.Y.h) == 0
    s2, lj2, acc2, st2, cor2, ll2 = outs()
    assert lib.bc_score_chunk_end(h, _p(s2), _p(lj2), _p(acc2), _p(st2), _p(cor2), _p(ll2)) == 0
    assert lib.bc_score_chunk_end(h, _p(s2), _p(lj2), _p(acc2), _p(st2), _p(cor2), _p(ll2)) == bad             # nothing is pending any more
    assert lib.bc_hmc_small_end(h) == 0
    assert np.array_equal(s2, s) and np.array_equal(lj2, lj) and np.array_equal(acc2, acc) and not st2.any()
    want_c, want_l = bc.samplers.logistic_score(held, s.reshape(-1, d))
    assert np.array_equal(cor2.ravel(), want_c) and np.array_equal(ll2.ravel(), want_l)
    # run 3: no samples, and a warm-up end that fetches neither samples nor scores
    assert lib.bc_hmc_small_begin(h, _p(rows), _p(w), _p(row_ptr), P, d, _p(start), c, _p(im), L, T) == 0
    assert lib.bc_hmc_small_chunk_begin(h, _p(E[:2]), _p(U[:2]), 0, 2, _p(eps)) == 0
    _, lj3, acc3, st3, _, _ = outs()
    assert lib.bc_score_chunk_end(h, None, _p(lj3[:, :2].copy()), _p(acc3), _p(st3), None, None) == 0
    assert lib.bc_hmc_small_chunk_begin(h, _p(E[2:]), _p(U[2:]), 0, T - 2, _p(eps)) == 0
    assert lib.bc_score_chunk(h, held.Z.h, held.Y.h) == 0
    k = T - 2
    lj4, acc4, cor4, ll4 = np.zeros((P, k, c)), np.zeros((P, k, c), dtype=np.int32), np.zeros((P, k, c), dtype=np.int32), np.zeros((P, k, c))
    assert lib.bc_score_chunk_end(h, None, _p(lj4), _p(acc4), _p(st3), _p(cor4), _p(ll4)) == 0
    assert lib.bc_hmc_small_end(h) == 0
    assert np.array_equal(lj4, lj[:, 2:]) and np.array_equal(acc4, acc[:, 2:])
    assert np.array_equal(cor4, cor2[:, 2:]) and np.array_equal(ll4, ll2[:, 2:])


# ------------------------------------------------------------------ 4. the fallback route
def test_fallback_route_is_scored_by_the_stand_alone_call(bc):
    d, c = 128, 2
    problems = [hc.make_data(n, d, 80 + i) for i, n in enumerate((10, 145, 60))]
    held = _held_for(bc, d, nt=21)
    rng = np.random.RandomState(12)
    kw = dict(n_samples=3, n_chains=c, n_leapfrog=2, step_size=0.02, start=rng.randn(c, d) * 0.05)
    res = bc.samplers.logistic_hmc_many(problems, rng=np.random.RandomState(4), score=held, **kw)
    assert res.fallback == [1] and [r.route for r in res] == ['small', 'single', 'small']
    lean = bc.samplers.logistic_hmc_many(problems, rng=np.random.RandomState(4), score=held, keep_samples=False, **kw)
    for r, l in zip(res, lean):
        cor, ll = bc.samplers.logistic_score(held, r.pooled())
        assert np.array_equal(r.correct.ravel(), cor) and np.array_equal(r.test_ll.ravel(), ll) and r.accuracy == held.accuracy(cor)
        assert l.samples is None and np.array_equal(l.correct, r.correct) and np.array_equal(l.test_ll, r.test_ll)


# ------------------------------------------------------------------ 5. tmc_shapley end to end
def test_tmc_shapley_against_a_host_loop(bc):
    rng = np.random.RandomState(31)
    sizes, d = (3, 8, 5, 4, 7), 3
    n = sum(sizes)
    X = np.hstack((rng.randn(n, d - 1), np.ones((n, 1))))
    Y = np.where(X[:, 0] - 0.5 * X[:, 1] + 0.5 * rng.randn(n) > 0, 1., -1.)
    Z = Y[:, None] * X
    bounds = np.concatenate(([0], np.cumsum(sizes)))
    order = rng.permutation(n)
    groups = [order[bounds[g]:bounds[g + 1]] for g in range(5)]
    Xt = np.hstack((rng.randn(50, d - 1), np.ones((50, 1))))
    Yt = np.where(Xt[:, 0] - 0.5 * Xt[:, 1] > 0, 1., -1.)
    held = bc.samplers.HeldOut(Xt, Yt)
    T, mg, cap = 4, 3, 6
    kw = dict(n_samples=8, n_chains=2, warmup=6, adapt_every=3, step_size=0.3, n_leapfrog=4)
    got = bc.valuation.tmc_shapley(Z, groups, held, T, mg, group_cap=cap, rng=np.random.RandomState(17), **kw)
    # the host loop: the documented draw order, logistic_hmc_many without a score, NumPy scoring of the returned samples
    r = np.random.RandomState(17)
    hseed = r.randint(2 ** 31 - 1)
    problems, perms = [], []
    for _ in range(T):
        idcs = r.permutation(5)
        perms.append(idcs)
        for j in range(mg):
            rows = [groups[i] if len(groups[i]) < cap else r.choice(groups[i], cap, replace=False) for i in idcs[:j + 1]]
            problems.append((Z[np.concatenate(rows)], None))
    res = bc.samplers.logistic_hmc_many(problems, rng=np.random.RandomState(hseed), draws='shared', start=np.zeros((2, d)), **kw)
    Zt = Yt[:, None] * Xt
    values = np.full((T, mg + 1), 0.5)
    for i, rr in enumerate(res):
        s = Zt.astype(np.longdouble).dot(rr.pooled().astype(np.longdouble).T)
        assert np.abs(s).min() >= sc.MIN_MARGIN                     # the input condition: the counts cannot differ by rounding
        cor = (((Yt[:, None] > 0) & (s >= 0)) | ((Yt[:, None] < 0) & (s > 0))).sum(axis=0)
        values[i // mg, 1 + i % mg] = cor.sum() / (cor.size * Zt.shape[0])
    assert np.array_equal(got.perms, np.array(perms)) and got.n_fallback == 0
    assert np.array_equal(got.values, values)
    phi, occ = np.zeros(5), np.zeros(5)
    for t in range(T):
        for j in range(mg):
            phi[perms[t][j]] += values[t, j + 1] - values[t, j]
            occ[perms[t][j]] += 1
    assert np.array_equal(got.occurrences, occ) and np.array_equal(got.phi, np.divide(phi, occ, out=np.zeros(5), where=occ != 0))
