"""The per-chain warm-up of the batched small-problem HMC run on the device (include/beta_cores_hmc_adapt.h, k_hmc_small<CPB, 1>):

1. The device against the long-double restatement on every case of tests/hmc_adapt_cases.py, by the rule and under the condition of
   tests/test_hmc_adapt_cpu.py, and both sharp checks on the device's own alphas and samples.
2. Bit for bit: the warm-up in chunks cut at the window ends against chunks of 7; 1, 2 and 4 chains per block; a problem alone
   against the same problem inside a batch.
3. With one chain: the kept chunk after the warm-up is, bit for bit, an ordinary run begun from the adapted position, step and mass.
4. score=, keep_samples=False and summary=True under adapt='stan' carry the bits of the stand-alone scorer and summary.
5. A marked problem stays local; the refusals.
6. One statistical guard.
"""
import contextlib
import ctypes
import functools
import os

import numpy as np
import pytest

import hmc_adapt_cases as ac
import hmc_cases as hc
import hmc_many_cases as mc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def bc():
    import beta_cores_amd as bc
    bc.default_context()
    return bc


def _p(x):
    return None if x is None else x.ctypes.data_as(ctypes.c_void_p)


@contextlib.contextmanager
def _chains_per_block(n):
    old = os.environ.get('BC_HMC_SMALL_CHAINS_PER_BLOCK')
    os.environ['BC_HMC_SMALL_CHAINS_PER_BLOCK'] = str(n)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop('BC_HMC_SMALL_CHAINS_PER_BLOCK', None)
        else:
            os.environ['BC_HMC_SMALL_CHAINS_PER_BLOCK'] = old


def _cuts(case, size=None):
    """The warm-up's chunk sizes: cut at every window end (so that the mass of every window can be read), or in chunks of `size`."""
    W = case['W']
    if size is not None:
        return [min(size, W - i) for i in range(0, W, size)]
    edges = [0] + ac.window_ends(case['flags']) + [W]
    return [b - a for a, b in zip(edges[:-1], edges[1:]) if b > a]


def _native_run(bc, case, problems=None, chunks=None, fill=7.):
    """A case through the entry points: the warm-up in `chunks`, the adapted state read after every chunk, then the kept iterations
    in one adapted chunk.  Returns per problem a dict for ac.compare / ac.check_sharp; `masses` holds the inverse masses read after
    the chunks that end with a window end.  Outputs are pre-filled with `fill` so that what was not copied shows."""
    from beta_cores_amd import _native as N
    lib, h = N.load(), bc.default_context().h
    problems = case['problems'] if problems is None else problems
    rows, w, row_ptr, start, im, _ = mc.pack([dict(pr, eps=0.) for pr in problems])
    P, c, d = start.shape
    E, U, L, W, K = np.ascontiguousarray(case['E']), np.ascontiguousarray(case['logU']), case['L'], case['W'], case['kept']
    T = W + K
    log_step = np.array([pr['log_step'] for pr in problems])
    s, lj, acc = np.full((P, T, c, d), fill), np.full((P, T, c), fill), np.full((P, T, c), int(fill), dtype=np.int32)
    stp, al, status = np.full((P, W, c), fill), np.full((P, W, c), fill), np.zeros(P, dtype=np.int32)
    masses = [[] for _ in range(P)]
    assert lib.bc_hmc_small_begin(h, _p(rows), _p(w), _p(row_ptr), P, d, _p(start), c, _p(im), L, T) == 0, N.last_error()
    try:
        assert lib.bc_hmc_adapt_begin(h, _p(log_step), case['delta'], ac.STAN['gamma'], ac.STAN['t0'], ac.STAN['kappa'], W, *case['bufs']) == 0, \
            N.last_error()
        ends, i0 = set(ac.window_ends(case['flags'])), 0
        fs, fm = np.full((P, c), fill), np.full((P, c, d), fill)
        for k in (chunks or _cuts(case)):
            assert lib.bc_hmc_adapt_chunk_begin(h, _p(E[i0:i0 + k]), _p(U[i0:i0 + k]), 0, k) == 0, N.last_error()
            cs, cl, ca = np.full((P, k, c, d), fill), np.full((P, k, c), fill), np.full((P, k, c), int(fill), dtype=np.int32)
            cst, cp, cal = np.zeros(P, dtype=np.int32), np.full((P, k, c), fill), np.full((P, k, c), fill)
            assert lib.bc_hmc_adapt_chunk_end(h, _p(cs), _p(cl), _p(ca), _p(cst), _p(cp), _p(cal)) == 0, N.last_error()
            s[:, i0:i0 + k], lj[:, i0:i0 + k], acc[:, i0:i0 + k], stp[:, i0:i0 + k], al[:, i0:i0 + k] = cs, cl, ca, cp, cal
            status |= cst
            i0 += k
            assert lib.bc_hmc_adapt_state(h, _p(fs), _p(fm)) == 0, N.last_error()
            if i0 in ends:
                for p in range(P):
                    masses[p].append(fm[p].copy())
        assert i0 == W
        assert lib.bc_hmc_adapted_chunk_begin(h, _p(E[W:]), _p(U[W:]), 0, K) == 0, N.last_error()
        cst = np.zeros(P, dtype=np.int32)
        ks, kl, ka = np.full((P, K, c, d), fill), np.full((P, K, c), fill), np.full((P, K, c), int(fill), dtype=np.int32)
        assert lib.bc_hmc_small_chunk_end(h, _p(ks), _p(kl), _p(ka), _p(cst)) == 0, N.last_error()
        s[:, W:], lj[:, W:], acc[:, W:] = ks, kl, ka
        status |= cst
    finally:
        assert lib.bc_hmc_small_end(h) == N.BC_OK
    return [dict(status=int(status[p]), samples=s[p], logjoint=lj[p], accept=acc[p], step=stp[p], alpha=al[p], masses=masses[p],
                 frozen_step=fs[p], frozen_mass=fm[p]) for p in range(P)]


_KEYS = ('samples', 'logjoint', 'accept', 'step', 'alpha', 'frozen_step', 'frozen_mass')


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in _KEYS)


@functools.lru_cache(maxsize=None)
def _device_case(name):
    """The device's run of a case, cut at the window ends: launched once, shared by the tests that compare against it."""
    import beta_cores_amd as bc
    return _native_run(bc, ac.make_case(name))


# ------------------------------------------------------------------ 1. the device against the restatement
@pytest.mark.parametrize('name', ac.CASE_NAMES)
def test_device_follows_the_long_double_restatement(bc, name):
    case = ac.make_case(name)
    got = _device_case(name)
    for p, (pr, g) in enumerate(zip(case['problems'], got)):
        ac.check_condition(name, ac.reference(name)[p])              # (on the restatement: rounding cannot flip a decision)
        assert g['status'] == 0
        ac.compare(g, name, p, 'device ' + pr['name'])
        ac.check_sharp(g['step'], g['frozen_step'], g['alpha'], g['samples'][:case['W']], g['masses'], pr, 'device ' + pr['name'])


# ------------------------------------------------------------------ 2. bit for bit
@pytest.mark.parametrize('name', ['small', 'batch', 'wide'])
def test_the_cut_of_the_warmup_changes_no_bit(bc, name):
    case = ac.make_case(name)
    one, sevens = _native_run(bc, case, chunks=[case['W']]), _native_run(bc, case, chunks=_cuts(case, 7))
    for a, b, c in zip(_device_case(name), one, sevens):
        assert _same(a, b) and _same(a, c)


@pytest.mark.parametrize('name', ['small', 'batch'])
def test_chains_per_block_change_no_bit(bc, name):
    case = ac.make_case(name)
    for cpb in (1, 2, 4):
        with _chains_per_block(cpb):
            got = _native_run(bc, case)
        assert all(_same(a, b) for a, b in zip(_device_case(name), got)), cpb


def test_a_problem_alone_has_the_bits_it_has_in_a_batch(bc):
    case = ac.make_case('batch')
    for p, pr in enumerate(case['problems']):
        alone = _native_run(bc, case, problems=[pr])
        assert _same(alone[0], _device_case('batch')[p]), p


# ------------------------------------------------------------------ 3. the kept chunk is an ordinary run from the adapted state
def test_kept_chunk_equals_an_ordinary_run_from_the_adapted_state(bc):
    from beta_cores_amd import _native as N
    lib, h = N.load(), bc.default_context().h
    case = ac.make_case('one')
    pr, g = case['problems'][0], _device_case('one')[0]
    W, K = case['W'], case['kept']
    assert case['c'] == 1 and g['accept'][W:].any()
    rows, w, row_ptr, _, _, _ = mc.pack([dict(pr, eps=0.)])
    start, im, eps = np.ascontiguousarray(g['samples'][W - 1][None]), np.ascontiguousarray(g['frozen_mass']), np.ascontiguousarray(g['frozen_step'])
    E, U = np.ascontiguousarray(case['E'][W:]), np.ascontiguousarray(case['logU'][W:])
    s, lj, acc, st = np.empty((1, K, 1, case['d'])), np.empty((1, K, 1)), np.empty((1, K, 1), dtype=np.int32), np.zeros(1, dtype=np.int32)
    assert lib.bc_hmc_small_begin(h, _p(rows), _p(w), _p(row_ptr), 1, case['d'], _p(start), 1, _p(im), case['L'], K) == 0, N.last_error()
    try:
        assert lib.bc_hmc_small_chunk_begin(h, _p(E), _p(U), 0, K, _p(eps)) == 0, N.last_error()
        assert lib.bc_hmc_small_chunk_end(h, _p(s), _p(lj), _p(acc), _p(st)) == 0, N.last_error()
    finally:
        assert lib.bc_hmc_small_end(h) == 0
    assert np.array_equal(s[0], g['samples'][W:]) and np.array_equal(lj[0], g['logjoint'][W:]) and np.array_equal(acc[0], g['accept'][W:])


# ------------------------------------------------------------------ 4. the Python route with scores and a summary
def test_stan_warmup_with_scores_and_summary_in_the_run(bc):
    from beta_cores_amd import samplers
    rng = np.random.RandomState(7)
    d, c = 5, 4
    probs = [hc.make_data(n, d, 70 + p) for p, n in enumerate((6, 30, 1))] + [(np.zeros((0, d)), None)]
    Xt = rng.randn(40, d)
    held = samplers.HeldOut(Xt, np.where(rng.rand(40) < 0.5, 1., -1.))
    kw = dict(n_samples=12, n_chains=c, step_size=0.3, n_leapfrog=4, start=rng.randn(c, d) * 0.1, warmup=30, chunk=8, adapt='stan')
    full = samplers.logistic_hmc_many(probs, rng=np.random.RandomState(3), **kw)
    lean = samplers.logistic_hmc_many(probs, rng=np.random.RandomState(3), score=held, keep_samples=False, summary=True, **kw)
    lap = samplers.logistic_hmc_many(probs, rng=np.random.RandomState(3), **dict(kw, start=None, inv_mass='laplace', laplace='batched'))
    for f, l, b in zip(full, lean, lap):
        assert f.route == 'small' and l.samples is None and f.samples.shape == (12, c, d)
        assert f.step_size.shape == (c,) and f.inv_mass.shape == (c, d) and f.warmup_steps.shape == (30, c) and f.warmup_accept_stat.shape == (30, c)
        assert np.all(f.step_size > 0) and np.all(f.inv_mass > 0) and np.all((f.warmup_accept_stat >= 0) & (f.warmup_accept_stat <= 1))
        assert np.array_equal(l.step_size, f.step_size) and np.array_equal(l.inv_mass, f.inv_mass) and np.array_equal(l.accept, f.accept)
        cor, tll = samplers.logistic_score(held, f.pooled())
        assert np.array_equal(l.correct.ravel(), cor) and np.array_equal(l.test_ll.ravel(), tll)
        cs = samplers.chain_summary(f.samples)
        assert all(np.array_equal(getattr(l.summary, k), getattr(cs, k), equal_nan=True) for k in ('mean', 'cov', 'rhat', 'ess'))
        assert b.samples.shape == (12, c, d) and np.all(np.isfinite(b.samples)) and b.inv_mass.shape == (c, d)
    # the Python loop against the entry points driven by hand on the same stream
    r = np.random.RandomState(3)
    draws = [(r.randn(k, c, d), np.log(r.rand(k, c))) for k in (8, 8, 8, 6, 8, 4)]
    flags, coef = ac.plan(30)
    Z, w = probs[1]
    case = dict(problems=[dict(Z=Z, w=w, start=kw['start'], inv_mass=np.ones(d), log_step=float(np.log(0.3)))], E=np.concatenate([e for e, _ in draws]),
                logU=np.concatenate([u for _, u in draws]), L=4, W=30, kept=12, delta=0.8, bufs=(75, 50, 25), flags=flags)
    by_hand = _native_run(bc, case, chunks=[30])[0]
    assert np.array_equal(by_hand['samples'][30:], full[1].samples) and np.array_equal(by_hand['step'], full[1].warmup_steps)
    assert np.array_equal(by_hand['alpha'], full[1].warmup_accept_stat) and np.array_equal(by_hand['frozen_step'], full[1].step_size)


# ------------------------------------------------------------------ 5. marked problems and refusals
def test_a_marked_problem_stays_local(bc):
    case = ac.make_case('batch')
    probs = [dict(pr) for pr in case['problems']]
    probs[1]['start'] = probs[1]['start'].copy()
    probs[1]['start'][2, 0] = np.inf
    got, clean = _native_run(bc, case, problems=probs), _device_case('batch')
    assert [g['status'] for g in got] == [0, 1, 0]
    assert _same(got[0], clean[0]) and _same(got[2], clean[2])
    bad = got[1]
    assert np.all(bad['samples'] == 7.) and np.all(bad['step'] == 7.) and np.all(bad['alpha'] == 7.)      # nothing was copied
    assert np.array_equal(bad['frozen_mass'], np.tile(probs[1]['inv_mass'], (case['c'], 1)))              # the state it began with
    assert np.allclose(bad['frozen_step'], np.exp(probs[1]['log_step']), rtol=1e-15)


def test_a_marked_problem_in_the_python_route(bc):
    """logistic_hmc_many(adapt='stan') with a weight that is not finite in one problem of a batch: strict=False returns the other
    problems with the bits they have without it and names the marked one; strict=True raises NumericalPrecisionError after the run
    is closed -- as adapt='chunks' does."""
    from beta_cores_amd import _native as N
    from beta_cores_amd import samplers
    d, c = 5, 4
    probs = [hc.make_data(n, d, 80 + p) for p, n in enumerate((6, 30, 9))]
    spoilt = [probs[0], (probs[1][0], np.where(np.arange(30) == 3, np.nan, probs[1][1])), probs[2]]
    kw = dict(n_samples=10, n_chains=c, step_size=0.3, n_leapfrog=4, start=np.random.RandomState(7).randn(c, d) * 0.1, warmup=24, chunk=6,
              adapt='stan')
    clean = samplers.logistic_hmc_many(probs, rng=np.random.RandomState(3), **kw)
    for extra in (dict(), dict(score=samplers.HeldOut(np.random.RandomState(8).randn(20, d), np.ones(20)), keep_samples=True, summary=True)):
        got = samplers.logistic_hmc_many(spoilt, rng=np.random.RandomState(3), strict=False, **kw, **extra)
        assert got.marked == [1] and got[1] is None and got.fallback == []
        for p in (0, 2):
            assert np.array_equal(got[p].samples, clean[p].samples) and np.array_equal(got[p].step_size, clean[p].step_size)
            assert np.array_equal(got[p].inv_mass, clean[p].inv_mass) and np.array_equal(got[p].warmup_accept_stat, clean[p].warmup_accept_stat)
    with pytest.raises(N.NumericalPrecisionError, match='problem\\(s\\) 1'):
        samplers.logistic_hmc_many(spoilt, rng=np.random.RandomState(3), **kw)
    assert samplers.logistic_hmc_many(spoilt, rng=np.random.RandomState(3), strict=False, **dict(kw, adapt='chunks')).marked == [1]


def test_refusals(bc):
    from beta_cores_amd import _native as N
    from beta_cores_amd import samplers
    lib, h = N.load(), bc.default_context().h
    BAD = N.BC_INVALID_ARGUMENT
    case = ac.make_case('small')
    pr = case['problems'][0]
    rows, w, row_ptr, start, im, _ = mc.pack([dict(pr, eps=0.)])
    P, c, d = start.shape
    E, U = np.ascontiguousarray(case['E']), np.ascontiguousarray(case['logU'])
    ls, W = np.array([pr['log_step']]), 24
    s2, st = np.empty((P, c)), np.empty((P, c, d))
    args = (0.8, 0.05, 10., 0.75, W, 6, 4, 5)
    assert lib.bc_hmc_adapt_begin(h, _p(ls), *args) == BAD                                    # no run is open
    assert lib.bc_hmc_small_begin(h, _p(rows), _p(w), _p(row_ptr), P, d, _p(start), c, _p(im), case['L'], 30) == 0, N.last_error()
    try:
        assert lib.bc_hmc_adapted_chunk_begin(h, _p(E[:2]), _p(U[:2]), 0, 2) == BAD and b'bc_hmc_adapt_begin' in lib.bc_last_error()
        assert lib.bc_hmc_adapt_chunk_begin(h, _p(E[:2]), _p(U[:2]), 0, 2) == BAD
        assert lib.bc_hmc_adapt_state(h, _p(s2), _p(st)) == BAD
        for bad in ((0., 0.05, 10., 0.75, W, 6, 4, 5), (1., 0.05, 10., 0.75, W, 6, 4, 5), (0.8, 0., 10., 0.75, W, 6, 4, 5), (0.8, 0.05, -1., 0.75, W, 6, 4, 5),
                    (0.8, 0.05, 10., 0., W, 6, 4, 5), (0.8, 0.05, 10., 0.75, 0, 6, 4, 5), (0.8, 0.05, 10., 0.75, 31, 6, 4, 5), (0.8, 0.05, 10., 0.75, W, -1, 4, 5),
                    (0.8, 0.05, 10., 0.75, W, 6, 4, 0)):
            assert lib.bc_hmc_adapt_begin(h, _p(ls), *bad) == BAD, bad
        assert lib.bc_hmc_adapt_begin(h, None, *args) == BAD and lib.bc_hmc_adapt_begin(h, _p(np.array([np.inf])), *args) == BAD
        assert lib.bc_hmc_adapt_begin(h, _p(ls), *args) == 0, N.last_error()
        assert lib.bc_hmc_adapt_begin(h, _p(ls), *args) == BAD                                # twice
        assert lib.bc_hmc_adapt_chunk_begin(h, None, _p(U[:2]), 0, 2) == BAD and lib.bc_hmc_adapt_chunk_begin(h, _p(E[:2]), _p(U[:2]), 0, 0) == BAD
        assert lib.bc_hmc_adapt_chunk_begin(h, _p(E[:2]), _p(U[:2]), 3, 2) == BAD              # a stride below k C D
        assert lib.bc_hmc_adapt_chunk_begin(h, _p(E[:25]), _p(U[:25]), 0, 25) == BAD and b'exceed' in lib.bc_last_error()      # more than planned
        k = 20
        assert lib.bc_hmc_adapt_chunk_begin(h, _p(E[:k]), _p(U[:k]), 0, k) == 0, N.last_error()
        assert lib.bc_hmc_adapt_state(h, _p(s2), _p(st)) == BAD                               # a chunk is pending
        lj, acc, cst, cp, cal = np.empty((P, k, c)), np.empty((P, k, c), dtype=np.int32), np.zeros(P, dtype=np.int32), np.empty((P, k, c)), np.empty((P, k, c))
        assert lib.bc_hmc_adapt_chunk_end(h, None, _p(lj), _p(acc), _p(cst), None, _p(cal)) == BAD      # ... and stays pending
        assert lib.bc_hmc_adapt_chunk_end(h, None, _p(lj), _p(acc), _p(cst), _p(cp), _p(cal)) == 0, N.last_error()
        assert lib.bc_hmc_adapt_chunk_end(h, None, _p(lj), _p(acc), _p(cst), _p(cp), _p(cal)) == BAD    # nothing is pending
        assert lib.bc_hmc_adapt_chunk_begin(h, _p(E[:5]), _p(U[:5]), 0, 5) == BAD              # 20 + 5 > 24
        assert lib.bc_hmc_adapted_chunk_begin(h, _p(E[:2]), _p(U[:2]), 0, 2) == 0, N.last_error()
        assert lib.bc_hmc_adapt_chunk_end(h, None, _p(lj), _p(acc), _p(cst), _p(cp), _p(cal)) == BAD    # not a warm-up chunk: it stays pending
        ks, kl, ka = np.empty((P, 2, c, d)), np.empty((P, 2, c)), np.empty((P, 2, c), dtype=np.int32)
        assert lib.bc_hmc_small_chunk_end(h, _p(ks), _p(kl), _p(ka), _p(cst)) == 0, N.last_error()
        assert lib.bc_hmc_adapted_chunk_begin(h, _p(E[:9]), _p(U[:9]), 0, 9) == BAD            # 22 + 9 > the run's 30
        assert lib.bc_hmc_adapt_state(h, None, _p(st)) == BAD and lib.bc_hmc_adapt_state(h, _p(s2), _p(st)) == 0
    finally:
        assert lib.bc_hmc_small_end(h) == 0
    assert lib.bc_hmc_adapt_state(h, _p(s2), _p(st)) == BAD                                   # the run is closed
    # the route that does not fit one block is refused by name before anything is launched
    big = [hc.make_data(5, 16, 1), hc.make_data(3000, 16, 2)]
    with pytest.raises(ValueError, match='problem 1 '):
        samplers.logistic_hmc_many(big, n_samples=4, n_chains=2, start=np.zeros((2, 16)), warmup=20, adapt='stan')
    # ... and a run without the argument still serves it
    res = samplers.logistic_hmc_many(big, n_samples=4, n_chains=2, start=np.zeros((2, 16)), warmup=4, rng=np.random.RandomState(1))
    assert res.fallback == [1]


# ------------------------------------------------------------------ 6. one statistical guard
def test_statistical_guard(bc):
    """mc.guard_problems() with inv_mass=None, warm-up 200, from the start steps 0.01 and 2.0: mc.check_guard's bars for both runs,
    the kept acceptance in [delta, 0.99] and the median adapted steps of the two runs within a factor 1.5 per problem.  The float64
    restatement clears them for this seed: tests/test_hmc_adapt_cpu.py::test_the_restatement_stays_inside_the_statistical_guard."""
    runs, fits = ac.guard_runs()
    assert all(r.route == 'small' for run in runs for r in run)
    ac.check_guard_runs(runs, fits, 'device')
