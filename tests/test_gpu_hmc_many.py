"""The batched small-problem HMC run (k_hmc_small, include/beta_cores_hmc_small.h) and samplers.logistic_hmc_many on the GPU.

1. The run of every problem of every batch case of tests/hmc_many_cases.py against the long-double restatement.
2. The in-LDS pass under the bound derived in tests/hmc_cases.py (rows_pass_bound), element-wise.
3. Independence and repeatability, bit for bit -- from the batch, and from how many chains share a block (1, 2 or 4).
4. logistic_hmc_many against a loop of logistic_hmc on equally seeded streams.
5. The capacity rule: the largest problem that fits, the first that does not, and the fallback.
6. Failures stay local.
7. Refusals.
8. One statistical guard against gross errors.
"""
import contextlib
import ctypes
import functools
import os

import numpy as np
import pytest

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


def _native_run(bc, problems, chunks=None, fill=7.):
    """(status of the calls, [dict(status, samples, logjoint, accept) per problem]) of a batch on shared draws through the chunked
    entry points; outputs are pre-filled with `fill` so that what was not copied shows."""
    from beta_cores_amd import _native as N
    lib, h = N.load(), bc.default_context().h
    rows, w, row_ptr, start, im, eps = mc.pack(problems)
    P, c, d = start.shape
    E, U, L = np.ascontiguousarray(problems[0]['E']), np.ascontiguousarray(problems[0]['logU']), problems[0]['L']
    T = E.shape[0]
    s, lj, acc = np.full((P, T, c, d), fill), np.full((P, T, c), fill), np.full((P, T, c), int(fill), dtype=np.int32)
    status = np.zeros(P, dtype=np.int32)
    st = lib.bc_hmc_small_begin(h, _p(rows), _p(w), _p(row_ptr), P, d, _p(start), c, _p(im), L, T)
    if st:
        return st, None
    i0 = 0
    for k in (chunks or [T]):
        st = lib.bc_hmc_small_chunk_begin(h, _p(E[i0:i0 + k]), _p(U[i0:i0 + k]), 0, k, _p(eps))
        cs, cl, ca = np.full((P, k, c, d), fill), np.full((P, k, c), fill), np.full((P, k, c), int(fill), dtype=np.int32)
        cst = np.zeros(P, dtype=np.int32)
        if not st:
            st = lib.bc_hmc_small_chunk_end(h, _p(cs), _p(cl), _p(ca), _p(cst))
        if st:
            break
        s[:, i0:i0 + k], lj[:, i0:i0 + k], acc[:, i0:i0 + k] = cs, cl, ca
        status |= cst
        i0 += k
    assert lib.bc_hmc_small_end(h) == N.BC_OK
    return st, [dict(status=int(status[p]), samples=s[p], logjoint=lj[p], accept=acc[p]) for p in range(P)]


def _same(a, b):
    return np.array_equal(a['samples'], b['samples']) and np.array_equal(a['logjoint'], b['logjoint']) and np.array_equal(a['accept'], b['accept'])


@functools.lru_cache(maxsize=None)
def _device_batch(name):
    """The device's run of a batch case in one chunk: launched once, shared by the tests that compare against it."""
    import beta_cores_amd as bc
    st, got = _native_run(bc, mc.make_batch_case(name)['problems'])
    assert st == 0
    return got


# ------------------------------------------------------------------ 1. the run against the restatement
@pytest.mark.parametrize('name', mc.BATCH_NAMES)
def test_run_follows_the_restatement(bc, name):
    case, refs = mc.make_batch_case(name), mc.batch_reference(name)
    mc.check_batch_condition(refs)                                  # (on the restatement: rounding cannot flip a decision)
    got = _device_batch(name)
    for pr, g, (ref, tol_s, tol_l) in zip(case['problems'], got, refs):
        assert g['status'] == 0
        mc.compare_with_reference(g, ref, tol_s, tol_l, pr['start'], 'device ' + pr['name'])
    # the same run in two chunks: the state a chunk leaves in global memory is the state the next one starts from
    st, two = _native_run(bc, case['problems'], chunks=[1, case['T'] - 1])
    assert st == 0 and all(_same(a, b) for a, b in zip(two, got))


# ------------------------------------------------------------------ 2. the in-LDS pass under the derived bound
def _logjoint(bc, problems, thetas, value=True):
    """bc_hmc_small_logjoint on a list of (Z, w) with thetas [P, C, D]: (values [P, C] or None, grads [P, C, D])."""
    from beta_cores_amd import _native as N
    prs = [dict(Z=Z, w=w, start=th, inv_mass=np.ones(Z.shape[1]), eps=1.) for (Z, w), th in zip(problems, thetas)]
    rows, w, row_ptr, th, _, _ = mc.pack(prs)
    P, c, d = th.shape
    val, grad = (np.full((P, c), 7.) if value else None), np.full((P, c, d), 7.)
    st = N.load().bc_hmc_small_logjoint(bc.default_context().h, _p(rows), _p(w), _p(row_ptr), P, d, _p(th), c, _p(val), _p(grad))
    assert st == 0, N.last_error()
    return val, grad


def _check_pass(bc, problems, thetas, label):
    val, grad = _logjoint(bc, problems, thetas)
    for p, ((Z, w), th) in enumerate(zip(problems, thetas)):
        rv, rg = hc.logjoint(Z, w, th, np.longdouble)
        bv, bg = hc.rows_pass_bound(Z, w, th)
        assert np.all(np.isfinite(val[p])) and np.all(np.isfinite(grad[p]))
        ev, eg = np.abs(val[p] - rv).astype(np.float64), np.abs(grad[p] - rg).astype(np.float64)
        print('in-LDS pass %s[%d]: worst error / bound: value %.3f, gradient %.3f' % (label, p, (ev / bv).max(), (eg / bg).max()))
        assert np.all(ev <= bv), (label, p, (ev / bv).max())
        assert np.all(eg <= bg), (label, p, (eg / bg).max())
    return val, grad


@pytest.mark.parametrize('name', mc.BATCH_NAMES)
@pytest.mark.parametrize('variant', ['weighted', 'unweighted', 'zero'])
def test_in_lds_pass_within_the_derived_bound(bc, name, variant):
    case = mc.make_batch_case(name)
    rng = np.random.RandomState(case['d'] + case['c'])
    thetas = [rng.randn(case['c'], case['d']) / np.sqrt(case['d']) for _ in case['problems']]
    weights = dict(weighted=lambda pr: pr['w'], unweighted=lambda pr: None, zero=lambda pr: np.zeros(pr['Z'].shape[0]))[variant]
    problems = [(pr['Z'], weights(pr)) for pr in case['problems']]
    val, grad = _check_pass(bc, problems, thetas, '%s %s' % (name, variant))
    if variant == 'zero':
        assert all(np.array_equal(g, -th) for g, th in zip(grad, thetas))      # the prior alone
    if variant == 'weighted':                                                    # the gradient-only pass: the same gradients
        nov, g2 = _logjoint(bc, problems, thetas, value=False)
        assert nov is None and np.array_equal(g2, grad)


@pytest.mark.parametrize('d,c', [(5, 3), (128, 17)])
def test_in_lds_pass_on_both_sides_of_the_branch(bc, d, c):
    """Rows with |m| in {0.5, 99.9, 100, 120, 800} for every chain, both signs (built as test_gpu_hmc.py builds them): no NaN,
    no inf, within the bound."""
    rng = np.random.RandomState(d)
    th = np.tile(rng.randn(d) / np.sqrt(d), (c, 1)) * (1. + 1e-3 * np.arange(c))[:, None]
    base = th[0] / th[0].dot(th[0])
    mags = np.array([0.5, 99.9, 100., 120., 800.])
    jitter = np.array([0., 1e-3, 1e-3, 1e-3])[:, None]
    Z = np.concatenate([s * m * base[None, :] + jitter * rng.randn(4, d) for m in mags for s in (1., -1.)])
    w = rng.rand(Z.shape[0]) + 0.5
    m = -Z.dot(th.T)
    assert np.abs(m).max() > 790 and (m >= 100).any() and (m < 100).any() and (np.abs(np.abs(m) - 100.) < 1.).any()
    _check_pass(bc, [(Z, w)], [th], 'branch rows D=%d C=%d' % (d, c))


# ------------------------------------------------------------------ 3. independence and repeatability
def test_a_problems_bits_do_not_depend_on_the_batch(bc):
    case = mc.make_batch_case('ragged5')
    probs = case['problems']
    base = _device_batch('ragged5')
    st, again = _native_run(bc, probs)
    assert st == 0 and all(_same(a, b) for a, b in zip(again, base))             # a second call
    st, rev = _native_run(bc, probs[::-1])
    assert st == 0 and all(_same(a, b) for a, b in zip(rev[::-1], base))         # the batch reversed
    for p in range(len(probs)):
        st, alone = _native_run(bc, [probs[p]])                                  # alone, P = 1
        assert st == 0 and _same(alone[0], base[p]), p
        one = dict(probs[p], start=probs[p]['start'][1:2], E=probs[p]['E'][:, 1:2], logU=probs[p]['logU'][:, 1:2])
        st, chain = _native_run(bc, [one])                                       # one chain of it alone against the same among C = 3
        assert st == 0 and np.array_equal(chain[0]['samples'][:, 0], base[p]['samples'][:, 1]), p
        assert np.array_equal(chain[0]['logjoint'][:, 0], base[p]['logjoint'][:, 1]) and np.array_equal(chain[0]['accept'][:, 0], base[p]['accept'][:, 1])


@contextlib.contextmanager
def _chains_per_block(v):
    """BC_HMC_SMALL_CHAINS_PER_BLOCK = v for the begins inside (the library reads it at every begin); None: the automatic choice."""
    old = os.environ.pop('BC_HMC_SMALL_CHAINS_PER_BLOCK', None)
    if v is not None:
        os.environ['BC_HMC_SMALL_CHAINS_PER_BLOCK'] = str(v)
    try:
        yield
    finally:
        os.environ.pop('BC_HMC_SMALL_CHAINS_PER_BLOCK', None)
        if old is not None:
            os.environ['BC_HMC_SMALL_CHAINS_PER_BLOCK'] = old


def test_packing_chains_into_a_block_changes_no_bits(bc):
    """The library chooses how many chains of a problem share a block (k_hmc_small<1 | 2 | 4>) from the batch's LARGEST problem, so
    the batch decides which instantiation runs a problem: independence from the batch needs the three to agree bit for bit.
    pack128 (D = 128, n = 5 | 40 | 100, C = 4): a block of four chains fits, so a forced count of 1, 2 and 4 is the count that
    runs.  Samples, log-joints and decisions are equal across the three and the automatic choice; the 4-chain run follows the
    restatement; a problem alone in a 1-chain block equals itself in the batch, and in the reversed batch, in 4-chain blocks --
    by the occupancy rule the automatic choice is 1 for the 5-row problem alone and 4 in the batch, and both are compared too.
    Then C = 8 (two groups of four, four of two) and the pass on its own."""
    case, refs = mc.make_batch_case('pack128'), mc.batch_reference('pack128')
    mc.check_batch_condition(refs)
    probs = case['problems']
    runs = {}
    for v in (1, 2, 4, None):
        with _chains_per_block(v):
            st, runs[v] = _native_run(bc, probs)
        assert st == 0, v
    for v in (2, 4, None):
        assert all(_same(a, b) for a, b in zip(runs[v], runs[1])), v
    for pr, g, (ref, tol_s, tol_l) in zip(probs, runs[4], refs):
        assert g['status'] == 0
        mc.compare_with_reference(g, ref, tol_s, tol_l, pr['start'], 'four chains per block ' + pr['name'])
    with _chains_per_block(4):
        st, rev = _native_run(bc, probs[::-1])
    assert st == 0 and all(_same(a, b) for a, b in zip(rev[::-1], runs[1]))
    for p in range(len(probs)):
        for v in (1, None):
            with _chains_per_block(v):
                st, alone = _native_run(bc, [probs[p]])
            assert st == 0 and _same(alone[0], runs[4][p]), (p, v)
        one = dict(probs[p], start=probs[p]['start'][2:3], E=probs[p]['E'][:, 2:3], logU=probs[p]['logU'][:, 2:3])
        st, chain = _native_run(bc, [one])                                       # C = 1: one chain per block whatever is asked
        assert st == 0 and np.array_equal(chain[0]['samples'][:, 0], runs[4][p]['samples'][:, 2])
        assert np.array_equal(chain[0]['logjoint'][:, 0], runs[4][p]['logjoint'][:, 2]) and np.array_equal(chain[0]['accept'][:, 0], runs[4][p]['accept'][:, 2])
    # eight chains: the block index walks (problem, group of chains); chain c of a group of four is chain c of a group of one
    wide = mc.build_batch('pack128x8', 128, (100, 5), 8, 2, 2, 0.08, 26)['problems']
    got = {}
    for v in (1, 2, 4, None):
        with _chains_per_block(v):
            st, got[v] = _native_run(bc, wide)
        assert st == 0, v
    for v in (2, 4, None):
        assert all(_same(a, b) for a, b in zip(got[v], got[1])), v
    assert not np.array_equal(got[4][0]['samples'][:, 0], got[4][0]['samples'][:, 4])      # (the chains differ: a mix-up would show)
    # the pass on its own (the start pass of a run is the same launch)
    rng = np.random.RandomState(3)
    thetas = [rng.randn(8, 128) / np.sqrt(128.) for _ in wide]
    problems = [(pr['Z'], pr['w']) for pr in wide]
    with _chains_per_block(1):
        v1, g1 = _logjoint(bc, problems, thetas)
    with _chains_per_block(4):
        v4, g4 = _logjoint(bc, problems, thetas)
    assert np.array_equal(v1, v4) and np.array_equal(g1, g4)


# ------------------------------------------------------------------ 4. agreement with the existing path
@pytest.mark.parametrize('name', ['ragged5', 'wide128'])
def test_many_agrees_with_a_loop_of_logistic_hmc(bc, name):
    """logistic_hmc_many(..., rng=RandomState(5)) against logistic_hmc(Z_p, w_p, ..., rng=RandomState(5)) per problem: two warm-up
    chunks of 3 iterations, 4 kept.  Seed 5: on the restatement (NumpyHMCEngine per problem) no decision is within 1e-6 of
    flipping -- the smallest margins are 1.4e-2 (ragged5) and 2.5e-4 (wide128) -- asserted below."""
    from beta_cores_amd import samplers
    case = mc.make_batch_case(name)
    prs = case['problems']
    problems = [(pr['Z'], pr['w']) for pr in prs]
    kw = dict(n_samples=4, n_chains=case['c'], n_leapfrog=case['L'], warmup=6, adapt_every=3)
    many_kw = dict(step_size=[pr['eps'] for pr in prs], inv_mass=np.array([pr['inv_mass'] for pr in prs]), start=np.array([pr['start'] for pr in prs]))
    engines = mc.MarginEngines()
    rest = samplers.logistic_hmc_many(problems, rng=np.random.RandomState(5), engine=engines, **many_kw, **kw)
    assert engines.min_margin() > 1e-6
    many = samplers.logistic_hmc_many(problems, rng=np.random.RandomState(5), **many_kw, **kw)
    assert many.fallback == [] and many.marked == [] and many.device_ms > 0.
    r = np.random.RandomState(5)
    for k in (3, 3):
        r.randn(k, case['c'], case['d']), r.rand(k, case['c'])
    E, U = r.randn(4, case['c'], case['d']), np.log(r.rand(4, case['c']))
    for p, pr in enumerate(prs):
        one = samplers.logistic_hmc(pr['Z'], pr['w'], step_size=pr['eps'], inv_mass=pr['inv_mass'], start=pr['start'],
                                    rng=np.random.RandomState(5), **kw)
        m = many[p]
        assert m.route == 'small' and np.array_equal(m.accept, one.accept) and np.array_equal(m.accept, rest[p].accept)
        assert np.array_equal(m.warmup_steps, one.warmup_steps) and m.step_size == one.step_size and m.warmup_steps.shape == (2,)
        # the tolerance of the kept iterations of this problem, from the restatement on the draws they used (as test_gpu_hmc.py's
        # weighted-coreset test takes it); both paths may deviate by it
        _, tol_s, tol_l = hc.trace_tolerance(dict(pr, eps=m.step_size, E=E, logU=U))
        ds, dl = hc.rel_dev(m.samples, one.samples), hc.rel_dev(m.logjoint, one.logjoint)
        print('%s[%d]: many against the loop: samples %.3g (tol %.3g), log-joint %.3g (tol %.3g)' % (name, p, ds, 2 * tol_s, dl, 2 * tol_l))
        assert ds <= 2. * tol_s and dl <= 2. * tol_l


# ------------------------------------------------------------------ 5. capacity
def _capacity_problem(n, d=128, c=2, T=3, seed=51):
    Z, w = hc.make_data(n, d, seed)
    r = np.random.RandomState(seed + 1)
    return dict(name='n=%d' % n, Z=Z, w=w, start=r.randn(c, d) * 0.1, inv_mass=0.5 + r.rand(d), eps=0.05, L=3, E=r.randn(T, c, d),
                logU=np.log(r.rand(T, c)))


def test_capacity_rule_and_fallback(bc):
    from beta_cores_amd import _native as N, samplers
    lib, h = N.load(), bc.default_context().h
    assert lib.bc_hmc_small_fits(h, 128, 128) == 1 and lib.bc_hmc_small_fits(h, 1000, 16) == 1 and lib.bc_hmc_small_fits(h, 60, 256) == 1
    assert lib.bc_hmc_small_fits(h, 0, 128) == 0 and lib.bc_hmc_small_fits(h, 10, 257) == 0 and lib.bc_hmc_small_fits(h, 10, 0) == 0
    n_over = next(n for n in range(1, 100000) if lib.bc_hmc_small_fits(h, n, 128) == 0)
    assert n_over > 128 and all(lib.bc_hmc_small_fits(h, n, 128) == 0 for n in (n_over + 1, 2 * n_over, 10 ** 6))
    # the largest problem that fits runs and follows the restatement
    big = _capacity_problem(n_over - 1)
    ref, tol_s, tol_l = hc.trace_tolerance(big)
    assert np.abs(ref['margin']).min() > 1e-6
    st, got = _native_run(bc, [big])
    assert st == 0 and got[0]['status'] == 0
    mc.compare_with_reference(got[0], ref, tol_s, tol_l, big['start'], 'largest that fits (n = %d)' % (n_over - 1))
    # the first that does not is refused by the C entry points, before a launch
    over = _capacity_problem(n_over)
    st, _ = _native_run(bc, [over])
    assert st == N.BC_INVALID_ARGUMENT and 'LDS' in N.last_error()
    assert lib.bc_hmc_small_end(h) == N.BC_INVALID_ARGUMENT                       # no run was opened
    # ... and served by logistic_hmc_many through logistic_hmc's engine, beside a problem that fits, on the same draws
    ref, tol_s, tol_l = hc.trace_tolerance(over)
    assert np.abs(ref['margin']).min() > 1e-6
    small = _capacity_problem(20)
    sref, stol_s, stol_l = hc.trace_tolerance(dict(small, E=over['E'], logU=over['logU']))
    assert np.abs(sref['margin']).min() > 1e-6
    rng = np.random.RandomState(52)                                              # _capacity_problem's stream, at its draws
    rng.randn(2, 128)
    rng.rand(128)
    res = samplers.logistic_hmc_many([(small['Z'], small['w']), (over['Z'], over['w'])], n_samples=3, n_chains=2, step_size=0.05, n_leapfrog=3,
                                     inv_mass=np.array([small['inv_mass'], over['inv_mass']]), start=np.array([small['start'], over['start']]), rng=rng)
    assert res.fallback == [1] and res[0].route == 'small' and res[1].route == 'single'
    for r, rf, ts, tl, pr in ((res[0], sref, stol_s, stol_l, small), (res[1], ref, tol_s, tol_l, over)):
        mc.compare_with_reference(dict(samples=r.samples, logjoint=r.logjoint, accept=r.accept), rf, ts, tl, pr['start'], 'fallback batch ' + r.route)


# ------------------------------------------------------------------ 6. failures stay local
def test_failures_stay_local(bc):
    from beta_cores_amd import _native as N, samplers
    import beta_cores_amd
    probs = [dict(pr) for pr in mc.make_batch_case('ragged5')['problems'][1:4]]
    st, clean = _native_run(bc, probs)
    assert st == 0
    probs[1]['start'] = probs[1]['start'].copy()
    probs[1]['start'][2, 3] = np.inf
    st, got = _native_run(bc, probs, chunks=[2, 4])
    assert st == 0 and [g['status'] for g in got] == [N.BC_OK, N.BC_NUMERICAL_PRECISION, N.BC_OK]
    assert np.all(got[1]['samples'] == 7.) and np.all(got[1]['logjoint'] == 7.) and np.all(got[1]['accept'] == 7)      # nothing was copied
    assert _same(got[0], clean[0]) and _same(got[2], clean[2])
    # a huge step rejects everything: the positions stay at the start bit for bit
    probs[0]['eps'] = 1e6
    st, got = _native_run(bc, probs)
    assert st == 0 and got[0]['status'] == 0 and not got[0]['accept'].any() and _same(got[2], clean[2])
    assert np.array_equal(got[0]['samples'], np.broadcast_to(probs[0]['start'], got[0]['samples'].shape))
    assert np.all(np.isfinite(got[0]['logjoint'])) and np.array_equal(got[0]['logjoint'], np.broadcast_to(got[0]['logjoint'][0], got[0]['logjoint'].shape))
    # through Python: strict raises after the run is closed, naming the problem; strict=False leaves None there
    kw = dict(n_samples=3, n_chains=3, step_size=0.1, n_leapfrog=2, inv_mass=np.array([pr['inv_mass'] for pr in probs]),
              start=np.array([pr['start'] for pr in probs]))
    problems = [(pr['Z'], pr['w']) for pr in probs]
    with pytest.raises(beta_cores_amd.NumericalPrecisionError, match=r'problem\(s\) 1 '):
        samplers.logistic_hmc_many(problems, rng=np.random.RandomState(1), **kw)
    res = samplers.logistic_hmc_many(problems, rng=np.random.RandomState(1), strict=False, **kw)      # (the raise closed the run)
    assert res[1] is None and res.marked == [1] and res[0].samples.shape == (3, 3, 5) and np.all(np.isfinite(res[2].samples))


# ------------------------------------------------------------------ 7. refusals
def test_refusals(bc):
    """Each is refused with BC_INVALID_ARGUMENT before a launch, and the context serves the next run."""
    from beta_cores_amd import _native as N
    lib, h = N.load(), bc.default_context().h
    probs = mc.make_batch_case('ragged5')['problems'][:3]
    rows, w, row_ptr, start, im, eps = mc.pack(probs)
    P, c, d = start.shape
    E, U = np.ascontiguousarray(probs[0]['E']), np.ascontiguousarray(probs[0]['logU'])
    T = E.shape[0]
    bad = N.BC_INVALID_ARGUMENT

    def begin(rows=rows, w=w, row_ptr=row_ptr, P=P, d=d, start=start, c=c, im=im, L=4, T=T):
        return lib.bc_hmc_small_begin(h, _p(rows), _p(w), _p(row_ptr), P, d, _p(start), c, _p(im), L, T)
    assert begin(c=65, start=np.zeros((P, 65, d))) == bad and 'chains' in N.last_error()
    assert begin(c=0) == bad
    assert begin(d=257, rows=np.zeros((int(row_ptr[-1]), 257)), start=np.zeros((P, c, 257)), im=np.ones((P, 257))) == bad and '256' in N.last_error()
    assert begin(row_ptr=np.array([0, 8, 8, 72], dtype=np.int64)) == bad and 'row_ptr' in N.last_error()      # an empty problem
    assert begin(row_ptr=np.array([0, 8, 1, 72], dtype=np.int64)) == bad and 'row_ptr' in N.last_error()      # not monotone
    assert begin(row_ptr=np.array([1, 8, 9, 72], dtype=np.int64)) == bad
    assert begin(P=0) == bad
    for missing in ('rows', 'w', 'row_ptr', 'start', 'im'):
        assert begin(**{missing: None}) == bad, missing
    assert begin(im=im * 0.) == bad and begin(L=0) == bad and begin(T=0) == bad
    g = np.empty((P, c, d))
    assert lib.bc_hmc_small_logjoint(h, _p(rows), _p(w), _p(row_ptr), P, d, _p(start), c, None, None) == bad
    assert lib.bc_hmc_small_logjoint(h, _p(rows), _p(w), _p(row_ptr), P, d, _p(start), 65, None, _p(g)) == bad
    assert lib.bc_hmc_small_end(h) == bad and lib.bc_hmc_small_chunk_begin(h, _p(E), _p(U), 0, T, _p(eps)) == bad      # no run is open
    # a run is open: a second one, the pass on its own and a single-problem run are refused; bad chunks are refused
    case = hc.make_trace_case('small')
    dz, wd = bc.DeviceData(case['Z']), bc.DeviceData(case['w'].reshape(-1, 1))
    hs, him = np.ascontiguousarray(case['start']), np.ascontiguousarray(case['inv_mass'])
    assert begin() == N.BC_OK
    assert begin() == bad and 'already open' in N.last_error()
    assert lib.bc_hmc_small_logjoint(h, _p(rows), _p(w), _p(row_ptr), P, d, _p(start), c, None, _p(g)) == bad
    assert lib.bc_hmc_begin(h, dz.h, wd.h, _p(hs), hs.shape[0], _p(him), 4, 6) == bad and 'bc_hmc_small_end' in N.last_error()
    s, lj, acc, stt = np.empty((P, T, c, d)), np.empty((P, T, c)), np.empty((P, T, c), dtype=np.int32), np.empty(P, dtype=np.int32)
    assert lib.bc_hmc_small_chunk_end(h, _p(s), _p(lj), _p(acc), _p(stt)) == bad                          # nothing was enqueued
    assert lib.bc_hmc_small_chunk_begin(h, _p(E), _p(U), 0, T + 1, _p(eps)) == bad                          # more than the run's iterations
    assert lib.bc_hmc_small_chunk_begin(h, _p(E), _p(U), T * c * d - 1, T, _p(eps)) == bad                  # a stride shorter than a problem's draws
    assert lib.bc_hmc_small_chunk_begin(h, _p(E), _p(U), 0, T, _p(eps * np.array([1., -1., 1.]))) == bad
    assert lib.bc_hmc_small_chunk_begin(h, None, _p(U), 0, T, _p(eps)) == bad and lib.bc_hmc_small_chunk_begin(h, _p(E), _p(U), 0, T, None) == bad
    assert lib.bc_hmc_small_chunk_begin(h, _p(E), _p(U), 0, T, _p(eps)) == N.BC_OK
    assert lib.bc_hmc_small_chunk_begin(h, _p(E), _p(U), 0, T, _p(eps)) == bad                              # a chunk is pending
    assert lib.bc_hmc_small_chunk_end(h, _p(s), _p(lj), _p(acc), None) == bad                               # an output is missing: it stays pending
    assert lib.bc_hmc_small_chunk_end(h, _p(s), _p(lj), _p(acc), _p(stt)) == N.BC_OK and not stt.any()
    assert lib.bc_hmc_small_end(h) == N.BC_OK
    base = _native_run(bc, probs)[1]
    assert all(np.array_equal(s[p], base[p]['samples']) and np.array_equal(acc[p], base[p]['accept']) for p in range(P))      # the refusals left the run alone
    # the converse: an open single-problem run refuses a batched one
    assert lib.bc_hmc_begin(h, dz.h, wd.h, _p(hs), hs.shape[0], _p(him), 4, 6) == N.BC_OK
    assert begin() == bad and 'bc_hmc' in N.last_error()
    assert lib.bc_hmc_small_logjoint(h, _p(rows), _p(w), _p(row_ptr), P, d, _p(start), c, None, _p(g)) == bad
    assert lib.bc_hmc_end(h) == N.BC_OK
    ms = ctypes.c_double(-1.)
    assert lib.bc_hmc_small_device_ms(h, ctypes.byref(ms)) == N.BC_OK and ms.value > 0.
    # independent draws through the C entry: problem p reads its own block; equal blocks give the shared run's bits
    assert begin() == N.BC_OK
    En, Un = np.ascontiguousarray(np.broadcast_to(E, (P,) + E.shape)), np.ascontiguousarray(np.broadcast_to(U, (P,) + U.shape))
    assert lib.bc_hmc_small_chunk_begin(h, _p(En), _p(Un), T * c * d, T, _p(eps)) == N.BC_OK
    assert lib.bc_hmc_small_chunk_end(h, _p(s), _p(lj), _p(acc), _p(stt)) == N.BC_OK and lib.bc_hmc_small_end(h) == N.BC_OK
    assert all(np.array_equal(s[p], base[p]['samples']) and np.array_equal(lj[p], base[p]['logjoint']) for p in range(P))


# ------------------------------------------------------------------ 8. one statistical guard
def test_statistical_guard(bc):
    """Eight weighted problems of n = 40, D = 4; 16 chains, L = 8, mass from the Laplace diagonal, start drawn from the device
    Laplace fit, 300 iterations with the first 100 dropped.  Per problem the pooled mean within 0.25 Laplace sd of the Newton mode,
    the pooled variance within [0.8, 1.25] of the Laplace variance (test_gpu_hmc.py's bars).  The float64 restatement stays inside
    them for this seed: tests/test_hmc_many_cpu.py::test_the_restatement_stays_inside_the_statistical_guard."""
    from beta_cores_amd import samplers
    g = mc.GUARD
    probs, fits = mc.guard_problems()
    res = samplers.logistic_hmc_many(probs, n_samples=g['n_samples'], n_chains=g['c'], step_size=g['step'], n_leapfrog=g['L'],
                                     inv_mass='laplace', rng=np.random.RandomState(g['rng_seed']))
    assert res.fallback == [] and all(r.route == 'small' for r in res)
    mc.check_guard(res, fits, 'device')
    # independent draws: the problems no longer share their random numbers, the same bars hold
    ind = samplers.logistic_hmc_many(probs, n_samples=g['n_samples'], n_chains=g['c'], step_size=g['step'], n_leapfrog=g['L'],
                                     inv_mass='laplace', rng=np.random.RandomState(g['rng_seed']), draws='independent')
    mc.check_guard(ind, fits, 'device, independent draws')
