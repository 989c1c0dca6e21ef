"""The chain summary on the device (include/beta_cores_diag.h; kernels k_diag_keep, k_diag_seq, k_diag_cov, k_diag_cov_reduce of
beta_cores_amd/csrc/bc_diag.hip) against the long-double restatement and the derived bounds of tests/diag_cases.py:

1. stand-alone, on the shapes and planted coordinates of diag_cases.SHAPES; ESS and R-hat as functions of the device's own rho
   and moments, so that the truncation index is decided by the numbers the device used;
2. max_lag = 1, 2, h - 1 and beyond (clipped);
3. a problem's bits alone, first, last and in the middle of a batch;
4. attached to a batched sampler run: bit-equal across chunkings, to chain_summary of the returned samples, and with no sample
   copied; the scores keep their bits;
5. marked problems, in the run and stand-alone;
6. the busy table and the refusals of the attached calls, the context free again after each.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import diag_cases as DC                                                          # noqa: E402
import hmc_cases as hc                                                           # noqa: E402

pytestmark = pytest.mark.gpu
FIELDS = ('mean', 'cov', 'rhat', 'ess', 'ess_truncated', 'rho', 'moments')


@pytest.fixture(scope='module')
def bc():
    import beta_cores_amd as bc
    bc.default_context()
    return bc


def _as_case(s):
    """a ChainSummary of one problem (with seams) as the dict diag_cases checks"""
    return dict(mean=s.mean, cov=s.cov, rhat=s.rhat, ess=s.ess, truncated=s.ess_truncated.astype(np.int64), rho=s.rho.T,
                W=s.moments[:, 0], varplus=s.moments[:, 1])


def _same(a, b, what):
    for k in FIELDS:
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None) == (y is None), (what, k)
        if x is not None:
            assert np.array_equal(x, y, equal_nan=True), '%s: %s differs' % (what, k)


# ------------------------------------------------------------------ 1. stand-alone against the cases
@pytest.mark.parametrize('shape', DC.SHAPES, ids=lambda s: 'x'.join(str(k) for k in s))
def test_stand_alone_follows_the_restatement(bc, shape):
    P, n, c, d = shape
    x = DC.make_batch(shape)
    got = bc.samplers.chain_summary(x, seams=True)
    assert got.status.shape == (P,) and not got.status.any()
    for p in range(P):
        g = _as_case(got.problem(p))
        what = 'device %r problem %d' % (shape, p)
        DC.check_against_reference(g, x[p], None, what)
        DC.check_own(g, n, c, what)
        assert np.array_equal(g['cov'], g['cov'].T), what
        for j, kind in DC.planted_kinds(p, d).items():
            if kind == 'const':
                assert np.isnan(g['rhat'][j]) and np.isnan(g['ess'][j]) and not g['cov'][j].any() and not g['cov'][:, j].any(), (what, j)
                assert g['mean'][j] == x[p, 0, 0, j]
            elif kind == 'big':
                assert abs(g['mean'][j] - 1e8) < 1. and 0.3 < g['cov'][j, j] < 3., (what, j)
            elif kind == 'anti':
                assert np.isnan(g['ess'][j]) and g['truncated'][j] == 0 and np.isnan(g['rho'][2:, j]).all(), (what, j)
            elif kind == 'ar9' and n == 64:
                assert g['truncated'][j] == 1 and np.isfinite(g['ess'][j]) and not np.isnan(g['rho'][:, j]).any(), (what, j)
            elif kind == 'shift' and 2 <= c <= 16:
                assert g['rhat'][j] > 1.5, (what, j)
    one = bc.samplers.chain_summary(x[P - 1], seams=True)      # n x C x D: the same problem, unbatched arrays
    assert one.mean.shape == (d,) and one.cov.shape == (d, d) and one.status == 0
    _same(one, got.problem(P - 1), 'a single problem')


# ------------------------------------------------------------------ 2. max_lag
def test_max_lag_gives_the_documented_lags_and_flags(bc):
    n, c, d = 64, 4, 9
    h = n // 2
    x = DC.make_problem(2, n, c, d)
    for lag, L in ((1, 1), (2, 2), (h - 1, h - 1), (h + 5, h - 1), (10 ** 12, h - 1)):
        got = bc.samplers.chain_summary(x, max_lag=lag, seams=True)
        g = _as_case(got)
        assert g['rho'].shape == (L + 1, d)
        ref = DC.check_against_reference(g, x, lag, 'device max_lag %d' % lag)
        DC.check_own(g, n, c, 'device max_lag %d' % lag)
        assert ref['L'] == L and np.array_equal(g['truncated'], ref['truncated'])
    _same(bc.samplers.chain_summary(x, max_lag=h - 1, seams=True), bc.samplers.chain_summary(x, seams=True), 'the default is every lag')
    for bad in (0, -3):
        with pytest.raises(ValueError):
            bc.samplers.chain_summary(x, max_lag=bad)
    with pytest.raises(ValueError):
        bc.samplers.chain_summary(x[:3])                       # n = 3


# ------------------------------------------------------------------ 3. batch independence
def test_a_problems_bits_do_not_depend_on_its_batch(bc):
    n, c, d = 37, 3, 17
    batch = np.stack([DC.make_problem(p, n, c, d, seed=3) for p in range(7)])
    x = batch[3]
    alone = bc.samplers.chain_summary(x, seams=True)
    for at in (0, 6, 2):
        b = batch.copy()
        b[at] = x
        _same(bc.samplers.chain_summary(b, seams=True).problem(at), alone, 'place %d of 7' % at)


# ------------------------------------------------------------------ 4. attached against stand-alone
def _problems(d, sizes=(1, 7, 19, 33, 40), seed=61):
    rng = np.random.RandomState(seed + d)
    return [(hc.make_data(m, d, seed + m)[0], 0.5 + rng.rand(m)) for m in sizes]


class _Tape:
    """A stream whose draws do not depend on how the iterations are cut into chunks: randn(k, C, D) and rand(k, C) hand out the
    next k iterations of two arrays drawn once (logistic_hmc_many asks for nothing else when start is given)."""

    def __init__(self, seed, total, c, d):
        rng = np.random.RandomState(seed)
        self.e, self.u, self.at_e, self.at_u = rng.randn(total, c, d), rng.rand(total, c), 0, 0

    def randn(self, k, c, d):
        self.at_e += k
        return self.e[self.at_e - k:self.at_e].copy()

    def rand(self, k, c):
        self.at_u += k
        return self.u[self.at_u - k:self.at_u].copy()


@pytest.mark.parametrize('d', [9, 128])
def test_attached_summary_equals_the_stand_alone_one(bc, d):
    c, n = 4, 24
    probs = _problems(d)
    rng = np.random.RandomState(7)
    held = bc.samplers.HeldOut(rng.randn(50, d), np.where(rng.rand(50) < 0.5, 1., -1.))
    kw = dict(n_samples=n, n_chains=c, step_size=0.03, n_leapfrog=3, start=0.1 * rng.randn(c, d), warmup=6, adapt_every=3)
    plain = bc.samplers.logistic_hmc_many(probs, rng=_Tape(11, n + 6, c, d), chunk=7, **kw)
    first = None
    for chunk in (1, 7, 24):
        res = bc.samplers.logistic_hmc_many(probs, rng=_Tape(11, n + 6, c, d), chunk=chunk, summary=True, **kw)
        for p, r in enumerate(res):
            assert r.route == 'small' and np.array_equal(r.samples, plain[p].samples) and np.array_equal(r.accept, plain[p].accept)
            _same(r.summary, bc.samplers.chain_summary(r.samples), 'chunks of %d, problem %d against chain_summary' % (chunk, p))
            assert r.summary.status == 0 and np.isfinite(r.summary.mean).all()
        if first is None:
            first = res
        for a, b in zip(first, res):
            _same(a.summary, b.summary, 'chunks of %d against chunks of 1' % chunk)
    scored = bc.samplers.logistic_hmc_many(probs, rng=_Tape(11, n + 6, c, d), chunk=7, score=held, keep_samples=False, **kw)
    lean = bc.samplers.logistic_hmc_many(probs, rng=_Tape(11, n + 6, c, d), chunk=7, score=held, keep_samples=False, summary=True, **kw)
    alone = bc.samplers.logistic_hmc_many(probs, rng=_Tape(11, n + 6, c, d), chunk=7, keep_samples=False, summary=True, **kw)
    for p in range(len(probs)):
        assert lean[p].samples is None and alone[p].samples is None and scored[p].summary is None
        _same(lean[p].summary, first[p].summary, 'no samples copied, problem %d' % p)
        _same(alone[p].summary, first[p].summary, 'summary alone, problem %d' % p)
        assert np.array_equal(lean[p].correct, scored[p].correct) and np.array_equal(lean[p].test_ll, scored[p].test_ll)
        assert np.array_equal(lean[p].logjoint, plain[p].logjoint) and np.array_equal(alone[p].accept, plain[p].accept)


def test_logistic_hmc_carries_a_summary(bc):
    Z, w = hc.make_data(40, 6, 31)
    rng = np.random.RandomState(3)
    kw = dict(n_samples=12, n_chains=3, step_size=0.05, n_leapfrog=3, start=0.1 * rng.randn(3, 6))
    a = bc.samplers.logistic_hmc(Z, w, rng=np.random.RandomState(5), **kw)
    b = bc.samplers.logistic_hmc(Z, w, rng=np.random.RandomState(5), summary=True, max_lag=2, **kw)
    assert a.summary is None and np.array_equal(a.samples, b.samples)
    _same(b.summary, bc.samplers.chain_summary(b.samples, max_lag=2), 'logistic_hmc')


# ------------------------------------------------------------------ 5. marked problems
def test_marked_problems_are_marked_alone(bc):
    from beta_cores_amd import _native as N
    d, c, n = 9, 4, 8
    probs = _problems(d, sizes=(5, 12, 3, 20))
    rng = np.random.RandomState(21)
    starts = 0.1 * rng.randn(len(probs), c, d)
    starts[2, 1, 4] = np.inf                                   # problem 2 is marked by the sampler at the start
    eng = bc.samplers._DeviceHMCMany(bc.default_context(), probs)
    eng.begin(starts, np.ones((len(probs), d)), 3, n)
    try:
        eng.attach_summary(n, None)
        e, u = rng.randn(n, c, d), np.log(rng.rand(n, c))
        s, lj, acc, status = eng.chunk(e, u, np.full(len(probs), 0.03), True, fold=True)
        got = eng.summary_end(seams=True)
    finally:
        eng.end()
    assert list(status) == [0, 0, N.BC_NUMERICAL_PRECISION, 0] and list(got.status) == list(status)
    for k in ('mean', 'cov', 'rhat', 'ess', 'rho', 'moments'):
        assert np.isnan(getattr(got, k)[2]).all(), k            # (as the arrays were handed in: untouched)
    assert not got.ess_truncated[2].any()
    for p in (0, 1, 3):
        _same(got.problem(p), bc.samplers.chain_summary(s[p], seams=True), 'beside a marked problem, %d' % p)
    # stand-alone: a NaN sample marks its own problem only
    x = DC.make_batch((4, 12, 3, 17))
    clean = bc.samplers.chain_summary(x, seams=True)
    x[1, 7, 2, 16] = np.nan
    got = bc.samplers.chain_summary(x, seams=True)
    assert list(got.status) == [0, N.BC_NUMERICAL_PRECISION, 0, 0] and np.isnan(got.mean[1]).all() and np.isnan(got.cov[1]).all()
    for p in (0, 2, 3):
        _same(got.problem(p), clean.problem(p), 'beside a NaN sample, %d' % p)


# ------------------------------------------------------------------ 6. the busy table and the refusals
def test_refusals_leave_the_context_free(bc):
    from beta_cores_amd import _native as N
    lib = N.load()
    ctx = bc.default_context()
    d, c = 9, 2
    probs = _problems(d, sizes=(4, 9))
    rng = np.random.RandomState(33)
    x = DC.make_batch((2, 8, 2, 9))
    want = bc.samplers.chain_summary(x)

    def free():
        _same(bc.samplers.chain_summary(x), want, 'a plain run after a refusal')

    eng = bc.samplers._DeviceHMCMany(ctx, probs)
    draws = lambda k: (rng.randn(k, c, d), np.log(rng.rand(k, c)), np.full(2, 0.03), True)      # noqa: E731
    assert lib.bc_diag_chunk(ctx.h) == N.BC_INVALID_ARGUMENT and lib.bc_diag_attach(ctx.h, 8, 3) == N.BC_INVALID_ARGUMENT      # no run is open
    assert lib.bc_diag_end(ctx.h, *[None] * 8) == N.BC_INVALID_ARGUMENT
    free()
    eng.begin(0.1 * rng.randn(2, c, d), np.ones((2, d)), 2, 9)
    try:
        with pytest.raises(ValueError, match='bc_hmc_small'):
            bc.samplers.chain_summary(x)                       # the stand-alone call while a run is open
        assert lib.bc_diag_attach(ctx.h, 3, 1) == N.BC_INVALID_ARGUMENT      # n_keep < 4
        assert lib.bc_diag_attach(ctx.h, 4, 0) == N.BC_INVALID_ARGUMENT      # max_lag < 1
        assert lib.bc_diag_chunk(ctx.h) == N.BC_INVALID_ARGUMENT            # nothing attached, no chunk pending
        eng.attach_summary(4, None)
        assert lib.bc_diag_attach(ctx.h, 4, 1) == N.BC_INVALID_ARGUMENT      # attached already
        assert lib.bc_diag_chunk(ctx.h) == N.BC_INVALID_ARGUMENT and b'no chunk' in lib.bc_last_error()
        eng.chunk(*draws(3), fold=True)
        out = bc.samplers._SummaryArrays(2, d, 1, False)
        assert lib.bc_diag_end(ctx.h, *out.pointers()) == N.BC_INVALID_ARGUMENT and b'3 of 4' in lib.bc_last_error()
        with pytest.raises(ValueError, match='exceed'):
            eng.chunk(*draws(2), fold=True)                    # 3 + 2 > n_keep: refused, the chunk stays pending and is not folded
        st = np.empty(2, dtype=np.int32)
        s2, l2, a2 = np.empty((2, 2, c, d)), np.empty((2, 2, c)), np.empty((2, 2, c), dtype=np.int32)
        N.call('bc_hmc_small_chunk_end', ctx.h, s2.ctypes.data, l2.ctypes.data, a2.ctypes.data, st.ctypes.data)
        k1 = eng.chunk(*draws(1), fold=True)
        assert lib.bc_diag_chunk(ctx.h) == N.BC_INVALID_ARGUMENT            # the chunk has been ended: none is pending
        eng.end()
        got = eng.summary_end()                                # after the run has been ended
        assert not got.status.any() and np.isfinite(got.mean).all() and k1[0].shape == (2, 1, c, d)
        assert lib.bc_diag_end(ctx.h, *out.pointers()) == N.BC_INVALID_ARGUMENT      # detached
    finally:
        eng.end()
    free()
    # a run of beta_cores_hmc.h is not one the summary attaches to
    Z, w = hc.make_data(30, d, 5)
    dz = bc.DeviceData(Z)
    one = bc.samplers._DeviceHMC(dz, None)
    one.begin(0.1 * rng.randn(c, d), np.ones(d), 2, 4)
    try:
        assert lib.bc_diag_attach(ctx.h, 4, 1) == N.BC_INVALID_ARGUMENT and lib.bc_diag_chunk(ctx.h) == N.BC_INVALID_ARGUMENT
        e2, u2 = rng.randn(2, c, d), np.log(rng.rand(2, c))
        N.call('bc_hmc_chunk_begin', ctx.h, e2.ctypes.data, u2.ctypes.data, 2, 0.03)
        assert lib.bc_diag_chunk(ctx.h) == N.BC_INVALID_ARGUMENT
        with pytest.raises(ValueError, match='bc_hmc '):
            bc.samplers.chain_summary(x)
    finally:
        one.end()
    free()
