"""What may be open on a context at once, and the buffers the chunked device runs keep between runs, through the C ABI
(bc_vi_optimize_*, bc_hmc_*, bc_hmc_small_*, bc_psvi_many_*, the fused gradients' _begin / _end).

1. The table of csrc/bc_core.hip (bc_ctx_refuse_busy): with a holder open -- G a pending gradient (csrc/bc_vigrad.hip), V / H / S / B an open
   bc_vi_optimize / bc_hmc / bc_hmc_small / bc_psvi_many run -- every entrant is refused with the holder named, or allowed and closed at once;
   the holder then finishes with the bits of the same run on an undisturbed context.
2. Buffers that grow and are reused at a smaller size: small run, larger run in two chunks, small run again, on one context.
3. A chunk that is abandoned (_chunk_begin, then _end) leaves the context fit for the next run, and the run's clock running.
"""
import ctypes
import math

import numpy as np
import pytest

import hmc_cases as hc
import hmc_many_cases as mc
import test_gpu_hmc as t_hmc
import test_gpu_hmc_many as t_many

pytestmark = pytest.mark.gpu

M, S = 6, 8                         # the coreset rows and samples of the gradient and of the weight optimisation
LOGISTIC_LL, LOGISTIC_BETA, SAMPLER_LOGISTIC = 2, 3, 2


@pytest.fixture(scope='module')
def bc():
    import beta_cores_amd as bc
    bc.default_context()
    return bc


def _p(x):
    return None if x is None else x.ctypes.data_as(ctypes.c_void_p)


def _lib():
    from beta_cores_amd import _native as N
    return N, N.load()


class _Site:
    """A context with the 40 x 6 rows (and their weights) resident on it: where the runs below take place."""

    def __init__(self, bc, ctx=None):
        from beta_cores_amd.device import Context
        self.bc, self.ctx = bc, ctx or Context()
        self.h = self.ctx.h
        self.Z, self.w = hc.make_data(40, 6, 31)
        self.dz = bc.DeviceData(self.Z, ctx=self.ctx)
        self.wd = bc.DeviceData(self.w.reshape(-1, 1), ctx=self.ctx)


def _hmc_case(site, c=3, T=2, L=2, seed=131):
    rng = np.random.RandomState(seed + c + T)
    d = site.Z.shape[1]
    return dict(Z=site.Z, w=site.w, start=rng.randn(c, d) * 0.1, inv_mass=0.5 + rng.rand(d), eps=0.1, L=L, E=rng.randn(T, c, d),
                logU=np.log(rng.rand(T, c)))


def _hmc_run(site, case, chunks=None):
    st, s, lj, acc = t_hmc._native_run(site.bc, site.dz, site.wd, case, chunks=chunks)
    assert st == 0
    return s, lj, acc


def _small_run(site, problems, chunks=None):
    """test_gpu_hmc_many's run, on the site's context in the place of the default one."""
    from beta_cores_amd import device
    old = device.default_context()
    device.set_default_context(site.ctx)
    try:
        st, got = t_many._native_run(site.bc, problems, chunks=chunks)
    finally:
        device.set_default_context(old)
    assert st == 0 and all(g['status'] == 0 for g in got)
    return [(g['samples'], g['logjoint'], g['accept']) for g in got]


def _grad_args(site):
    d = site.Z.shape[1]
    keep = [np.ascontiguousarray(site.Z[:M]), np.zeros((S, d)), np.ones(M)]
    return keep, (site.h, site.dz.h, _p(keep[0]), M, LOGISTIC_LL, _p(keep[1]), S, None, 0, _p(keep[2]), 1., None)


def _opt_problem(site, m=M, s=S, itrs=2):
    d = site.Z.shape[1]
    i = np.arange(itrs)
    steps = np.ascontiguousarray(np.vstack((np.full(itrs, 0.05), 1. - 0.9 ** (i + 1), 1. - 0.999 ** (i + 1))))
    return dict(core=np.ascontiguousarray(site.Z[:m]), w0=np.ones(m), sp=np.zeros(d + 1), steps=steps, m=m, s=s, itrs=itrs,
                E=np.random.RandomState(m + s + itrs).randn(itrs, s, d))


def _opt_begin(site, a):
    _, lib = _lib()
    return lib.bc_vi_optimize_begin(site.h, site.dz.h, _p(a['core']), a['m'], LOGISTIC_LL, None, 0, SAMPLER_LOGISTIC, _p(a['sp']), a['s'],
                                    _p(a['w0']), a['itrs'], _p(a['steps']), 0, 1., 0)


def _opt_finish(site, a, chunks=None):
    N, lib = _lib()
    i0 = 0
    for k in (chunks or [a['itrs']]):
        assert lib.bc_vi_optimize_chunk_begin(site.h, _p(a['E'][i0:i0 + k]), None, k) == N.BC_OK, N.last_error()
        assert lib.bc_vi_optimize_chunk_end(site.h) == N.BC_OK, N.last_error()
        i0 += k
    out = np.full(a['m'], 7.)
    assert lib.bc_vi_optimize_end(site.h, _p(out), None) == N.BC_OK, N.last_error()
    return (out,)


def _opt_run(site, a, chunks=None):
    N, _ = _lib()
    assert _opt_begin(site, a) == N.BC_OK, N.last_error()
    return _opt_finish(site, a, chunks)


def _psvi_case(site, d, s, n_sub, itrs, sizes, seed=171):
    """A batched BatchPSVI run (logistic kind) on 40 rows of width d resident on the site's context: problem p starts at the first
    sizes[p] rows with weights 40 / sizes[p]; all problems share each step's normals and row numbers."""
    rng = np.random.RandomState(seed + d + s + itrs)
    Z = rng.randn(40, d)
    i = np.arange(itrs)
    row_ptr = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    return dict(Z=Z, dd=site.bc.DeviceData(Z, ctx=site.ctx), pts=np.ascontiguousarray(np.vstack([Z[:m] for m in sizes])),
                w0=np.concatenate([np.full(m, 40. / m) for m in sizes]), row_ptr=row_ptr, P=len(sizes), d=d, s=s, n_sub=n_sub, itrs=itrs,
                steps=np.ascontiguousarray(np.tile(0.05 / (1. + i), (len(sizes), 1))),
                moments=np.ascontiguousarray(np.vstack((1. - 0.9 ** (i + 1), 1. - 0.999 ** (i + 1)))),
                E=rng.randn(itrs, s, d), idx=rng.randint(40, size=(itrs, n_sub)).astype(np.int64))


def _psvi_on(site, a):
    """The case with its rows resident on another site's context."""
    return dict(a, dd=site.bc.DeviceData(a['Z'], ctx=site.ctx))


def _psvi_begin(site, a):
    _, lib = _lib()
    return lib.bc_psvi_many_begin(site.h, a['dd'].h, LOGISTIC_LL, SAMPLER_LOGISTIC, 0, _p(a['pts']), _p(a['w0']), _p(a['row_ptr']), a['P'], None,
                                  a['s'], a['itrs'], _p(a['steps']), _p(a['moments']), a['n_sub'], 40. / a['n_sub'])


def _psvi_finish(site, a, chunks=None):
    N, lib = _lib()
    i0 = 0
    for k in (chunks or [a['itrs']]):
        assert lib.bc_psvi_many_chunk_begin(site.h, _p(a['E'][i0:i0 + k]), _p(a['idx'][i0:i0 + k]), k) == N.BC_OK, N.last_error()
        assert lib.bc_psvi_many_chunk_end(site.h, None) == N.BC_OK, N.last_error()
        i0 += k
    R = int(a['row_ptr'][-1])
    w, pts, modes, status = np.full(R, 7.), np.full((R, a['d']), 7.), np.full((a['P'], a['d']), 7.), np.full(a['P'], 7, dtype=np.int32)
    assert lib.bc_psvi_many_end(site.h, _p(w), _p(pts), _p(modes), _p(status)) == N.BC_OK and not status.any(), (N.last_error(), status)
    return w, pts, modes


def _psvi_run(site, a, chunks=None):
    N, _ = _lib()
    assert _psvi_begin(site, a) == N.BC_OK, N.last_error()
    return _psvi_finish(site, a, chunks)


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------ 1. the table
# holder: (the substring every refusal by it carries, the entrants' own wording when they are of its kind)
HOLDERS = {'G': ('pending', 'already pending'), 'V': ('optimi', 'already open'), 'H': ('bc_hmc_end', 'already open'),
           'S': ('bc_hmc_small_end', 'already open'), 'B': ('bc_psvi_many_end', 'already open')}
# entrant: (its own kind or None, the holders that let it in)
ENTRANTS = {'bc_vi_gradient_begin': ('G', 'V'), 'bc_vi_beta_gradient_begin': ('G', 'V'), 'bc_psvi_gradient_begin': ('G', 'V'),
            'bc_vi_optimize_begin': ('V', ''), 'bc_hmc_begin': ('H', ''), 'bc_logistic_logjoint_batch': (None, 'GVB'),
            'bc_hmc_small_begin': ('S', ''), 'bc_hmc_small_logjoint': ('S', ''), 'bc_psvi_many_begin': ('B', '')}


def _entrants(site, small):
    """name -> a call that returns the entrant's status and, where it was let in, closes it at once with its own _end."""
    N, lib = _lib()
    h, d = site.h, site.Z.shape[1]
    keep, grad_args = _grad_args(site)
    beta = np.array([0.5])
    g, r, gp = np.empty(M), np.empty(S), np.empty((M, d))
    opt = _opt_problem(site)
    case = _hmc_case(site)
    start, im = np.ascontiguousarray(case['start']), np.ascontiguousarray(case['inv_mass'])
    c = start.shape[0]
    val, grad = np.empty(c), np.empty((c, d))
    rows, w, row_ptr, sstart, sim, _ = mc.pack(small)
    P, sc, sd = sstart.shape
    sval, sgrad = np.empty((P, sc)), np.empty((P, sc, sd))
    psvi = _psvi_case(site, 3, 2, 5, 1, (1, 2))
    keep += [beta, g, r, gp, opt, start, im, val, grad, rows, w, row_ptr, sstart, sim, sval, sgrad, psvi]

    def closing(st, end):
        if st == N.BC_OK:
            assert end() == N.BC_OK, N.last_error()
        return st
    calls = {
        'bc_vi_gradient_begin': lambda: closing(lib.bc_vi_gradient_begin(*grad_args), lambda: lib.bc_vi_gradient_end(h, _p(g), _p(r))),
        'bc_vi_beta_gradient_begin': lambda: closing(
            lib.bc_vi_beta_gradient_begin(h, site.dz.h, _p(keep[0]), M, LOGISTIC_BETA, _p(keep[1]), S, _p(beta), 1, _p(keep[2]), 1., None),
            lambda: lib.bc_vi_beta_gradient_end(h, _p(g), _p(np.empty(M)), _p(r))),
        'bc_psvi_gradient_begin': lambda: closing(
            lib.bc_psvi_gradient_begin(h, site.dz.h, _p(keep[0]), M, LOGISTIC_LL, _p(keep[1]), S, None, 0, _p(keep[2]), 1.),
            lambda: lib.bc_psvi_gradient_end(h, _p(g), _p(gp), _p(r))),
        'bc_vi_optimize_begin': lambda: closing(_opt_begin(site, opt), lambda: lib.bc_vi_optimize_end(h, None, None)),
        'bc_hmc_begin': lambda: closing(lib.bc_hmc_begin(h, site.dz.h, site.wd.h, _p(start), c, _p(im), 2, 2), lambda: lib.bc_hmc_end(h)),
        'bc_logistic_logjoint_batch': lambda: lib.bc_logistic_logjoint_batch(h, site.dz.h, site.wd.h, _p(start), c, _p(val), _p(grad)),
        'bc_hmc_small_begin': lambda: closing(
            lib.bc_hmc_small_begin(h, _p(rows), _p(w), _p(row_ptr), P, sd, _p(sstart), sc, _p(sim), 4, 6), lambda: lib.bc_hmc_small_end(h)),
        'bc_hmc_small_logjoint': lambda: lib.bc_hmc_small_logjoint(h, _p(rows), _p(w), _p(row_ptr), P, sd, _p(sstart), sc, _p(sval), _p(sgrad)),
        'bc_psvi_many_begin': lambda: closing(_psvi_begin(site, psvi), lambda: lib.bc_psvi_many_end(h, None, None, None, None)),
    }
    return calls, keep


@pytest.fixture(scope='module')
def shared_site(bc):
    return _Site(bc)


@pytest.mark.parametrize('holder', ['G', 'V', 'H', 'S', 'B'])
def test_the_table(bc, shared_site, holder):
    N, lib = _lib()
    site, fresh = shared_site, _Site(bc)
    small = mc.make_batch_case('ragged5')['problems'][:3]
    case, opt = _hmc_case(site), _opt_problem(site)
    E, U = np.ascontiguousarray(case['E']), np.ascontiguousarray(case['logU'])
    T, c, d = E.shape

    def grad_open(st):
        kept, args = _grad_args(st)
        assert lib.bc_vi_gradient_begin(*args) == N.BC_OK, N.last_error()

        def grad_finish():
            g, r = np.full(M, 7.), np.full(S, 7.)
            assert lib.bc_vi_gradient_end(st.h, _p(g), _p(r)) == N.BC_OK, (N.last_error(), len(kept))
            return g, r
        return grad_finish
    # the undisturbed run, then the holder opened on the shared context
    if holder == 'G':
        want = grad_open(fresh)()
        finish = grad_open(site)
    elif holder == 'V':
        want = _opt_run(fresh, opt)
        assert _opt_begin(site, opt) == N.BC_OK, N.last_error()
        finish = lambda: _opt_finish(site, opt)
    elif holder == 'H':
        want = _hmc_run(fresh, case)
        start, im = np.ascontiguousarray(case['start']), np.ascontiguousarray(case['inv_mass'])
        assert lib.bc_hmc_begin(site.h, site.dz.h, site.wd.h, _p(start), c, _p(im), case['L'], T) == N.BC_OK, N.last_error()

        def finish():
            s, lj, acc = np.full((T, c, d), 7.), np.full((T, c), 7.), np.full((T, c), 7, dtype=np.int32)
            assert lib.bc_hmc_chunk_begin(site.h, _p(E), _p(U), T, case['eps']) == N.BC_OK, N.last_error()
            assert lib.bc_hmc_chunk_end(site.h, _p(s), _p(lj), _p(acc)) == N.BC_OK and lib.bc_hmc_end(site.h) == N.BC_OK
            return s, lj, acc
    elif holder == 'B':
        held = _psvi_case(site, 5, 8, 33, 2, (1, 16, 17))
        want = _psvi_run(fresh, _psvi_on(fresh, held))
        assert _psvi_begin(site, held) == N.BC_OK, N.last_error()
        finish = lambda: _psvi_finish(site, held)
    else:
        want = sum(_small_run(fresh, small), ())
        rows, w, row_ptr, sstart, sim, eps = mc.pack(small)
        P, sc, sd = sstart.shape
        sE, sU, sT = np.ascontiguousarray(small[0]['E']), np.ascontiguousarray(small[0]['logU']), small[0]['E'].shape[0]
        assert lib.bc_hmc_small_begin(site.h, _p(rows), _p(w), _p(row_ptr), P, sd, _p(sstart), sc, _p(sim), small[0]['L'], sT) == N.BC_OK

        def finish():
            s, lj, acc = np.full((P, sT, sc, sd), 7.), np.full((P, sT, sc), 7.), np.full((P, sT, sc), 7, dtype=np.int32)
            status = np.full(P, 7, dtype=np.int32)
            assert lib.bc_hmc_small_chunk_begin(site.h, _p(sE), _p(sU), 0, sT, _p(eps)) == N.BC_OK, N.last_error()
            assert lib.bc_hmc_small_chunk_end(site.h, _p(s), _p(lj), _p(acc), _p(status)) == N.BC_OK and not status.any()
            assert lib.bc_hmc_small_end(site.h) == N.BC_OK
            return sum(((s[p], lj[p], acc[p]) for p in range(P)), ())
    calls, keep = _entrants(site, small)
    named, own_words = HOLDERS[holder]
    for name, (own, let_in) in ENTRANTS.items():
        st = calls[name]()
        if holder in let_in:
            assert st == N.BC_OK, (holder, name, N.last_error())
            continue
        msg = N.last_error()
        assert st == N.BC_INVALID_ARGUMENT and named in msg, (holder, name, st, msg)
        if own == holder:
            assert own_words in msg, (holder, name, msg)
    got = finish()
    assert _same(got, want), (holder, [np.array_equal(x, y) for x, y in zip(got, want)])
    del keep


# ------------------------------------------------------------------ 2. buffers that regrow
def _runs(kind, site):
    """(small, large) of a kind as calls on `site`: the large one in a chunk of 3 and a chunk of 1."""
    if kind == 'hmc':
        a, b = _hmc_case(site, c=2, T=1), _hmc_case(site, c=5, T=4)
        return (lambda st: _hmc_run(st, a, [1])), (lambda st: _hmc_run(st, b, [3, 1]))
    if kind == 'hmc_small':
        a = mc.build_batch('regrow1', 5, (7,), 3, 4, 1, 0.25, 51)['problems']
        b = mc.build_batch('regrow3', 5, (1, 64, 65), 3, 4, 4, 0.25, 52)['problems']
        return (lambda st: sum(_small_run(st, a, [1]), ())), (lambda st: sum(_small_run(st, b, [3, 1]), ()))
    if kind == 'psvi_many':
        # the large run: two full 16-row tiles of gathered rows and one row; problems of one tile, one tile exactly, one row over
        a, b = _psvi_case(site, 3, 2, 5, 1, (1, 2)), _psvi_case(site, 5, 8, 33, 4, (1, 16, 17))
        return (lambda st: _psvi_run(st, _psvi_on(st, a), [1])), (lambda st: _psvi_run(st, _psvi_on(st, b), [3, 1]))
    a, b = _opt_problem(site, m=3, s=4, itrs=1), _opt_problem(site, m=6, s=8, itrs=4)
    return (lambda st: _opt_run(st, a, [1])), (lambda st: _opt_run(st, b, [3, 1]))


@pytest.mark.parametrize('kind', ['hmc', 'hmc_small', 'vi_optimize', 'psvi_many'])
def test_buffers_that_regrow(bc, kind):
    site = _Site(bc)
    small, large = _runs(kind, site)
    for label, run in (('small', small), ('large', large), ('small again', small)):
        got, want = run(site), run(_Site(bc))
        assert _same(got, want), (kind, label)


# ------------------------------------------------------------------ 3. an abandoned chunk
@pytest.mark.parametrize('kind', ['hmc', 'hmc_small', 'vi_optimize', 'psvi_many'])
def test_an_abandoned_chunk(bc, kind):
    N, lib = _lib()
    site = _Site(bc)
    h = site.h
    if kind == 'hmc':
        case = _hmc_case(site)
        T, c, d = case['E'].shape
        start, im = np.ascontiguousarray(case['start']), np.ascontiguousarray(case['inv_mass'])
        E, U = np.ascontiguousarray(case['E']), np.ascontiguousarray(case['logU'])
        assert lib.bc_hmc_begin(h, site.dz.h, site.wd.h, _p(start), c, _p(im), case['L'], T) == N.BC_OK, N.last_error()
        assert lib.bc_hmc_chunk_begin(h, _p(E), _p(U), T, case['eps']) == N.BC_OK and lib.bc_hmc_end(h) == N.BC_OK
        run, clock = (lambda st: _hmc_run(st, case)), lib.bc_hmc_device_ms
    elif kind == 'hmc_small':
        small = mc.make_batch_case('ragged5')['problems'][:3]
        rows, w, row_ptr, start, im, eps = mc.pack(small)
        P, c, d = start.shape
        E, U = np.ascontiguousarray(small[0]['E']), np.ascontiguousarray(small[0]['logU'])
        T = E.shape[0]
        assert lib.bc_hmc_small_begin(h, _p(rows), _p(w), _p(row_ptr), P, d, _p(start), c, _p(im), small[0]['L'], T) == N.BC_OK, N.last_error()
        assert lib.bc_hmc_small_chunk_begin(h, _p(E), _p(U), 0, T, _p(eps)) == N.BC_OK and lib.bc_hmc_small_end(h) == N.BC_OK
        run, clock = (lambda st: sum(_small_run(st, small), ())), lib.bc_hmc_small_device_ms
    elif kind == 'psvi_many':
        a = _psvi_case(site, 5, 8, 33, 2, (1, 16, 17))
        assert _psvi_begin(site, a) == N.BC_OK, N.last_error()
        assert lib.bc_psvi_many_chunk_begin(h, _p(a['E']), _p(a['idx']), a['itrs']) == N.BC_OK and \
            lib.bc_psvi_many_end(h, None, None, None, None) == N.BC_OK
        run, clock = (lambda st: _psvi_run(st, _psvi_on(st, a))), lib.bc_psvi_many_device_ms
    else:
        opt = _opt_problem(site)
        assert _opt_begin(site, opt) == N.BC_OK, N.last_error()
        assert lib.bc_vi_optimize_chunk_begin(h, _p(opt['E']), None, opt['itrs']) == N.BC_OK and lib.bc_vi_optimize_end(h, None, None) == N.BC_OK
        run, clock = (lambda st: _opt_run(st, opt)), lib.bc_vi_optimize_device_ms
    assert _same(run(site), run(_Site(bc))), kind
    ms = ctypes.c_double(-1.)
    assert clock(h, ctypes.byref(ms)) == N.BC_OK and ms.value > 0. and math.isfinite(ms.value)
