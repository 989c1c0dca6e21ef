"""The state the fused VI gradient keeps on a context between calls (csrc/bc_vigrad.hip: the two cached Phis of the coreset
rows, the result buffer and its pinned landing area, the side stream, the phase clock, what is pending), through the projector
where that reaches and through the C ABI where it does not.  A pin of what the library does, bit for bit: every result is
compared with the same call on a context that has done nothing else.

1. Buffers that grow, shrink and change shape on one context, the three kinds of gradient in turn.
2. The instrumented route (timing on: one stream) against the usual one (the coreset rows beside the data rows), and the
   phase clock's reads.
3. A refused _begin leaves nothing pending and nothing changed.
4. A context's first use: the clock, the three _ends, and bc_ctx_destroy before and after the first gradient.

300 rows (two full tiles and a ragged one), d = 6, three models: linear regression (rows [x, y]), logistic regression, and a
Gaussian with a non-identity Siginv (the one model that uses both row-aux scratches)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_ROWS, D = 300, 6
MODELS = ('linreg', 'logistic', 'gauss')
KINDS = ('plain', 'beta', 'psvi')
BETA = {'linreg': 0.3, 'logistic': 0.2, 'gauss': 0.5}
SCALE = 1.7


@pytest.fixture(scope='module')
def bc():
    import beta_cores_amd as bc
    bc.default_context()
    return bc


def _native():
    from beta_cores_amd import _native as N
    from beta_cores_amd.device import _ptr
    return N, _ptr


def _model(bc, name):
    if name == 'linreg':
        return bc.likelihoods.LinearRegression(1.3, beta_gradient=True)
    if name == 'logistic':
        return bc.likelihoods.LogisticRegression(beta_gradient=True)
    A = np.random.RandomState(5).randn(D, D) * 0.3
    Sig = A.dot(A.T) + np.eye(D)
    Siginv = np.linalg.inv(Sig)
    assert np.abs(Siginv - np.diag(np.diag(Siginv))).max() > 1e-3          # not the identity, not diagonal
    return bc.likelihoods.GaussianLocation(Siginv, np.linalg.slogdet(Sig)[1])


def _rows(name):
    rng = np.random.RandomState(11 + MODELS.index(name))
    return np.ascontiguousarray(rng.randn(N_ROWS, D + (name == 'linreg')))


def _theta(s):
    return np.random.RandomState(100 + s).randn(s, D) * 0.3


def _weights(m):
    return np.random.RandomState(200 + m).uniform(0., 3., m)


class _Site:
    """A context of its own with one model's 300 rows resident on it."""

    def __init__(self, bc, name, ctx=None):
        from beta_cores_amd.device import Context
        self.bc, self.name, self.ctx = bc, name, ctx or Context()
        self.model = _model(bc, name)
        self.Z = _rows(name)
        self.dd = bc.DeviceData(self.Z, ctx=self.ctx)

    def grad(self, kind, m, s):
        """One gradient of `kind` over the first m rows as the coreset and s samples, through the projector: (grad, resid) |
        (grad, beta_dots, resid) | (grad_w, grad_p, resid)."""
        bc, th = self.bc, _theta(s)
        core, w = np.ascontiguousarray(self.Z[:m]), _weights(m)
        if kind == 'beta':
            prj = bc.DeviceBetaProjector(lambda n, wts, pts: th, s, self.model, ctx=self.ctx)
            out = prj.vi_gradient(self.dd, core, w, SCALE, beta=BETA[self.name], want_resid=True, want_beta_grad=True)
        else:
            prj = bc.DeviceProjector(lambda n, wts, pts: th, s, self.model, ctx=self.ctx)
            out = prj.vi_gradient(self.dd, core, w, SCALE, want_resid=True) if kind == 'plain' \
                else prj.psvi_gradient(self.dd, core, w, SCALE, want_resid=True)
        assert out is not None and len(out) == (2 if kind == 'plain' else 3)
        assert all(np.isfinite(a).all() for a in out)
        return out

    def native_args(self, kind, m, s, n_params_wrong=False):
        """(arrays to keep alive, the arguments of the kind's _begin) for the C ABI"""
        _, _ptr = _native()
        beta = BETA[self.name] if kind == 'beta' else None
        model_id = self.model.beta_model_id if kind == 'beta' else self.model.model_id
        params = np.ascontiguousarray(self.model.params(beta=beta), dtype=np.float64)
        if n_params_wrong:
            params = np.concatenate((params, [1.]))
        th, core, w = _theta(s), np.ascontiguousarray(self.Z[:max(m, 1)]), _weights(max(m, 1))
        args = (self.ctx.h, self.dd.h, _ptr(core), m, int(model_id), _ptr(th), s, _ptr(params), int(params.shape[0]), _ptr(w), SCALE)
        return (th, core, w, params), args + (() if kind == 'psvi' else (None,))


ENTRY = {'plain': 'bc_vi_gradient', 'beta': 'bc_vi_beta_gradient', 'psvi': 'bc_psvi_gradient'}


def _ends_are_refused(ctx):
    """each of the three _ends says that nothing is pending"""
    N, _ptr = _native()
    g, x, r = np.empty(512), np.empty(512 * (D + 1)), np.empty(256)
    for kind in KINDS:
        args = (ctx.h, _ptr(g), _ptr(r)) if kind == 'plain' else (ctx.h, _ptr(g), _ptr(x), _ptr(r))
        with pytest.raises(ValueError, match='%s_end: no gradient is pending on this context' % ENTRY[kind]):
            N.call(ENTRY[kind] + '_end', *args)


_fresh_results = {}


def _fresh(bc, name, kind, m, s):
    """the call on a context that has done nothing else (one per distinct call for the whole module; never written to)"""
    key = (name, kind, m, s)
    if key not in _fresh_results:
        out = _Site(bc, name).grad(kind, m, s)
        for a in out:
            a.flags.writeable = False
        _fresh_results[key] = out
    return _fresh_results[key]


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------ 1. buffers that grow, shrink and change shape
# (kind, m, S): 257 is one past the 256 rows the coreset rows' Phi starts with; S = 5 -> 20 rebuilds both cached Phis; (130, 100) is
# the S = 97..100 tail instance of K1; the beta kind adds the second Phi, the PSVI kind the m x dz block behind grad | resid
SEQUENCE = (('plain', 3, 5), ('plain', 257, 5), ('plain', 3, 5), ('plain', 3, 20), ('plain', 130, 100), ('beta', 7, 20),
            ('psvi', 7, 20), ('plain', 3, 5))


@pytest.mark.parametrize('name', MODELS)
def test_buffers_grow_shrink_and_change_shape_on_one_context(bc, name):
    site = _Site(bc, name)
    for step, (kind, m, s) in enumerate(SEQUENCE):
        if kind == 'psvi' and not site.model.has_grad_x:
            continue
        got, want = site.grad(kind, m, s), _fresh(bc, name, kind, m, s)
        assert _same(got, want), (name, step, kind, m, s, [np.array_equal(x, y) for x, y in zip(got, want)])


# ------------------------------------------------------------------ 2. the instrumented route
@pytest.mark.parametrize('name', MODELS)
def test_instrumented_route_has_the_bits_of_the_side_stream_route_and_a_clock(bc, name):
    timed = _Site(bc, name)
    timed.ctx.enable_timing(1)
    kinds = [k for k in KINDS if k != 'psvi' or timed.model.has_grad_x]
    for kind in kinds:
        got, want = timed.grad(kind, 7, 20), _fresh(bc, name, kind, 7, 20)      # (a fresh context: timing off, the side stream)
        assert _same(got, want), (name, kind)
    first = timed.ctx.phase_times(reset=False)
    ms, calls = first
    assert list(ms) == list(timed.ctx.VI_PHASES) and len(ms) == 5
    assert all(np.isfinite(v) and v >= 0. for v in ms.values()), ms
    assert calls == len(kinds)
    assert timed.ctx.phase_times(reset=True) == first                           # the read that resets returns the same
    assert timed.ctx.phase_times() == (dict.fromkeys(timed.ctx.VI_PHASES, 0.), 0)
    # timing on again: counted from zero; then off: not counted, and the bits are still the same
    assert _same(timed.grad('plain', 7, 20), _fresh(bc, name, 'plain', 7, 20))
    assert timed.ctx.phase_times(reset=False)[1] == 1
    timed.ctx.enable_timing(0)
    for kind in kinds:
        assert _same(timed.grad(kind, 7, 20), _fresh(bc, name, kind, 7, 20)), (name, kind)
    ms, calls = timed.ctx.phase_times()
    assert calls == 1 and all(np.isfinite(v) and v >= 0. for v in ms.values())
    assert timed.ctx.phase_times() == (dict.fromkeys(timed.ctx.VI_PHASES, 0.), 0)


# ------------------------------------------------------------------ 3. a refused begin
@pytest.mark.parametrize('name', MODELS)
def test_a_refused_begin_leaves_nothing_behind(bc, name):
    N, _ = _native()
    site = _Site(bc, name)
    refused = (('plain', 3, 257, False), ('plain', 0, 5, False), ('beta', 3, 5, True))      # S = 257 | m = 0 | a wrong n_params
    for used in (False, True):                       # on a context that has allocated nothing yet, then on one that has
        for kind, m, s, wrong in refused:
            keep, args = site.native_args(kind, m, s, n_params_wrong=wrong)
            with pytest.raises(ValueError):
                N.call(ENTRY[kind] + '_begin', *args)
            _ends_are_refused(site.ctx)
            del keep
        assert _same(site.grad('plain', 3, 5), _fresh(bc, name, 'plain', 3, 5)), (name, used)
        assert _same(site.grad('beta', 7, 20), _fresh(bc, name, 'beta', 7, 20)), (name, used)
    assert site.ctx.phase_times() == (dict.fromkeys(site.ctx.VI_PHASES, 0.), 0)


# ------------------------------------------------------------------ 4. first use
def test_first_use_of_a_context(bc):
    from beta_cores_amd.device import Context
    N, _ptr = _native()
    # never took a gradient: the clock reads zeros, the three _ends are refused, and it is destroyed without error
    ctx = Context()
    assert ctx.phase_times(reset=False) == (dict.fromkeys(ctx.VI_PHASES, 0.), 0)
    _ends_are_refused(ctx)
    assert ctx.phase_times() == (dict.fromkeys(ctx.VI_PHASES, 0.), 0)
    assert ctx._fin() == N.BC_OK
    ctx = Context()                                  # (nothing at all was called on this one)
    assert ctx._fin() == N.BC_OK
    # _begin and _end ran once (the side stream exists and has run): destroyed without error
    site = _Site(bc, 'gauss')
    keep, args = site.native_args('plain', 7, 20)
    g, r = np.full(7, 7.), np.full(20, 7.)
    N.call('bc_vi_gradient_begin', *args)
    N.call('bc_vi_gradient_end', site.ctx.h, _ptr(g), _ptr(r))
    assert _same((g, r), _fresh(bc, 'gauss', 'plain', 7, 20))                  # (the C ABI and the projector: the same call)
    assert site.dd._fin() == N.BC_OK
    assert site.ctx._fin() == N.BC_OK
    del keep
    # a pending gradient that is never fetched: the context is destroyed without error all the same
    site = _Site(bc, 'linreg')
    keep, args = site.native_args('beta', 7, 20)
    N.call('bc_vi_beta_gradient_begin', *args)
    assert site.ctx._fin() == N.BC_OK
    assert site.dd._fin() == N.BC_OK
    del keep
    # and the device is as it was: the next context computes what every fresh one does
    assert _same(_Site(bc, 'gauss').grad('plain', 7, 20), _fresh(bc, 'gauss', 'plain', 7, 20))
