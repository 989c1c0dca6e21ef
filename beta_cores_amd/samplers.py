"""Posterior samplers for the greedy-VI coresets: callables `sampler(S, wts, pts) -> S x D` (projector.py:37,66).

The reference's drivers define these as closures over `weighted_post`
(examples/zellner_neural_linear/main.py:119-124, examples/zellner_gaussian/main.py:90-95):

    muw, LSigw, _ = weighted_post(mu0, Sig0inv, sigsq, pts, wts)
    return muw + np.random.randn(n, muw.shape[0]).dot(LSigw.T)

The classes here compute exactly that (K4 on the device for the Gram of the <= M coreset rows, LAPACK on the host for the
D x D Cholesky, the normals from NumPy's legacy stream) and add ONE thing the closures cannot offer: `prefetch()` draws the
normals of the NEXT call ahead of time.  The fused gradient of BetaCoreset / SparseVI (`bc_vi_gradient`) calls it between
enqueueing a gradient on the GPU and waiting for it -- the ~60-120 us of `randn(S, D)` then run beside K1 instead of between
two launches.  The draws come from the same stream in the same order, and a prefetched matrix is always consumed by the very
next call, so the results and the RNG position after a build are the reference's (tests/test_gpu_storefree.py).
"""

import numpy as np

import scipy.linalg as sl
from scipy.optimize import minimize

from . import _native as N
from ._runs import device_ms, pack_problems
from .device import DeviceData, _ptr
from .posterior import HMC_MAX_DIM, check_hmc_problem, gaussian_weighted_post, logistic_newton_pass, small_lapack_scope, weighted_post, _weights_on_device


class _PosteriorSampler:
    def __init__(self, rng=None):
        self._rng = rng                # None: the global np.random stream, like the reference's closures
        self._ahead = None

    def _randn(self, n, d):
        return np.random.randn(n, d) if self._rng is None else self._rng.randn(n, d)

    def scope(self):
        """Context for a run of calls (the optimisation loop of BetaCoreset / SparseVI opens it once): the single-thread
        BLAS limit the D x D solves want is entered once instead of per call."""
        return small_lapack_scope(self._dim())

    def prefetch(self):
        """Draw the next call's normals now (no-op if they are already waiting).  Only legal when the very next draw
        from this sampler's stream is this sampler's next call with the shape of its previous one: the block is taken
        from the stream HERE, so anything else drawn in between would see the stream one block further than the
        reference's (GreedyVICoreset never prefetches after the last gradient of a loop for that reason)."""
        if self._ahead is None and self._shape is not None:
            self._ahead = self._randn(*self._shape)

    def _normals(self, n, d):
        e, self._ahead = self._ahead, None
        self._shape = (n, d)
        if e is None:
            return self._randn(n, d)
        if e.shape != (n, d):
            # the block was already drawn from the stream: dropping it silently would leave the stream one S x D block
            # ahead of the reference's from here on
            raise RuntimeError('sampler called for %r normals while a prefetched block of shape %r is pending; '
                               'prefetch() may only precede a call of the same shape' % ((n, d), e.shape))
        return e


class LinregPosteriorSampler(_PosteriorSampler):
    """theta ~ N(mu_w, Sigma_w) of Bayesian linear regression on the weighted coreset (model_linreg.py:25-34; the
    `sampler_w` of zellner_neural_linear/main.py:119-124).  Rows pts = [x (D), y]."""

    def __init__(self, th0, Sig0inv, sigsq, rng=None, ctx=None):
        super().__init__(rng)
        self.th0, self.Sig0inv, self.sigsq = np.asarray(th0, dtype=np.float64), np.asarray(Sig0inv, dtype=np.float64), float(sigsq)
        self.ctx = ctx
        self._shape = None

    def _dim(self):
        return self.th0.shape[0]

    def __call__(self, n, wts, pts):
        d = self.th0.shape[0]
        if pts.shape[0] == 0:
            wts, pts = np.zeros(1), np.zeros((1, d + 1))
        muw, LSigw, _ = weighted_post(self.th0, self.Sig0inv, self.sigsq, pts, wts, ctx=self.ctx)
        return muw + self._normals(n, d).dot(LSigw.T)

    def device_spec(self):
        """(sampler kind, parameters) as bc_vi_optimize takes them (include/beta_cores_viopt.h): th0 | Sig0inv | sigsq.  A
        sampler with this method can be evaluated by k_vi_sampler; its normals still come from `_normals`, on the host."""
        return 0, np.concatenate((self.th0, self.Sig0inv.ravel(), [self.sigsq]))


class GaussianPosteriorSampler(_PosteriorSampler):
    """The Gaussian location model's `sampler_w` (zellner_gaussian/main.py:90-95, gaussian.py:28-32)."""

    def __init__(self, mu0, Sig0inv, Siginv, rng=None, ctx=None):
        super().__init__(rng)
        self.mu0, self.Sig0inv, self.Siginv = np.asarray(mu0, dtype=np.float64), np.asarray(Sig0inv, dtype=np.float64), np.asarray(Siginv, dtype=np.float64)
        self.ctx = ctx
        self._shape = None

    def _dim(self):
        return self.mu0.shape[0]

    def __call__(self, n, wts, pts):
        d = self.mu0.shape[0]
        if pts.shape[0] == 0:
            wts, pts = np.zeros(1), np.zeros((1, d))
        muw, LSigw, _ = gaussian_weighted_post(self.mu0, self.Sig0inv, self.Siginv, pts, wts, ctx=self.ctx)
        return muw + self._normals(n, d).dot(LSigw.T)

    def device_spec(self):
        """(sampler kind, parameters) as bc_vi_optimize takes them: mu0 | Sig0inv | Siginv (see LinregPosteriorSampler)."""
        return 1, np.concatenate((self.mu0, self.Sig0inv.ravel(), self.Siginv.ravel()))


# ---- logistic regression: Laplace approximation around the mode of the weighted log-joint (<= M coreset rows: host work
# in the reference too; the formulas keep model_lr.py's expression order so that, on one host, the
# optimiser walks the same path as the reference's)
def _lr_m(z, th):
    z = np.atleast_2d(z)
    th = np.atleast_2d(th)
    m = -z.dot(th.T)
    return z, th, m, m < 100


def _lr_log_joint(z, th, wts):
    """model_lr.py:72-79, 88-93"""
    z, th, m, small = _lr_m(z, th)
    m[small] = -np.log1p(np.exp(m[small]))
    m[np.logical_not(small)] = -m[np.logical_not(small)]
    return (wts[:, np.newaxis] * m).sum(axis=0) + (-0.5 * th.shape[1] * np.log(2. * np.pi) - 0.5 * (th ** 2).sum(axis=1))


def _lr_grad_log_joint(z, th, wts):
    """model_lr.py:98-105, 116-121"""
    z, th, m, small = _lr_m(z, th)
    m[small] = np.exp(m[small]) / (1. + np.exp(m[small]))
    m[np.logical_not(small)] = 1.
    return -th + (wts[:, np.newaxis, np.newaxis] * (m[:, :, np.newaxis] * z[:, np.newaxis, :])).sum(axis=0)


def _lr_hess_log_joint(z, th, wts, diag):
    """model_lr.py:123-137 (full) / 139-153 (diagonal)"""
    z, th, m, small = _lr_m(z, th)
    m[small] = np.exp(m[small]) / (1. + np.exp(m[small])) ** 2
    m[np.logical_not(small)] = 0.
    if diag:
        hl = -m[:, :, np.newaxis] * z[:, np.newaxis, :] ** 2
        return np.tile(-np.ones(th.shape[1]), (th.shape[0], 1)) + (wts[:, np.newaxis, np.newaxis] * hl).sum(axis=0)
    hl = -m[:, :, np.newaxis, np.newaxis] * z[:, np.newaxis, :, np.newaxis] * z[:, np.newaxis, np.newaxis, :]
    return np.tile(-np.eye(th.shape[1]), (th.shape[0], 1, 1)) + (wts[:, np.newaxis, np.newaxis, np.newaxis] * hl).sum(axis=0)


def _lr_mode_newton(Zw, ww, mu0, max_iter=200):
    """The mode of the weighted log-joint by damped Newton steps.  The log-joint is strictly concave (the N(0, I) prior puts
    its Hessian below -I), so the maximiser is unique: it is the point scipy's BFGS converges to, reached here in ~10
    iterations of D x D linear algebra instead of hundreds of rank-two updates (410 -> ~1 ms per sampler call at M = 100,
    D = 128 with weights N/M: the BFGS iteration count grows with the posterior's condition number)."""
    d = mu0.shape[0]
    mu = np.array(mu0, dtype=np.float64)

    def value(th):
        m = -Zw.dot(th)
        return -(ww * (np.maximum(m, 0.) + np.log1p(np.exp(-np.fabs(m))))).sum() - 0.5 * d * np.log(2. * np.pi) - 0.5 * th.dot(th)
    f = value(mu)
    eye = np.eye(d)
    for _ in range(max_iter):
        m = -Zw.dot(mu)
        p = 0.5 * (1. + np.tanh(0.5 * m))                     # e^m / (1 + e^m), overflow-free
        g = -mu + Zw.T.dot(ww * p)
        H = eye + (Zw * (ww * p * (1. - p))[:, np.newaxis]).T.dot(Zw)      # minus the Hessian: positive definite
        step = sl.cho_solve(sl.cho_factor(H, lower=True, check_finite=False), g, check_finite=False)
        t, dec = 1., g.dot(step)
        while True:                                           # backtracking: Newton's full step once near the mode
            cand = mu + t * step
            fc = value(cand)
            if fc >= f + 1e-4 * t * dec or t < 1e-10:
                break
            t *= 0.5
        mu, f = cand, fc
        # stop after a FULL Newton step whose decrement g.H^-1.g (twice the distance of f from its maximum) was already at
        # the rounding floor of f: the point before it was within sqrt(2 dec) <= 2e-6 of the mode, the step squares that.
        # (The gradient cannot be driven below ~ max(w) * eps -- with weights N/M a criterion on |step| alone would spin in
        # rounding noise for the remaining iterations.)
        if (t == 1. and dec <= 64. * np.finfo(np.float64).eps * (1. + abs(f))) or np.fabs(t * step).max() <= 1e-13 * (1. + np.fabs(mu).max()):
            break
    return mu


def _newton_mode(lik, mu0, max_iter=200):
    """_lr_mode_newton's iteration -- same start, backtracking constants and stopping rule, same expressions -- with the
    likelihood parts supplied by a pass `lik(th, hessian) -> (value, grad, H or None)` of sum_n w_n ll_n (value), its gradient and
    minus its Hessian (the device's logistic_newton_pass, or any stand-in).  Each iteration is one pass with the Hessian, each
    backtracking trial one value-only pass."""
    d = mu0.shape[0]
    mu = np.array(mu0, dtype=np.float64)

    def value(th):
        return lik(th, False)[0] - 0.5 * d * np.log(2. * np.pi) - 0.5 * th.dot(th)
    f = value(mu)
    eye = np.eye(d)
    for _ in range(max_iter):
        _, gl, Hl = lik(mu, True)
        g = -mu + gl
        H = eye + Hl
        step = sl.cho_solve(sl.cho_factor(H, lower=True, check_finite=False), g, check_finite=False)
        t, dec = 1., g.dot(step)
        while True:
            cand = mu + t * step
            fc = value(cand)
            if fc >= f + 1e-4 * t * dec or t < 1e-10:
                break
            t *= 0.5
        mu, f = cand, fc
        if (t == 1. and dec <= 64. * np.finfo(np.float64).eps * (1. + abs(f))) or np.fabs(t * step).max() <= 1e-13 * (1. + np.fabs(mu).max()):
            break
    return mu


def _device_laplace(wts, Z, mu0, diag, rng, solver, newton_start, ctx, comm):
    """logistic_laplace over rows resident on the device: every pass over Z is K5 (+ K4 for the Hessian), the D x D algebra
    stays on the host.  With `comm` each rank holds a shard of the rows (and of wts); the passes are summed in rank order, so
    every rank walks the same iterates."""
    n, d = Z.shape
    mu0 = np.asarray(mu0, dtype=np.float64)
    if mu0.shape != (d,):
        raise ValueError('mu0 must have %d entries (one per column of Z), got shape %r' % (d, mu0.shape))
    if wts is not None:
        wts = np.asarray(wts, dtype=np.float64)
        if wts.shape != (n,):
            raise ValueError('wts must have one weight per row of Z (%d), got shape %r' % (n, wts.shape))
    if solver not in ('bfgs', 'newton'):
        raise ValueError("solver must be 'bfgs' (the reference's scipy.optimize.minimize call) or 'newton'")
    if ctx is not None and ctx is not Z.ctx:
        raise ValueError('ctx must be the context the rows Z live on')
    # the reference keeps the rows with wts > 0 (Z[wts > 0]): the others get weight 0, which contributes exactly nothing
    wd = None if wts is None else _weights_on_device(np.where(wts > 0, wts, 0.), n, Z.ctx)

    def lik(th, hessian):
        return logistic_newton_pass(Z, th, wd, hessian=hessian, comm=comm)[:3]
    half_log_2pi = 0.5 * d * np.log(2. * np.pi)
    if solver == 'newton':
        mu = _newton_mode(lik, mu0 if newton_start is None else np.asarray(newton_start, dtype=np.float64))
    trials = 10
    while solver == 'bfgs':
        def neg(th):
            v, g, _ = lik(th, False)
            return -(v - half_log_2pi - 0.5 * th.dot(th)), -(-th + g)
        try:
            res = minimize(neg, mu0, jac=True)
        except (RuntimeError, ValueError):
            raise                       # a failed (or misused) device pass: no restarts on a GPU that may have faulted
        except Exception:
            mu0 = mu0.copy()
            mu0 += np.sqrt((mu0 ** 2).sum()) * 0.1 * (np.random.randn(mu0.shape[0]) if rng is None else rng.randn(mu0.shape[0]))
            trials -= 1
            if trials <= 0:
                raise RuntimeError('logistic_laplace: the mode search failed ten times')
            continue
        mu = res.x
        break
    if diag:
        sq = np.sqrt(1. + logistic_newton_pass(Z, mu, wd, hessian=False, diag=True, comm=comm)[3])
        return mu, np.diag(1. / sq), np.diag(sq)
    LSigInv = np.linalg.cholesky(np.eye(d) + lik(mu, True)[2])
    LSig = sl.solve_triangular(LSigInv, np.eye(d), lower=True, overwrite_b=True, check_finite=False)
    return mu, LSig, LSigInv


def logistic_laplace(wts, Z, mu0, diag=False, rng=None, solver='bfgs', newton_start=None, ctx=None, comm=None):
    """`get_laplace` (examples/zellner_logreg/main.py:86-111 == bayesiancoresets/util/opt.py:9-33): (mu, LSig, LSigInv) of
    the Laplace approximation N(mu, LSig LSig^T) to the posterior of the rows Z with weights wts; the mode comes from
    scipy.optimize.minimize's default method started at mu0 (third-party arithmetic, shared with the reference, not
    restated), a failing optimisation restarts from a perturbed mu0 up to ten times.  diag=True returns the driver's
    diagonal MATRICES (main.py:105-108; util/opt.py:27-29 has vectors, which its own caller cannot multiply with).
    solver='newton' (not the reference's call, same unique mode): see _lr_mode_newton; BFGS stops at a gradient norm of
    1e-5, i.e. ~1e-6 from the mode in theta, which is how far the two answers are apart.

    Z a DeviceData (rows resident on the GPU, e.g. the full data set): the same fit with every pass over the rows on the device
    (_device_laplace; wts: n_rows host weights, zeros allowed, or None = all ones; comm: Z and wts are this rank's shard).  The
    device route has no CPU fallback."""
    if isinstance(Z, DeviceData):
        return _device_laplace(wts, Z, mu0, diag, rng, solver, newton_start, ctx, comm)
    trials = 10
    Zw = Z[wts > 0, :]
    ww = wts[wts > 0]
    if solver == 'newton':
        # (newton_start: where to begin -- the maximiser is unique, so the start only decides how many steps it takes)
        mu = _lr_mode_newton(Zw, ww, mu0 if newton_start is None else newton_start)
    elif solver != 'bfgs':
        raise ValueError("solver must be 'bfgs' (the reference's scipy.optimize.minimize call) or 'newton'")
    while solver == 'bfgs':
        try:
            res = minimize(lambda mu: -_lr_log_joint(Zw, mu, ww)[0], mu0, jac=lambda mu: -_lr_grad_log_joint(Zw, mu, ww)[0, :])
        except Exception:
            mu0 = mu0.copy()
            mu0 += np.sqrt((mu0 ** 2).sum()) * 0.1 * (np.random.randn(mu0.shape[0]) if rng is None else rng.randn(mu0.shape[0]))
            trials -= 1
            if trials <= 0:
                raise RuntimeError('logistic_laplace: the mode search failed ten times')     # (the reference dies on `res` here)
            continue
        mu = res.x
        break
    if diag:
        sq = np.sqrt(-_lr_hess_log_joint(Zw, mu, ww, True)[0, :])
        return mu, np.diag(1. / sq), np.diag(sq)
    if solver == 'newton':
        # (the reference's Hessian expression builds M x D x D temporaries -- 13 MB and ~10 ms at M = 100, D = 128; the same
        # matrix as one BLAS product, equal to rounding)
        m = -Zw.dot(mu)
        p = 0.5 * (1. + np.tanh(0.5 * m))
        LSigInv = np.linalg.cholesky(np.eye(mu.shape[0]) + (Zw * (ww * p * (1. - p))[:, np.newaxis]).T.dot(Zw))
    else:
        LSigInv = np.linalg.cholesky(-_lr_hess_log_joint(Zw, mu, ww, False)[0, :, :])
    LSig = sl.solve_triangular(LSigInv, np.eye(LSigInv.shape[0]), lower=True, overwrite_b=True, check_finite=False)
    return mu, LSig, LSigInv


class LogisticLaplaceSampler(_PosteriorSampler):
    """The logistic drivers' `sampler_w` (examples/zellner_logreg/main.py:139-144): theta = mu_w + randn(S, D).LSig_w^T with
    (mu_w, LSig_w) the Laplace fit of the weighted coreset rows pts = y*x (model_lr.py:29); an empty coreset gives the
    prior N(0, I).  `mu0` is the optimiser's starting point (the drivers pass the prior mean), `diag` their `graddiag`."""

    def __init__(self, mu0, diag=False, rng=None, solver='bfgs'):
        super().__init__(rng)
        self.mu0, self.diag, self.solver = np.asarray(mu0, dtype=np.float64), bool(diag), solver
        self._shape = None
        self._mode = None             # solver='newton': the previous call's mode, the next call's starting point (consecutive
                                      # gradients move the weights a little: 2-3 Newton steps instead of 10-20 from mu0)

    def _dim(self):
        return self.mu0.shape[0]

    def prefetch(self):
        """No look-ahead with the reference's mode search: a failing `minimize` draws its restart perturbation `randn(D)`
        BEFORE the sample normals (main.py:96-101, then :144), so a block drawn ahead would come from the wrong place in the
        stream on such a call.  The Newton search draws nothing, and prefetching stays on for it."""
        if self.solver != 'bfgs':
            super().prefetch()

    def device_spec(self):
        """(sampler kind, parameters) as bc_vi_optimize takes them: start [D] | diag flag, with the start point this sampler's
        next call would begin at.  Only for solver='newton' (k_vi_laplace restates that search); None with the reference's
        optimiser, which stops elsewhere and may draw restart perturbations from the stream: the host loop keeps it."""
        if self.solver != 'newton':
            return None
        return 2, np.concatenate((self.mu0 if self._mode is None else self._mode, [1. if self.diag else 0.]))

    def __call__(self, n, wts, pts):
        d = self.mu0.shape[0]
        if pts.shape[0] == 0:
            wts, pts = np.zeros(1), np.zeros((1, d))
        # (D x D and M x D linear algebra, thousands of tiny BLAS calls inside the mode search: one thread -- a 128-thread
        # pool spends milliseconds synchronising on each; re-entrant, the optimisation loop usually holds the scope already)
        with small_lapack_scope(d):
            muw, LSigw, _ = logistic_laplace(np.asarray(wts, dtype=np.float64), np.atleast_2d(pts), self.mu0, self.diag, rng=self._rng,
                                             solver=self.solver, newton_start=self._mode if self.solver == 'newton' else None)
            if self.solver == 'newton' and np.all(np.isfinite(muw)):
                self._mode = muw.copy()
            return muw + self._normals(n, d).dot(LSigw.T)


class LaplaceFullDataSampler(_PosteriorSampler):
    """theta ~ the Laplace approximation of the logistic posterior of ALL the resident rows (the `sampler_optimal` /
    `sampler_realistic` pattern of zellner_gaussian/main.py:71,83, for logistic data): fitted once, on the device, at
    construction (logistic_laplace with Z = dz, a DeviceData of rows z = y*x); every call returns mu + randn(n, D).LSig^T and
    ignores (wts, pts).  wts: per-row weights of dz (e.g. N/m on a sub-sample, zeros elsewhere), None = all ones."""

    def __init__(self, dz, mu0, wts=None, diag=False, solver='newton', rng=None, comm=None):
        super().__init__(rng)
        self._shape = None
        self.mu, self.LSig, self.LSigInv = logistic_laplace(wts, dz, np.asarray(mu0, dtype=np.float64), diag=diag, rng=rng,
                                                            solver=solver, comm=comm)

    def _dim(self):
        return self.mu.shape[0]

    def __call__(self, n, wts=None, pts=None):
        return self.mu + self._normals(n, self.mu.shape[0]).dot(self.LSig.T)


# ---- exact-posterior samples of the logistic model: multi-chain HMC with every pass over the rows on the device
class HMCResult:
    """What logistic_hmc returns.  samples: n_samples x n_chains x D (the position of every chain after every kept iteration);
    logjoint: n_samples x n_chains; accept: n_samples x n_chains (bool); accept_rate: per chain, over the kept iterations;
    step_size: the step the kept iterations ran with (frozen after warm-up); warmup_steps: the step of every warm-up chunk;
    start, inv_mass: what the run began with; device_ms: GPU milliseconds of the run's chunks (None from a stand-in engine).
    From logistic_hmc_many(score=held) also: correct (n_samples x n_chains: held-out rows predicted correctly by every kept
    position), test_ll (n_samples x n_chains: its summed held-out log-likelihood) and accuracy (held.accuracy(correct)); None
    otherwise.  samples is None from a run with keep_samples=False.  From a run with summary=True also: summary, the
    ChainSummary of the kept iterations (chain_summary has the definitions); None otherwise.  From
    logistic_hmc_many(adapt='stan'): step_size is (n_chains,), inv_mass (n_chains, D), warmup_steps (warmup, n_chains) and
    warmup_accept_stat (warmup, n_chains) holds the acceptance statistic of every warm-up iteration; None otherwise."""

    correct = test_ll = accuracy = summary = warmup_accept_stat = None

    def __init__(self, samples, logjoint, accept, step_size, warmup_steps, start, inv_mass, device_ms):
        self.samples, self.logjoint, self.accept = samples, logjoint, accept
        self.accept_rate = accept.mean(axis=0) if accept.shape[0] else np.zeros(accept.shape[1])
        self.step_size, self.warmup_steps, self.start, self.inv_mass, self.device_ms = step_size, warmup_steps, start, inv_mass, device_ms

    def pooled(self):
        """All chains' samples as one (n_samples * n_chains) x D array, the `thetas` the drivers score."""
        return self.samples.reshape(-1, self.samples.shape[2])


class _DeviceHMC:
    """The engine behind logistic_hmc: the chunked entry points of include/beta_cores_hmc.h."""

    def __init__(self, Z, wd):
        self.Z, self.wd = Z, wd

    def begin(self, start, inv_mass, n_leapfrog, n_iter):
        self._cd = start.shape
        N.call('bc_hmc_begin', self.Z.ctx.h, self.Z.h, self.wd.h if self.wd is not None else None, _ptr(start), int(start.shape[0]),
               _ptr(inv_mass), int(n_leapfrog), int(n_iter))

    def auto_chunk(self, c, d):
        return int(N.load().bc_hmc_auto_chunk(int(c), int(d)))

    def chunk(self, normals, log_u, step_size):
        k = normals.shape[0]
        N.call('bc_hmc_chunk_begin', self.Z.ctx.h, _ptr(normals), _ptr(log_u), int(k), float(step_size))
        samples, lj, acc = np.empty((k,) + self._cd), np.empty((k, self._cd[0])), np.empty((k, self._cd[0]), dtype=np.int32)
        N.call('bc_hmc_chunk_end', self.Z.ctx.h, _ptr(samples), _ptr(lj), _ptr(acc))
        return samples, lj, acc

    def end(self):
        N.load().bc_hmc_end(self.Z.ctx.h)      # (status ignored: also called to close a failed run)
        return device_ms('bc_hmc_device_ms', self.Z.ctx)


def hmc_warmup_step(step, accept_fraction, rate=1.0, target=0.8):
    """The warm-up rule of logistic_hmc: step <- step * exp(rate * (accept_fraction - target))."""
    return float(step) * float(np.exp(rate * (accept_fraction - target)))


def logistic_hmc(Z, wts=None, n_samples=1000, n_chains=16, step_size=0.1, n_leapfrog=8, inv_mass=None, start=None, warmup=0, rng=None,
                 ctx=None, comm=None, adapt_every=25, adapt_rate=1.0, chunk=None, engine=None, summary=False, max_lag=None,
                 summarizer=None):
    """Samples of the logistic posterior of the rows Z = y*x with weights wts under the N(0, I) prior -- the reference's weighted
    log-joint (model_lr.py:88-93; the Stan programs of zellner_logreg/main.py:24-62 with the intercept as a column) -- by plain
    HMC: `n_chains` chains in lock-step, a diagonal inverse mass, a fixed step and `n_leapfrog` leapfrog steps.  Not NUTS, no
    dual averaging here: logistic_hmc_many(adapt='stan') adapts step and mass per chain as Stan's warm-up does, for problems
    that fit one block's LDS.  Every pass over the rows serves all chains at once on the device (k_lr_rows_mc); a chunk of iterations is
    enqueued whole and waited for once.  No CPU fallback.

    Z: a DeviceData (the full data, resident), or an ndarray, which is uploaded -- a weighted coreset of a few hundred points goes
      through the same call.  wts: one weight per row (zeros allowed: such a row contributes exactly nothing), None = all ones.
    start: n_chains x D; None = draws mu + randn(n_chains, D).LSig^T from the device Laplace fit
      (logistic_laplace(..., solver='newton') started at 0).
    inv_mass: D positive numbers, None = ones, 'laplace' = 1 / (1 + diag) with diag from logistic_newton_pass(..., diag=True) at
      the Laplace mode (the posterior variances of the diagonal Laplace approximation).
    Warm-up: `warmup` iterations in chunks of `adapt_every`; after every such chunk
      step <- step * exp(adapt_rate * (acc - 0.8)),   acc = the fraction of accepted proposals of that chunk over all chains
    (hmc_warmup_step: deterministic, host arithmetic between chunks).  Warm-up iterations are discarded, and the step is frozen for
    the n_samples kept iterations.
    Draws (NumPy's stream `rng`, or the global one), in this order: the start's normals (start=None only); then per chunk of k
    iterations randn(k, n_chains, D) followed by log(rand(k, n_chains)).  Kept iterations are chunked by `chunk` (None = as many
    as keep the staged draws under 32 MB).
    summary=True: the result carries `.summary` = chain_summary(result.samples, max_lag) (n_samples >= 4): the samples reach the
      host anyway.  summarizer: a stand-in `summarizer(samples, max_lag) -> summary` for chain_summary (CPU tests).  Off by
      default; it changes no draw and no other output.
    Limits: 1 <= n_chains <= 64, D <= 256, one device (comm.world > 1 raises NotImplementedError).
    Returns an HMCResult."""
    if engine is None and not isinstance(Z, DeviceData):
        if isinstance(Z, np.ndarray) and Z.dtype == np.float32 and Z.ndim == 2:
            Z = DeviceData(Z, ctx=ctx, dtype=np.float32)
        else:
            Z = DeviceData(np.atleast_2d(np.asarray(Z, dtype=np.float64)), ctx=ctx)
    check_hmc_problem(Z.shape, n_chains, comm=comm, ctx=ctx, rows_ctx=getattr(Z, 'ctx', None))
    n, d = Z.shape
    c = int(n_chains)
    if n_samples < 1 or warmup < 0 or n_leapfrog < 1 or adapt_every < 1:
        raise ValueError('needs n_samples >= 1, warmup >= 0, n_leapfrog >= 1 and adapt_every >= 1')
    if not (np.isfinite(step_size) and step_size > 0.):
        raise ValueError('step_size must be finite and positive, got %r' % (step_size,))
    if wts is not None:
        wts = np.ascontiguousarray(wts, dtype=np.float64)
        if wts.shape != (n,):
            raise ValueError('wts must have one weight per row of Z (%d), got shape %r' % (n, wts.shape))
    randn = np.random.randn if rng is None else rng.randn
    mode = None
    if start is None or (isinstance(inv_mass, str) and inv_mass == 'laplace'):
        if engine is not None:
            raise ValueError('a stand-in engine has no Laplace fit: pass start and inv_mass')
        mode, LSig, _ = logistic_laplace(wts, Z, np.zeros(d), solver='newton')
    if isinstance(inv_mass, str):
        if inv_mass != 'laplace':
            raise ValueError("inv_mass must be D positive numbers, None or 'laplace'")
        inv_mass = 1. / (1. + logistic_newton_pass(Z, mode, None if wts is None else np.where(wts > 0, wts, 0.), hessian=False, diag=True)[3])
    inv_mass = np.ones(d) if inv_mass is None else np.ascontiguousarray(inv_mass, dtype=np.float64)
    if inv_mass.shape != (d,) or not np.all(np.isfinite(inv_mass)) or not np.all(inv_mass > 0.):
        raise ValueError('inv_mass must be %d finite positive numbers' % d)
    if start is None:
        start = mode + randn(c, d).dot(LSig.T)
    start = np.ascontiguousarray(start, dtype=np.float64)
    if start.shape != (c, d):
        raise ValueError('start must be n_chains x D = %d x %d, got shape %r' % (c, d, start.shape))
    eng = engine(Z, wts) if engine is not None else _DeviceHMC(Z, None if wts is None else _weights_on_device(wts, n, Z.ctx))
    if chunk is None:
        chunk = eng.auto_chunk(c, d)
    if chunk < 1:
        raise ValueError('chunk must be >= 1')
    # the loop is _run_hmc_group's, for a batch of one on shared draws; a start that is not finite raises from the engine's chunk
    res, _, ms = _run_hmc_group(_SingleAsBatch(eng, swallow=False), [0], start[None], inv_mass[None], [float(step_size)],
                                _ManyDraws(rng, True, 1, c, d, keep=False), c, d, int(n_samples), n_leapfrog, warmup, adapt_every,
                                adapt_rate, chunk)
    out_s, out_l, out_a, step, warm_steps = res[0]
    result = HMCResult(out_s, out_l, out_a, step, warm_steps, start, inv_mass, ms)
    if summary:
        result.summary = summarizer(out_s, max_lag) if summarizer is not None else chain_summary(out_s, max_lag, ctx=getattr(Z, 'ctx', None))
    return result


# ---- held-out scores of many thetas at once (include/beta_cores_score.h)
class HeldOut:
    """Held-out data of the logistic drivers, resident on the device for logistic_score and logistic_hmc_many(score=...):
    Xt (Nt x D, the intercept as a column where the model has one) and the labels Yt in {-1, +1}.  Kept: Z = Yt[:, None] * Xt
    (float64; dtype=np.float32 takes a float32 Xt and keeps the product, which is exact, as float32) and Yt (Nt x 1)."""

    def __init__(self, Xt, Yt, ctx=None, dtype=None):
        Xt = np.asarray(Xt)
        Yt = np.asarray(Yt, dtype=np.float64).ravel()
        if Xt.ndim != 2 or Xt.shape[0] < 1 or Xt.shape[1] < 1:
            raise ValueError('Xt must be Nt x D with Nt >= 1 and D >= 1, got shape %r' % (Xt.shape,))
        if Yt.shape[0] != Xt.shape[0]:
            raise ValueError('Yt must have one label per row of Xt (%d), got %d' % (Xt.shape[0], Yt.shape[0]))
        if not np.all((Yt == 1.) | (Yt == -1.)):
            raise ValueError('Yt must hold labels -1 and +1 only')
        if dtype is not None and np.dtype(dtype) == np.float32:
            if Xt.dtype != np.float32:
                raise ValueError('dtype=float32 takes a float32 Xt (got %s): the library never rounds the caller\'s data' % Xt.dtype)
            Z = np.ascontiguousarray(Yt.astype(np.float32)[:, None] * Xt)
        else:
            Z = Yt[:, None] * np.asarray(Xt, dtype=np.float64)
        if not 1 <= Z.shape[1] <= HMC_MAX_DIM:
            raise ValueError('the rows must have 1 .. %d columns, got %d' % (HMC_MAX_DIM, Z.shape[1]))
        self.Z = DeviceData(Z, ctx=ctx, dtype=dtype)
        self.ctx = self.Z.ctx
        self.Y = DeviceData(np.ascontiguousarray(Yt[:, None]), ctx=self.ctx)
        self.shape = self.Z.shape

    def accuracy(self, correct):
        """correct.sum() / (T * Nt): the reference's compute_accuracy over the thetas `correct` was counted for."""
        correct = np.asarray(correct)
        return float(correct.sum()) / (correct.size * self.shape[0])


def logistic_score(held, thetas):
    """(correct [T] int64, ll [T]) of T parameter vectors against the held-out data `held`: correct[t] counts the rows theta_t
    predicts as the reference does (model_lr.py:32-42: -1 iff log_likelihood(-x, theta) > log_likelihood(x, theta), +1 on a tie;
    in terms of s = y x . theta: correct iff (y = +1 and s >= 0) or (y = -1 and s > 0)), ll[t] = sum_n log_likelihood(z_n, theta_t).
    One kernel (k_lr_score, the contraction on the fp64 matrix cores); the bits of a theta's scores do not depend on the others in
    the batch.  thetas: T x D, finite.  No CPU fallback."""
    th = np.ascontiguousarray(np.atleast_2d(np.asarray(thetas, dtype=np.float64)))
    if th.ndim != 2 or th.shape[0] < 1 or th.shape[1] != held.shape[1]:
        raise ValueError('thetas must be T x %d with T >= 1, got shape %r' % (held.shape[1], th.shape))
    cor, ll = np.empty(th.shape[0], dtype=np.int32), np.empty(th.shape[0])
    N.call('bc_lr_score', held.ctx.h, held.Z.h, held.Y.h, _ptr(th), int(th.shape[0]), _ptr(cor), _ptr(ll))
    return cor.astype(np.int64), ll


# ---- held-out Gaussian predictive scores of the linear-regression family (include/beta_cores_predict.h)
PREDICT_MAX_DIM = 512


class RegressionHeldOut:
    """Held-out rows `[x, y]` of the linear-regression drivers, resident on the device for linreg_predictive.

    Zt: an ndarray, a CUDA torch tensor (borrowed, see DeviceData.from_torch) or a DeviceData, Nt x (D + 1).  Kept once; `dtype`
    as in DeviceData (float32 keeps a float32 array as it is).  With an `encoder` (encoders.MLPEncoder) Zt holds RAW rows
    `[raw x, y]`: they stay resident beside a cache of the encoded rows, which is refilled by DeviceData.encode(..., out=cache)
    whenever `encoder.version` has moved, in `encoded_dtype` -- float32 by default, the storage DeviceProjector(encoder=...) uses
    for its encoded rows, so the scorer sees the features K1 saw.  `.shape` is (Nt, D + 1) of what the kernel reads."""

    def __init__(self, Zt, encoder=None, ctx=None, dtype=None, encoded_dtype=np.float32):
        if isinstance(Zt, DeviceData):
            raw = Zt
        elif hasattr(Zt, 'is_cuda') and hasattr(Zt, 'data_ptr'):
            raw = DeviceData.from_torch(Zt, ctx=ctx)
        else:
            Zt = np.asarray(Zt)
            if Zt.ndim != 2 or Zt.shape[0] < 1 or Zt.shape[1] < 2:
                raise ValueError('Zt must be Nt x (D + 1) rows [x, y] with Nt >= 1 and D >= 1, got shape %r' % (Zt.shape,))
            if encoder is None and Zt.shape[1] - 1 > PREDICT_MAX_DIM:
                raise ValueError('the rows must have 1 .. %d features, got %d' % (PREDICT_MAX_DIM, Zt.shape[1] - 1))
            raw = DeviceData(Zt, ctx=ctx, dtype=dtype)
        if ctx is not None and raw.ctx is not ctx:
            raise ValueError('the held-out rows live on another context')
        self.ctx = raw.ctx
        self.raw = raw
        self.encoder = encoder
        self.encoded_dtype = np.dtype(encoded_dtype)
        self._cache, self._cache_version = None, None
        if encoder is not None:
            if encoder.ctx is not self.ctx:
                raise ValueError('the encoder lives on another context than the held-out rows')
            if raw.shape[1] != encoder.widths[0] + 1:
                raise ValueError('the held-out rows have %d columns, the encoder takes %d + 1 (y)' % (raw.shape[1], encoder.widths[0]))
            width = encoder.widths[-1]
        else:
            width = raw.shape[1] - 1
        if raw.shape[0] < 1 or not 1 <= width <= PREDICT_MAX_DIM:
            raise ValueError('the scored rows must be Nt >= 1 rows of 1 .. %d features and y, got %d x (%d + 1)' % (PREDICT_MAX_DIM, raw.shape[0], width))
        self.shape = (raw.shape[0], width + 1)

    def rows(self):
        """The DeviceData the kernel reads: the resident rows, or with an encoder their encoded copy (re-encoded when
        `encoder.version` has moved since the cache was filled)."""
        if self.encoder is None:
            return self.raw
        if self._cache_version != self.encoder.version:
            self._cache = self.raw.encode(self.encoder, pass_cols=1, dtype=self.encoded_dtype, out=self._cache)
            self._cache_version = self.encoder.version
        return self._cache


class PredictiveScores:
    """What linreg_predictive returns: `.ll` and `.sse` ([T]: the summed Gaussian predictive log density and the summed squared
    error of each posterior over the Nt held-out rows), `.n` = Nt, and `.mean` / `.var` (T x Nt, or None without per_row)."""

    def __init__(self, ll, sse, n, mean=None, var=None):
        self.ll, self.sse, self.n, self.mean, self.var = ll, sse, int(n), mean, var

    def nll(self):
        """-ll / Nt: the neural-linear driver's average loss (the mean negative log density)."""
        return -self.ll / self.n

    def rmse(self, output_std=1.0):
        """output_std * sqrt(sse / Nt): the reference's RMSE after un-normalising (the output mean cancels in the residual)."""
        return output_std * np.sqrt(self.sse / self.n)


def linreg_predictive(held, mu, factor, noise, scale=1.0, per_row=False):
    """Held-out scores of T Gaussian posteriors N(mu_t, F_t F_t^T) of a linear head against a RegressionHeldOut:

        m = phi . mu,   var = noise + scale * ||F^T phi||^2,   ll = sum_n log N(y_n; m_n, var_n),   sse = sum_n (y_n - m_n)^2

    mu: D or T x D.  factor: D x D or T x D x D, ANY factor of the covariance (weighted_post's LSigp gives the covariance the
    reference's samplers draw from, the TRANSPOSE of weighted_post_corrected's LSigp the true posterior, whose covariance is
    LSigp^T LSigp); it enters as a factor so that the
    variance cannot go negative.  noise (> 0), scale (>= 0): scalars or T-vectors; noise = sigma^2, scale = 1 is the reference's
    BayesianRegressionDense, noise = scale = b / a the variance of its fully Bayesian head.  The density is Gaussian only.
    One kernel (k_linreg_predict, the contraction on the fp64 matrix cores, rows split over blocks) and a fixed-order sum of the
    block partials; a posterior's bits do not depend on its batch or on per_row.  D <= 512, one device.  No CPU fallback."""
    if not isinstance(held, RegressionHeldOut):
        raise TypeError('linreg_predictive wants a RegressionHeldOut, got %s' % type(held).__name__)
    nt, d = held.shape[0], held.shape[1] - 1
    mu = np.asarray(mu, dtype=np.float64)
    factor = np.asarray(factor, dtype=np.float64)
    if mu.ndim == 1:
        mu = mu[None]
    if factor.ndim == 2:
        factor = factor[None]
    if mu.ndim != 2 or mu.shape[0] < 1 or mu.shape[1] != d:
        raise ValueError('mu must be %d or T x %d with T >= 1, got shape %r' % (d, d, mu.shape))
    T = mu.shape[0]
    if factor.shape != (T, d, d):
        raise ValueError('factor must be %d x %d or %d x %d x %d, got shape %r' % (d, d, T, d, d, factor.shape))
    vecs = []
    for name, v in (('noise', noise), ('scale', scale)):
        v = np.asarray(v, dtype=np.float64)
        if v.ndim > 1 or (v.ndim == 1 and v.shape[0] != T):
            raise ValueError('%s must be a scalar or %d values, got shape %r' % (name, T, v.shape))
        vecs.append(np.ascontiguousarray(np.broadcast_to(v, (T,))))
    mu, factor = np.ascontiguousarray(mu), np.ascontiguousarray(factor)
    ll, sse = np.empty(T), np.empty(T)
    mean, var = (np.empty((T, nt)), np.empty((T, nt))) if per_row else (None, None)
    N.call('bc_linreg_predict', held.ctx.h, held.rows().h, _ptr(mu), _ptr(factor), _ptr(vecs[0]), _ptr(vecs[1]), T, _ptr(ll), _ptr(sse),
           _ptr(mean) if per_row else None, _ptr(var) if per_row else None)
    return PredictiveScores(ll, sse, nt, mean, var)


# ---- posterior moments, split-R-hat and ESS of chains on the device (include/beta_cores_diag.h)
DIAG_MIN_KEPT = 4


class ChainSummary:
    """What chain_summary returns, per problem (a leading axis P where the samples had one): mean [D], cov [D x D] (ddof = 1, over
    all kept draws of all chains), rhat [D] (split-R-hat: every chain cut into its first and last n // 2 draws), ess [D] (Geyer's
    initial monotone sequence over the split chains' autocorrelations up to max_lag), ess_truncated [D] (bool: the sum ran into
    max_lag before a pair of autocorrelations turned non-positive: ess is then an over-estimate) and status (0, or
    BC_NUMERICAL_PRECISION for a problem with a draw that is not finite or one the sampler had marked: its entries are NaN).
    rhat and ess are NaN for a coordinate that does not vary; ess is NaN where the first pair is not positive (an antithetic
    chain).  rho [D x (L + 1)] and moments [D x 2: W, varplus] are test seams (None unless asked for)."""

    def __init__(self, mean, cov, rhat, ess, ess_truncated, status, rho=None, moments=None):
        self.mean, self.cov, self.rhat, self.ess, self.ess_truncated, self.status = mean, cov, rhat, ess, ess_truncated, status
        self.rho, self.moments = rho, moments

    def problem(self, j):
        """Problem j's entry of a batched summary."""
        opt = [None if a is None else a[j] for a in (self.rho, self.moments)]
        return ChainSummary(self.mean[j], self.cov[j], self.rhat[j], self.ess[j], self.ess_truncated[j], int(self.status[j]), *opt)

    def worst_rhat(self):
        """The largest R-hat over the coordinates that vary (NaN if none does)."""
        r = np.asarray(self.rhat)
        return float(np.nanmax(r)) if np.any(np.isfinite(r)) else float('nan')

    def least_ess(self):
        """The smallest ESS over the coordinates that have one (NaN if none has)."""
        e = np.asarray(self.ess)
        return float(np.nanmin(e)) if np.any(np.isfinite(e)) else float('nan')


def _summary_lag(n, max_lag):
    """(the max_lag handed to the library, L = the lag it clips to) for n kept iterations; None = every lag, n // 2 - 1"""
    if n < DIAG_MIN_KEPT:
        raise ValueError('a summary needs at least %d kept iterations (two per half), got %d' % (DIAG_MIN_KEPT, n))
    top = n // 2 - 1
    lag = top if max_lag is None else int(max_lag)
    if lag < 1:
        raise ValueError('max_lag must be >= 1, got %r' % (max_lag,))
    return lag, min(lag, top)


class _SummaryArrays:
    """The host arrays of one summary call (NaN where the library leaves a marked problem's slices alone) and their pointers."""

    def __init__(self, P, d, L, seams):
        self.mean, self.cov = np.full((P, d), np.nan), np.full((P, d, d), np.nan)
        self.rhat, self.ess = np.full((P, d), np.nan), np.full((P, d), np.nan)
        self.trunc, self.status = np.zeros((P, d), dtype=np.int32), np.zeros(P, dtype=np.int32)
        self.rho = np.full((P, d, L + 1), np.nan) if seams else None
        self.moments = np.full((P, d, 2), np.nan) if seams else None

    def pointers(self):
        return [_ptr(a) if a is not None else None
                for a in (self.mean, self.cov, self.rhat, self.ess, self.trunc, self.status, self.rho, self.moments)]

    def result(self):
        return ChainSummary(self.mean, self.cov, self.rhat, self.ess, self.trunc != 0, self.status, self.rho, self.moments)


def chain_summary(samples, max_lag=None, ctx=None, seams=False):
    """Posterior mean and covariance, split-R-hat and effective sample size of HMC chains, computed on the device
    (include/beta_cores_diag.h states the definitions; kernels k_diag_keep, k_diag_seq, k_diag_cov: the covariance on the fp64
    matrix cores).  samples: n x C x D (kept iterations x chains x coordinates, as HMCResult.samples) or P x n x C x D for P
    problems at once; n >= 4, C <= 64, D <= 256.  max_lag: the largest autocorrelation lag looked at (None = n // 2 - 1, every
    lag a half chain has; a larger request is clipped).  A problem's bits do not depend on the others in the batch.
    seams=True also returns rho and moments (tests).  No CPU fallback.  Returns a ChainSummary."""
    x = np.asarray(samples, dtype=np.float64)
    if x.ndim not in (3, 4):
        raise ValueError('samples must be n x C x D or P x n x C x D, got shape %r' % (x.shape,))
    one = x.ndim == 3
    x = np.ascontiguousarray(x[None] if one else x)
    P, n, c, d = x.shape
    if P < 1:
        raise ValueError('needs at least one problem')
    lag, L = _summary_lag(n, max_lag)
    if ctx is None:
        from .device import default_context
        ctx = default_context()
    out = _SummaryArrays(P, d, L, seams)
    N.call('bc_chain_summary', ctx.h, _ptr(x), int(P), int(n), int(c), int(d), int(lag), *out.pointers())
    res = out.result()
    return res.problem(0) if one else res


# ---- the same for MANY small problems at once: the weighted coresets of an evaluation curve (include/beta_cores_hmc_small.h)
class HMCManyResult(list):
    """What logistic_hmc_many returns: a list with one HMCResult per problem (None for a marked problem under strict=False).
    Every HMCResult carries `route`: 'small' (sampled by the batched in-LDS kernel) or 'single' (too large for one block's LDS:
    sampled by logistic_hmc's engine on the same draws).  fallback: the indices that took the 'single' route; marked: the
    indices whose start was not finite; device_ms: GPU milliseconds of the batched launches (None from a stand-in engine)."""

    def __init__(self, results, fallback, marked, device_ms):
        super().__init__(results)
        self.fallback, self.marked, self.device_ms = list(fallback), list(marked), device_ms


class _SingleAsBatch:
    """One logistic_hmc engine (begin / auto_chunk / chunk / end) behind the batched protocol of _run_hmc_group, as a batch of one.
    swallow: a NumericalPrecisionError of the engine's chunk becomes the problem's status (logistic_hmc_many's marked problems);
    False lets it through as it is (logistic_hmc)."""

    def __init__(self, eng, swallow=True):
        self.eng, self.swallow = eng, swallow

    def begin(self, starts, inv_mass, n_leapfrog, n_iter):
        self.eng.begin(np.ascontiguousarray(starts[0]), np.ascontiguousarray(inv_mass[0]), n_leapfrog, n_iter)

    def auto_chunk(self, c, d):
        return self.eng.auto_chunk(c, d)

    adapted = False      # set by _run_hmc_group after a per-chain warm-up: the kept chunks run at the engine's frozen state

    def adapt_begin(self, log_steps, target_accept, warmup):
        self.eng.adapt_begin(float(log_steps[0]), target_accept, warmup)

    def adapt_chunk(self, normals, log_u, shared):
        e, u = (normals, log_u) if shared else (normals[0], log_u[0])
        lj, acc, stp, alpha = self.eng.adapt_chunk(np.ascontiguousarray(e), np.ascontiguousarray(u))
        return lj[None], acc[None], np.zeros(1, dtype=np.int32), stp[None], alpha[None]

    def adapt_state(self):
        stp, im = self.eng.adapt_state()
        return stp[None], im[None]

    def chunk(self, normals, log_u, steps, shared):
        e, u = (normals, log_u) if shared else (normals[0], log_u[0])
        try:
            if self.adapted:
                s, lj, acc = self.eng.adapted_chunk(np.ascontiguousarray(e), np.ascontiguousarray(u))
            else:
                s, lj, acc = self.eng.chunk(np.ascontiguousarray(e), np.ascontiguousarray(u), float(steps[0]))
        except N.NumericalPrecisionError:
            if not self.swallow:
                raise
            return None, None, None, np.array([N.BC_NUMERICAL_PRECISION], dtype=np.int32)
        return s[None], lj[None], acc[None], np.zeros(1, dtype=np.int32)

    def end(self):
        return self.eng.end()


class _DeviceHMCMany:
    """The batched engine: the chunked entry points of include/beta_cores_hmc_small.h over packed host problems."""

    def __init__(self, ctx, probs):
        self.ctx = ctx
        self.rows, self.w, self.row_ptr = pack_problems(probs)
        self.P, self.d = len(probs), probs[0][0].shape[1]

    def begin(self, starts, inv_mass, n_leapfrog, n_iter):
        self.c = starts.shape[1]
        N.call('bc_hmc_small_begin', self.ctx.h, _ptr(self.rows), _ptr(self.w), _ptr(self.row_ptr), self.P, self.d,
               _ptr(np.ascontiguousarray(starts)), self.c, _ptr(np.ascontiguousarray(inv_mass)), int(n_leapfrog), int(n_iter))

    def auto_chunk(self, c, d):
        return int(N.load().bc_hmc_auto_chunk(int(c), int(d)))

    adapted = False      # set by _run_hmc_group after a per-chain warm-up: the kept chunks run at the chains' frozen state

    def adapt_begin(self, log_steps, target_accept, warmup):
        """The per-chain warm-up of include/beta_cores_hmc_adapt.h on the open run, with Stan's constants and windows."""
        log_steps = np.ascontiguousarray(log_steps, dtype=np.float64)
        N.call('bc_hmc_adapt_begin', self.ctx.h, _ptr(log_steps), float(target_accept), 0.05, 10., 0.75, int(warmup), 75, 50, 25)

    def adapt_chunk(self, normals, log_u, shared):
        """One warm-up chunk, one launch: (logjoint, accept, status, step, alpha), each P x k x C; no sample is copied."""
        k = normals.shape[0] if shared else normals.shape[1]
        normals, log_u = np.ascontiguousarray(normals), np.ascontiguousarray(log_u)
        N.call('bc_hmc_adapt_chunk_begin', self.ctx.h, _ptr(normals), _ptr(log_u), 0 if shared else k * self.c * self.d, int(k))
        lj, stp, alpha = np.zeros((self.P, k, self.c)), np.zeros((self.P, k, self.c)), np.zeros((self.P, k, self.c))
        acc, status = np.zeros((self.P, k, self.c), dtype=np.int32), np.empty(self.P, dtype=np.int32)
        N.call('bc_hmc_adapt_chunk_end', self.ctx.h, None, _ptr(lj), _ptr(acc), _ptr(status), _ptr(stp), _ptr(alpha))
        return lj, acc, status, stp, alpha

    def adapt_state(self):
        stp, im = np.empty((self.P, self.c)), np.empty((self.P, self.c, self.d))
        N.call('bc_hmc_adapt_state', self.ctx.h, _ptr(stp), _ptr(im))
        return stp, im

    def _begin_chunk(self, normals, log_u, steps, shared):
        k = normals.shape[0] if shared else normals.shape[1]
        normals, log_u = np.ascontiguousarray(normals), np.ascontiguousarray(log_u)
        if self.adapted:
            N.call('bc_hmc_adapted_chunk_begin', self.ctx.h, _ptr(normals), _ptr(log_u), 0 if shared else k * self.c * self.d, int(k))
        else:
            steps = np.ascontiguousarray(steps, dtype=np.float64)
            N.call('bc_hmc_small_chunk_begin', self.ctx.h, _ptr(normals), _ptr(log_u), 0 if shared else k * self.c * self.d, int(k), _ptr(steps))
        lj = np.empty((self.P, k, self.c))
        acc, status = np.zeros((self.P, k, self.c), dtype=np.int32), np.empty(self.P, dtype=np.int32)
        return k, lj, acc, status

    def attach_summary(self, n_keep, max_lag):
        """A chain summary of the run's n_keep kept iterations (include/beta_cores_diag.h): chunks run with fold=True are
        retained on the device, summary_end() reduces them."""
        self._lag = _summary_lag(int(n_keep), max_lag)
        N.call('bc_diag_attach', self.ctx.h, int(n_keep), self._lag[0])

    def summary_end(self, seams=False):
        out = _SummaryArrays(self.P, self.d, self._lag[1], seams)
        N.call('bc_diag_end', self.ctx.h, *out.pointers())
        return out.result()

    def chunk(self, normals, log_u, steps, shared, fold=False):
        k, lj, acc, status = self._begin_chunk(normals, log_u, steps, shared)
        if fold:
            N.call('bc_diag_chunk', self.ctx.h)
        s = np.empty((self.P, k, self.c, self.d))
        N.call('bc_hmc_small_chunk_end', self.ctx.h, _ptr(s), _ptr(lj), _ptr(acc), _ptr(status))
        return s, lj, acc, status

    def chunk_scored(self, normals, log_u, steps, shared, held, keep_samples, fold=False):
        """chunk() with the held-out scores of every position, computed on the device where the chunk's samples lie (k_lr_score):
        (samples or None, logjoint, accept, status, correct, test_ll).  held=None: a warm-up chunk -- nothing is scored and no
        samples are copied (None for samples, correct and test_ll).  fold: the chunk is retained for the attached summary."""
        k, lj, acc, status = self._begin_chunk(normals, log_u, steps, shared)
        if fold:
            N.call('bc_diag_chunk', self.ctx.h)
        s = np.empty((self.P, k, self.c, self.d)) if keep_samples and held is not None else None
        cor = tll = None
        if held is not None:
            N.call('bc_score_chunk', self.ctx.h, held.Z.h, held.Y.h)
            cor, tll = np.zeros((self.P, k, self.c), dtype=np.int32), np.zeros((self.P, k, self.c))
        N.call('bc_score_chunk_end', self.ctx.h, _ptr(s) if s is not None else None, _ptr(lj), _ptr(acc), _ptr(status),
               _ptr(cor) if cor is not None else None, _ptr(tll) if tll is not None else None)
        return s, lj, acc, status, cor, tll

    def end(self):
        N.load().bc_hmc_small_end(self.ctx.h)      # (status ignored: also called to close a failed run)
        return device_ms('bc_hmc_small_device_ms', self.ctx)


class _ManyDraws:
    """The draws of logistic_hmc_many, made once per chunk in the documented order and kept while a later group still needs them.
    shared: randn(k, C, D) then log(rand(k, C)), for all problems.  independent: the same pair for p = 0 .. P - 1 in order."""

    def __init__(self, rng, shared, P, c, d, keep):
        self.randn = np.random.randn if rng is None else rng.randn
        self.rand = np.random.rand if rng is None else rng.rand
        self.shared, self.P, self.c, self.d, self.keep, self.made = shared, P, c, d, keep, []

    def get(self, i, k, idx):
        if i == len(self.made):
            if self.shared:
                pair = (self.randn(k, self.c, self.d), np.log(self.rand(k, self.c)))
            else:
                e, u = np.empty((self.P, k, self.c, self.d)), np.empty((self.P, k, self.c))
                for p in range(self.P):
                    e[p], u[p] = self.randn(k, self.c, self.d), np.log(self.rand(k, self.c))
                pair = (e, u)
            self.made.append(pair)
        e, u = self.made[i]
        assert (e.shape[0] if self.shared else e.shape[1]) == k
        if not self.keep:
            self.made[i] = None
        return (e, u) if self.shared else (e[idx], u[idx])


def _run_hmc_group(eng, idx, starts, ims, steps0, draws, c, d, n_samples, n_leapfrog, warmup, adapt_every, adapt_rate, chunk, held=None,
                   keep_samples=True, summaries=None, max_lag=None, stan=None, adapted=None):
    """The loop of logistic_hmc and logistic_hmc_many -- warm-up chunks with hmc_warmup_step per problem, then the kept chunks at
    frozen steps -- for the problems `idx` of one engine.  Returns ({p: (samples, logjoint, accept, step, warm_steps)}, marked indices, device ms).
    held (with an engine that has chunk_scored): the kept chunks are scored on the device, warm-up chunks are neither scored nor
    copied, keep_samples=False copies no samples at all (samples is None); the result tuples end with (correct, test_ll).
    summaries (a dict, with an engine that has attach_summary): the kept chunks -- and only those -- are retained on the device in
    order, and after the last one summaries[p] is problem p's ChainSummary (max_lag as chain_summary's); such a run too can do
    without the sample copies.  None: exactly the calls of a run without a summary.
    stan (a target acceptance, with an engine that has adapt_begin): the warm-up is the engine's per-chain one, in chunks of `chunk`
    iterations; the kept chunks run at every chain's frozen step and mass.  step is then (C,) and warm_steps (warmup, C), and
    adapted[p] = (inv_mass (C, D), alpha (warmup, C)).  None: exactly the calls of a run without it."""
    G = len(idx)
    step = [float(steps0[p]) for p in idx]
    warm = [[] for _ in idx]
    in_run = held is not None and hasattr(eng, 'chunk_scored')
    on_dev = summaries is not None and hasattr(eng, 'attach_summary')
    fold = dict(fold=True) if on_dev else {}
    keep = keep_samples or not (in_run or on_dev)
    out = [(np.empty((n_samples, c, d)) if keep else None, np.empty((n_samples, c)), np.empty((n_samples, c), dtype=bool)) for _ in idx]
    sc = [(np.empty((n_samples, c), dtype=np.int64), np.empty((n_samples, c))) for _ in idx] if in_run else None
    bad = np.zeros(G, dtype=bool)
    eng.begin(np.ascontiguousarray(starts[idx]), np.ascontiguousarray(ims[idx]), int(n_leapfrog), int(warmup) + int(n_samples))
    try:
        if on_dev:
            eng.attach_summary(int(n_samples), max_lag)
        ci, left = 0, int(warmup)
        if stan is not None:
            eng.adapt_begin(np.log(np.array(step)), float(stan), int(warmup))
            traces = []
            while left > 0 and not bad.all():
                k = min(left, int(chunk))
                e, u = draws.get(ci, k, idx)
                status, stp, alpha = eng.adapt_chunk(e, u, draws.shared)[2:]
                bad |= status != 0
                traces.append((stp, alpha))
                left -= k
                ci += 1
            if not bad.all():
                step_c, im_c = eng.adapt_state()
                for j, p in enumerate(idx):
                    if not bad[j]:
                        step[j], warm[j] = step_c[j].copy(), np.concatenate([t[0][j] for t in traces])
                        adapted[p] = (im_c[j].copy(), np.concatenate([t[1][j] for t in traces]))
            eng.adapted = True
        while left > 0 and not bad.all():
            k = min(left, int(adapt_every))
            e, u = draws.get(ci, k, idx)
            if in_run:
                acc, status = eng.chunk_scored(e, u, np.array(step), draws.shared, None, False)[2:4]
            else:
                _, _, acc, status = eng.chunk(e, u, np.array(step), draws.shared)
            bad |= status != 0
            for j in range(G):
                if not bad[j]:
                    warm[j].append(step[j])
                    step[j] = hmc_warmup_step(step[j], float(np.mean(acc[j] != 0)), adapt_rate)
            left -= k
            ci += 1
        # (after a per-chain warm-up the engine runs at its chains' own frozen steps: none is passed, and a marked problem's entry,
        # which stays the start's number beside the others' arrays, is never packed)
        kept_steps = None if stan is not None else np.array(step)
        i0 = 0
        while i0 < n_samples and not bad.all():
            k = min(n_samples - i0, int(chunk))
            e, u = draws.get(ci, k, idx)
            if in_run:
                s, lj, acc, status, cor, tll = eng.chunk_scored(e, u, kept_steps, draws.shared, held, keep, **fold)
            elif not keep:      # (a summarised run that keeps no samples and scores nothing: no sample copy, nothing scored)
                s, lj, acc, status = eng.chunk_scored(e, u, kept_steps, draws.shared, None, False, **fold)[:4]
            else:
                s, lj, acc, status = eng.chunk(e, u, kept_steps, draws.shared, **fold)
            bad |= status != 0
            for j in range(G):
                if not bad[j]:
                    out[j][1][i0:i0 + k], out[j][2][i0:i0 + k] = lj[j], acc[j] != 0
                    if keep:
                        out[j][0][i0:i0 + k] = s[j]
                    if in_run:
                        sc[j][0][i0:i0 + k], sc[j][1][i0:i0 + k] = cor[j], tll[j]
            i0 += k
            ci += 1
        if on_dev and i0 == n_samples:
            every = eng.summary_end()
            summaries.update((p, every.problem(j)) for j, p in enumerate(idx) if not bad[j] and every.status[j] == 0)
    finally:
        ms = eng.end()
    res = {p: out[j] + (step[j], np.array(warm[j])) + (sc[j] if in_run else ()) for j, p in enumerate(idx) if not bad[j]}
    return res, [p for j, p in enumerate(idx) if bad[j]], ms


def _per_problem(x, P, shape, what):
    """x as a P x shape array: one value / array for all problems, or one per problem."""
    a = np.asarray(x, dtype=np.float64)
    if a.shape == shape:
        return np.ascontiguousarray(np.broadcast_to(a, (P,) + shape))
    if a.shape == (P,) + shape:
        return np.ascontiguousarray(a)
    raise ValueError('%s must have shape %r (for all problems) or %r (one per problem), got %r' % (what, shape, (P,) + shape, a.shape))


def _small_problems(problems):
    """The problems of logistic_hmc_many / logistic_laplace_many as a list of (Z_p float64 n_p x D contiguous, w_p [n_p]) and D:
    None weights are ones, an empty coreset is one zero row with weight 0, float32 rows are widened."""
    probs, d = [], None
    for p, pair in enumerate(problems):
        Z, w = pair
        Z = np.asarray(Z)
        if Z.ndim != 2:
            raise ValueError('problem %d: the rows must be n x D, got shape %r' % (p, Z.shape))
        if d is None:
            d = Z.shape[1]
        if Z.shape[1] != d:
            raise ValueError('problem %d: %d columns, the problems before it have %d' % (p, Z.shape[1], d))
        Z = np.ascontiguousarray(Z, dtype=np.float64)
        n = Z.shape[0]
        if w is not None:
            w = np.ascontiguousarray(w, dtype=np.float64)
            if w.shape != (n,):
                raise ValueError('problem %d: wts must have one weight per row of Z (%d), got shape %r' % (p, n, w.shape))
        if n == 0:
            Z, w = np.zeros((1, d)), np.zeros(1)
        probs.append((Z, np.ones(Z.shape[0]) if w is None else w))
    if not probs:
        raise ValueError('needs at least one problem')
    return probs, d


# ---- the Laplace fit of many small problems at once (include/beta_cores_laplace_small.h)
LAPLACE_SMALL_MAX_DIM = 128
LAPLACE_SMALL_MAX_DRAWS = 256


class LaplaceFit:
    """One problem's entry of logistic_laplace_many: mu, LSig (= C^-1) and LSigInv (= C = chol H(mu)) as logistic_laplace returns
    them, hdiag = diag H(mu), value = the log-joint at mu, newton = the Newton steps taken, halvings = the halvings of the last
    line search (halvings_all: of all of them), draws (S x D, or None); with score: correct, test_ll [S] and accuracy."""

    def __init__(self, mu, LSig, LSigInv, hdiag, value, counts, draws):
        self.mu, self.LSig, self.LSigInv, self.hdiag, self.value, self.draws = mu, LSig, LSigInv, hdiag, float(value), draws
        self.newton, self.halvings, self.halvings_all = int(counts[0]), int(counts[1]), int(counts[2])
        self.correct = self.test_ll = self.accuracy = None


class LaplaceManyResult(list):
    """What logistic_laplace_many returns: a list with one LaplaceFit per problem (None for a marked problem under strict=False).
    marked: the indices the device refused; device_ms: GPU milliseconds of the call's launches."""

    def __init__(self, fits, marked, device_ms):
        super().__init__(fits)
        self.marked, self.device_ms = list(marked), device_ms


def logistic_laplace_many(problems, mu0=None, diag=False, n_draws=0, rng=None, draws='shared', score=None, keep_draws=True, strict=True,
                          ctx=None):
    """logistic_laplace(solver='newton') for MANY small problems in one native call: the Laplace posteriors of the weighted
    coresets of an evaluation curve.  One thread block per problem finds the mode by damped Newton steps, factorises H(mu),
    inverts the factor and draws (k_laplace_many: the device function of the weight optimisation loop's logistic sampler);
    nothing crosses the host link before the end.  No CPU fallback.

    problems: as logistic_hmc_many takes them -- a sequence of (Z_p, wts_p): rows z = y*x (n_p x D, D common; float32 rows are
      widened) and one weight per row, or None = all ones.  An empty coreset (0 x D) is one zero row with weight 0: the prior.
    mu0: D numbers or P x D: where the Newton iteration starts (not a prior mean: the prior is N(0, I)); None = zeros.
    diag: the drivers' diagonal form: LSig / LSigInv are np.diag(1 / sqrt(hdiag)) / np.diag(sqrt(hdiag)), as logistic_laplace
      returns them, and the draws are mu + E / sqrt(hdiag).
    n_draws = S: entry p's `draws` are what LogisticLaplaceSampler would draw, mu_p + E.dot(LSig_p.T), computed on the device.
      draws='shared': E = randn(S, D), drawn ONCE from rng (None: the global NumPy stream) and read by every problem;
      draws='independent': randn(S, D) per problem, for p = 0 .. P - 1 in order.  S = 0 draws nothing from the stream.
    score: a HeldOut.  Every entry then carries `correct` and `test_ll` (S each: the bits of logistic_score(score, draws)),
      computed on the device where the draws lie, and `accuracy` = score.accuracy(correct).  Needs n_draws >= 1.
    keep_draws=False (with score): `draws` is None and no draw is copied.
    A problem with a weight, start, value, decrement or pivot that is not finite is marked on the device and costs the others
      nothing: strict=True raises NumericalPrecisionError naming the indices after everything has been copied, strict=False
      leaves None there.
    Limits: D <= 128, S <= 256, one device, Newton only (the reference's BFGS search stays in logistic_laplace).  Returns a
    LaplaceManyResult."""
    if not keep_draws and score is None:
        raise ValueError('keep_draws=False needs score: nothing of the draws would be returned')
    if draws not in ('shared', 'independent'):
        raise ValueError("draws must be 'shared' or 'independent'")
    probs, d = _small_problems(problems)
    P, s = len(probs), int(n_draws)
    if not 1 <= d <= LAPLACE_SMALL_MAX_DIM:
        raise ValueError('logistic_laplace_many serves 1 .. %d columns (one block\'s LDS holds the factor and its inverse), got %d; '
                         'logistic_laplace has no such limit' % (LAPLACE_SMALL_MAX_DIM, d))
    if not 0 <= s <= LAPLACE_SMALL_MAX_DRAWS:
        raise ValueError('n_draws must be 0 .. %d, got %d' % (LAPLACE_SMALL_MAX_DRAWS, s))
    if score is not None and s < 1:
        raise ValueError('score needs n_draws >= 1')
    start = None if mu0 is None else _per_problem(mu0, P, (d,), 'mu0')
    from .device import default_context
    ctx = default_context() if ctx is None else ctx
    if score is not None and (score.ctx is not ctx or score.shape[1] != d):
        raise ValueError('score must hold rows of %d columns on the context of the call' % d)
    diag = bool(diag)
    rows, w, row_ptr = pack_problems(probs)
    randn = np.random.randn if rng is None else rng.randn
    E, stride = None, 0
    if s > 0 and draws == 'shared':
        E = randn(s, d)
    elif s > 0:
        E, stride = np.empty((P, s, d)), s * d
        for p in range(P):
            E[p] = randn(s, d)
    mu, hd, val = np.zeros((P, d)), np.zeros((P, d)), np.zeros(P)
    cnt, status = np.zeros((P, 3), dtype=np.int32), np.zeros(P, dtype=np.int32)
    chol = inv = theta = cor = tll = None
    if not diag:
        chol, inv = np.zeros((P, d, d)), np.zeros((P, d, d))
    if s > 0 and keep_draws:
        theta = np.zeros((P, s, d))
    if score is not None:
        cor, tll = np.zeros((P, s), dtype=np.int32), np.zeros((P, s))

    def opt(a):
        return None if a is None else _ptr(a)
    N.call('bc_laplace_small', ctx.h, _ptr(rows), _ptr(w), _ptr(row_ptr), P, d, opt(start), int(diag), opt(E), stride, s,
           None if score is None else score.Z.h, None if score is None else score.Y.h, _ptr(mu), _ptr(hd), _ptr(val), _ptr(cnt),
           _ptr(status), opt(chol), opt(inv), opt(theta), opt(cor), opt(tll))
    ms = device_ms('bc_laplace_small_device_ms', ctx)
    fits, marked = [], []
    for p in range(P):
        if status[p] != 0:
            fits.append(None)
            marked.append(p)
            continue
        if diag:
            sq = np.sqrt(hd[p])
            f = LaplaceFit(mu[p], np.diag(1. / sq), np.diag(sq), hd[p], val[p], cnt[p], None if theta is None else theta[p])
        else:
            f = LaplaceFit(mu[p], inv[p], chol[p], hd[p], val[p], cnt[p], None if theta is None else theta[p])
        if score is not None:
            f.correct, f.test_ll = cor[p].astype(np.int64), tll[p]
            f.accuracy = score.accuracy(f.correct)
        fits.append(f)
    if marked and strict:
        raise N.NumericalPrecisionError('logistic_laplace_many: problem(s) %s could not be fitted (a weight, start, value, decrement or '
                                        'pivot that is not finite)' % ', '.join(str(p) for p in marked))
    return LaplaceManyResult(fits, marked, ms)


def logistic_hmc_many(problems, n_samples=1000, n_chains=16, step_size=0.1, n_leapfrog=8, inv_mass=None, start=None, warmup=0, rng=None,
                      draws='shared', adapt_every=25, adapt_rate=1.0, chunk=None, strict=True, ctx=None, engine=None, score=None,
                      keep_samples=True, scorer=None, laplace='each', summary=False, summarizer=None, max_lag=None, adapt='chunks',
                      target_accept=0.8):
    """logistic_hmc for MANY small problems in one batched run: the posteriors of the weighted coresets of an evaluation curve
    (`for m in range(M + 1): sample the coreset of size m` in the logistic drivers).  One thread block per problem and group of
    up to four chains holds the problem's rows in LDS and runs whole chunks of iterations there (k_hmc_small); a chunk is one
    launch for all problems.  No CPU fallback.

    problems: a sequence of (Z_p, wts_p): rows z = y*x (n_p x D, D common; float32 rows are widened) and one weight per row, or
      None = all ones.  An empty coreset (0 x D) is taken as one zero row with weight 0: the prior, the drivers' convention.
    start, inv_mass, step_size: as logistic_hmc's, one for all problems or one per problem (start: C x D or P x C x D; inv_mass:
      D, P x D, None or 'laplace'; step_size: a number or P numbers).  start=None and 'laplace' use the device Laplace fit of each
      problem, as logistic_hmc does.
    laplace='each' (default): those fits are made one problem at a time by logistic_laplace(solver='newton') on the problem's
      resident rows.  'batched': all of them by ONE logistic_laplace_many call (D <= 128; a problem it cannot fit raises
      NumericalPrecisionError before the run): start = mu_p + e0.dot(LSig_p.T), inv_mass = 1 / hdiag_p.  The two agree to the
      rounding of the mode search, not bit for bit.
    draws='shared' (default): the draws are made ONCE, in logistic_hmc's order and chunking -- the start's normals randn(C, D)
      if start is None; then per chunk randn(k, C, D) followed by log(rand(k, C)); warm-up chunks of adapt_every iterations, kept
      chunks of `chunk` (None = bc_hmc_auto_chunk(C, D)) -- and every problem reads the same ones: entry p equals, to rounding,
      logistic_hmc(Z_p, wts_p, ..., rng=RandomState(seed)) with every problem seeded alike (common random numbers).
    draws='independent': per chunk (and for the start) the pair is drawn for p = 0 .. P - 1 in order; the automatic chunk is
      divided by P so that the staged draws stay under 32 MB.
    Warm-up: hmc_warmup_step per problem, from that problem's own accepted fraction; the steps diverge per problem and are frozen
      for the kept iterations.
    A problem that does not fit one block's LDS (bc_hmc_small_fits says; INTEGRATION.md has the formula) is sampled by
      logistic_hmc's engine on the same draws after the batched run; the returned list names those in `.fallback`, and each result
      has `.route`.
    A problem whose start is not finite (a non-finite weight shows there) is marked on the device and costs the others nothing:
      strict=True raises NumericalPrecisionError naming the indices after the run is closed, strict=False leaves None there.
    score: a HeldOut.  Every HMCResult then carries `correct` and `test_ll` (n_samples x C: the held-out rows predicted correctly
      by every kept position and its summed held-out log-likelihood) and `accuracy` = score.accuracy(correct), the reference's
      compute_accuracy over the pooled samples.  On the 'small' route the kept chunks are scored on the device where their
      samples lie, before anything is copied; warm-up chunks are neither scored nor copied.  A problem on the 'single' route is
      scored by logistic_score on its returned samples after the run.  Both give the bits of
      logistic_score(score, result.pooled()).  None: nothing changes.
    keep_samples=False (with score or summary): `samples` is None and no chunk's samples are copied -- the largest transfer of a
      chunk.
    summary=True: every HMCResult carries `.summary`, the ChainSummary of its kept iterations (posterior mean and covariance,
      split-R-hat, ESS: chain_summary has the definitions; n_samples >= 4; max_lag as chain_summary's).  On the 'small' route
      the kept chunks -- never a warm-up chunk -- are retained on the device as they are produced and reduced there after the
      last one, so it needs no sample on the host; on the 'single' route it is chain_summary of the returned samples.  Both
      give the bits of chain_summary(result.samples, max_lag).  Off by default: no draw, output or bit of a run changes with it.
    adapt='chunks' (default): the warm-up above.  'stan': every CHAIN adapts its own step and its own diagonal inverse mass on the
      device, as Stan's warm-up does (include/beta_cores_hmc_adapt.h): dual averaging of log(step) towards a mean acceptance
      statistic of `target_accept` (gamma 0.05, t0 10, kappa 0.75), the variances of the positions estimated in doubling windows
      (75 / 50 / 25; none with warmup < 20) and regularised as Stan does.  No NUTS, no step-size search, no step jitter.  The
      warm-up runs in chunks of `chunk` iterations, one launch each, with today's draws per chunk; adapt_every and adapt_rate
      are ignored; step_size and inv_mass are where every chain of a problem starts.  The kept iterations run at each chain's
      averaged step and adapted mass.  Every HMCResult then has step_size (C,), inv_mass (C, D), warmup_steps (warmup, C: the
      step of every warm-up iteration) and warmup_accept_stat (warmup, C: its acceptance statistic min(1, exp(H0 - H1))).
      Needs warmup >= 1; a problem that does not fit one block's LDS is refused with a ValueError before anything is launched.
      score, keep_samples, summary and laplace combine with it unchanged.
    engine: a stand-in `engine(Z_p, wts_p)` per problem with logistic_hmc's engine protocol (CPU tests); scorer: a stand-in
      `scorer(held, thetas) -> (correct, ll)` for logistic_score (CPU tests); summarizer: a stand-in
      `summarizer(samples, max_lag) -> summary` for chain_summary (CPU tests).
    Limits: 1 <= n_chains <= 64, D <= 256, one device.  Returns an HMCManyResult."""
    if not keep_samples and score is None and not summary:
        raise ValueError('keep_samples=False needs score: nothing would be returned')
    if summary:
        _summary_lag(int(n_samples), max_lag)
    if scorer is None:
        scorer = logistic_score
    if draws not in ('shared', 'independent'):
        raise ValueError("draws must be 'shared' or 'independent'")
    if laplace not in ('each', 'batched'):
        raise ValueError("laplace must be 'each' or 'batched'")
    if adapt not in ('chunks', 'stan'):
        raise ValueError("adapt must be 'chunks' or 'stan'")
    stan = adapt == 'stan'
    if stan and (warmup < 1 or not 0. < float(target_accept) < 1.):
        raise ValueError("adapt='stan' needs warmup >= 1 and 0 < target_accept < 1")
    probs, d = _small_problems(problems)
    P = len(probs)
    c = int(n_chains)
    check_hmc_problem((1, d), c)
    if n_samples < 1 or warmup < 0 or n_leapfrog < 1 or adapt_every < 1:
        raise ValueError('needs n_samples >= 1, warmup >= 0, n_leapfrog >= 1 and adapt_every >= 1')
    steps0 = _per_problem(step_size, P, (), 'step_size')
    if not (np.all(np.isfinite(steps0)) and np.all(steps0 > 0.)):
        raise ValueError('step_size must be finite and positive, got %r' % (step_size,))
    shared = draws == 'shared'
    randn = np.random.randn if rng is None else rng.randn
    want_laplace = isinstance(inv_mass, str) and inv_mass == 'laplace'
    if isinstance(inv_mass, str) and not want_laplace:
        raise ValueError("inv_mass must be D positive numbers (or P x D), None or 'laplace'")
    if engine is None:
        from .device import default_context
        ctx = default_context() if ctx is None else ctx
        if score is not None and (score.ctx is not ctx or score.shape[1] != d):
            raise ValueError('score must hold rows of %d columns on the context of the run' % d)
    fits = [True] * P if engine is not None else [bool(N.load().bc_hmc_small_fits(ctx.h, int(z.shape[0]), int(d))) for z, _ in probs]
    if stan and not all(fits):
        p = fits.index(False)
        raise ValueError("adapt='stan': problem %d (%d rows x %d) does not fit one block's LDS; the per-chain warm-up serves the "
                         "batched route only" % (p, probs[p][0].shape[0], d))
    resident = {}

    def on_device(p):      # (the rows of p on the device: the Laplace fit and the single-problem route share them)
        if p not in resident:
            resident[p] = DeviceData(probs[p][0], ctx=ctx)
        return resident[p]
    if start is None or want_laplace:
        if engine is not None:
            raise ValueError('a stand-in engine has no Laplace fit: pass start and inv_mass')
        if laplace == 'batched':
            many = logistic_laplace_many(probs, ctx=ctx)
            fit = [(r.mu, r.LSig) for r in many]
            if want_laplace:
                inv_mass = np.array([1. / r.hdiag for r in many])
        else:
            fit = [logistic_laplace(w, on_device(p), np.zeros(d), solver='newton')[:2] for p, (z, w) in enumerate(probs)]
        if want_laplace and laplace != 'batched':
            inv_mass = np.array([1. / (1. + logistic_newton_pass(on_device(p), fit[p][0], np.where(w > 0, w, 0.), hessian=False, diag=True)[3])
                                 for p, (z, w) in enumerate(probs)])
    ims = _per_problem(np.ones(d) if inv_mass is None else inv_mass, P, (d,), 'inv_mass')
    if not np.all(np.isfinite(ims)) or not np.all(ims > 0.):
        raise ValueError('inv_mass must be %d finite positive numbers' % d)
    if start is None:
        e0 = randn(c, d) if shared else None
        starts = np.array([fit[p][0] + (e0 if shared else randn(c, d)).dot(fit[p][1].T) for p in range(P)])
    else:
        starts = _per_problem(start, P, (c, d), 'start')
    # the groups: the problems that fit go through the batched engine together, every other problem through its own engine
    if engine is not None:
        groups = [(_SingleAsBatch(engine(z, w)), [p]) for p, (z, w) in enumerate(probs)]
    else:
        small = [p for p in range(P) if fits[p]]
        groups = [(_DeviceHMCMany(ctx, [probs[p] for p in small]), small)] if small else []
        for p in range(P):
            if not fits[p]:
                groups.append((_SingleAsBatch(_DeviceHMC(on_device(p), _weights_on_device(probs[p][1], probs[p][0].shape[0], ctx))), [p]))
    if chunk is None:
        chunk = groups[0][0].auto_chunk(c, d)
        if not shared:
            chunk = max(1, chunk // P)
    if chunk < 1:
        raise ValueError('chunk must be >= 1')
    stream = _ManyDraws(rng, shared, P, c, d, keep=len(groups) > 1)
    done, marked, ms_small = {}, [], None
    for eng, idx in groups:
        sums = {} if summary else None
        extra = dict(summaries=sums, max_lag=max_lag) if summary else {}
        own = {}
        if stan:
            extra.update(stan=float(target_accept), adapted=own)
        res, bad, ms = _run_hmc_group(eng, idx, starts, ims, steps0, stream, c, d, int(n_samples), n_leapfrog, warmup, adapt_every,
                                      adapt_rate, chunk, held=score, keep_samples=keep_samples, **extra)
        for p, r in res.items():
            s, lj, acc, step, warm = r[:5]
            done[p] = HMCResult(s, lj, acc, step, warm, starts[p], own[p][0] if stan else ims[p], ms)
            if stan:
                done[p].warmup_accept_stat = own[p][1]
            done[p].route = 'small' if fits[p] else 'single'
            if summary:
                if p in sums:
                    done[p].summary = sums[p]
                else:      # (the route that returns its samples anyway)
                    done[p].summary = summarizer(s, max_lag) if summarizer is not None else chain_summary(s, max_lag, ctx=ctx)
                    if not keep_samples and score is None:
                        done[p].samples = None
            if score is not None:
                if len(r) > 5:
                    cor, tll = r[5:]
                else:
                    cor, tll = scorer(score, done[p].pooled())
                    cor, tll = np.asarray(cor, dtype=np.int64).reshape(lj.shape), np.asarray(tll, dtype=np.float64).reshape(lj.shape)
                    if not keep_samples:
                        done[p].samples = None
                done[p].correct, done[p].test_ll, done[p].accuracy = cor, tll, score.accuracy(cor)
        marked += bad
        if isinstance(eng, _DeviceHMCMany):
            ms_small = ms
    marked.sort()
    if marked and strict:
        raise N.NumericalPrecisionError('logistic_hmc_many: the log-joint or its gradient at the start of problem(s) %s is not finite '
                                        '(a weight or a start point that is not finite)' % ', '.join(str(p) for p in marked))
    return HMCManyResult([done.get(p) for p in range(P)], [p for p in range(P) if not fits[p]], marked, ms_small)
