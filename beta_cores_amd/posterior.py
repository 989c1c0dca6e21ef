"""Weighted Gaussian posteriors (the samplers' `weighted_post`), with the row reductions on the GPU.

  weighted_post(th0, Sig0inv, sigsq, z, w)            linear regression,
      examples/common/model_linreg.py:25-34 == model_neurlinr.py:115-122
  gaussian_weighted_post(th0, Sig0inv, Siginv, x, w)  Gaussian location model, gaussian.py:28-32

The O(N D^2) part -- X^T diag(w) X and X^T (w*y) -- is kernel K4 (bc_weighted_gram, fp64 MFMA);
the D x D Cholesky / triangular solve stay in LAPACK on the host, with the reference's exact
expressions.  NOTE: the reference forms  LSigp @ LSigp.T  (= C^-1 C^-T) where the
true posterior covariance is C^-T C^-1; that is reproduced on purpose -- parity target is the
reference's output.  `weighted_post_corrected` is the mathematically right variant.
"""
import ctypes as C

import numpy as np
import scipy.linalg as sl

import contextlib

from . import _native as N
from .device import DeviceData, _ptr, default_context

try:
    from threadpoolctl import ThreadpoolController as _Controller
except Exception:                                     # pragma: no cover
    _Controller = None
_controller = None


_limit_depth = 0


@contextlib.contextmanager
def small_lapack_scope(d):
    """The D x D Cholesky / triangular solve of a coreset posterior is microseconds of work; on a
    many-core host a multi-threaded BLAS spends milliseconds synchronising its pool on it (measured:
    4.9 ms per solve_triangular at D = 64 with 128 threads).  Same routines, one thread.  The controller is
    created once: discovering the loaded BLAS libraries costs ~0.9 ms, more than the solve it guards.
    Re-entrant: entering the limit costs ~10 us, so a caller that runs many posteriors in a row (the greedy-VI
    optimisation loop) opens the scope once and the calls inside find it open."""
    global _controller, _limit_depth
    if _Controller is None or d > 512 or _limit_depth > 0:
        yield
        return
    if _controller is None:
        _controller = _Controller()
    with _controller.limit(limits=1, user_api='blas'):
        _limit_depth += 1
        try:
            yield
        finally:
            _limit_depth -= 1


_small_lapack = small_lapack_scope


def weighted_gram(z, w=None, ctx=None, comm=None):
    """(X^T diag(w) X, X^T (w*y)) for rows z = [x, y]; `z` may be an ndarray or a DeviceData.
    With `comm` the rows are this rank's shard and the two results are summed over ranks."""
    ctx = ctx or default_context()
    if w is not None:
        w = np.ascontiguousarray(w, dtype=np.float64)
    if isinstance(z, np.ndarray) and z.dtype == np.float32 and z.ndim == 2 and z.shape[0] * (z.shape[1] + 1) > 60000:
        z = DeviceData(z, ctx=ctx, dtype=np.float32)      # a large float32 array is uploaded as it is (the same bits, half the bytes)
    if not isinstance(z, DeviceData):
        z = np.ascontiguousarray(np.atleast_2d(z), dtype=np.float64)
        if w is not None and w.shape != (z.shape[0],):
            raise ValueError('w must have one weight per row')
        if z.shape[0] * (z.shape[1] + 1) <= 60000 and z.shape[1] * z.shape[1] <= 60000:
            # coreset-sized call (the samplers, once per gradient): rows, weights and results in one native call
            d = z.shape[1] - 1
            G, v = np.empty((max(d, 0), max(d, 0))), np.empty(max(d, 0))
            N.call('bc_weighted_gram_host', ctx.h, _ptr(z), int(z.shape[0]), int(z.shape[1]), _ptr(w) if w is not None else None,
                   _ptr(G), _ptr(v))
            if comm is not None and comm.world > 1:
                G = comm.sum_in_rank_order(G)
                v = comm.sum_in_rank_order(v)
            return G, v
        data = DeviceData(z, ctx=ctx)
    else:
        data = z
    n, dz = data.shape
    d = dz - 1
    G = np.empty((d, d))
    v = np.empty(d)
    if w is not None and w.shape != (n,):
        raise ValueError('w must have one weight per row')
    N.call('bc_weighted_gram', data.ctx.h, data.h, _ptr(w) if w is not None else None, _ptr(G), _ptr(v))
    if comm is not None and comm.world > 1:
        G = comm.sum_in_rank_order(G)
        v = comm.sum_in_rank_order(v)
    return G, v


def weighted_post(th0, Sig0inv, sigsq, z, w, ctx=None, comm=None):
    G, v = weighted_gram(z, w, ctx=ctx, comm=comm)
    with _small_lapack(G.shape[0]):
        LSigpInv = np.linalg.cholesky(Sig0inv + G / sigsq)
        LSigp = sl.solve_triangular(LSigpInv, np.eye(LSigpInv.shape[0]), lower=True, overwrite_b=True, check_finite=False)
        mup = np.dot(LSigp.dot(LSigp.T), np.dot(Sig0inv, th0) + v / sigsq)
    return mup, LSigp, LSigpInv


def weighted_post_corrected(th0, Sig0inv, sigsq, z, w, ctx=None, comm=None):
    """Same inputs, true posterior mean Sigma_p (Sig0inv th0 + X^T W y / sigsq) with Sigma_p = C^-T C^-1."""
    G, v = weighted_gram(z, w, ctx=ctx, comm=comm)
    LSigpInv = np.linalg.cholesky(Sig0inv + G / sigsq)
    LSigp = sl.solve_triangular(LSigpInv, np.eye(LSigpInv.shape[0]), lower=True, check_finite=False)
    mup = np.dot(LSigp.T.dot(LSigp), np.dot(Sig0inv, th0) + v / sigsq)
    return mup, LSigp, LSigpInv


def gaussian_weighted_post(th0, Sig0inv, Siginv, x, w, ctx=None, comm=None):
    """gaussian.py:28-32.  sum_i w_i x_i is taken from K4 by appending a column of ones as `y`."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    w = np.ascontiguousarray(w, dtype=np.float64)
    _, xw = weighted_gram(np.hstack((x, np.ones((x.shape[0], 1)))), w, ctx=ctx, comm=comm)
    wsum = w.sum()
    if comm is not None and comm.world > 1:
        wsum = comm.sum_in_rank_order(np.array([wsum]))[0]
    with _small_lapack(Siginv.shape[0]):
        LSigpInv = np.linalg.cholesky(Sig0inv + wsum * Siginv)
        LSigp = sl.solve_triangular(LSigpInv, np.eye(LSigpInv.shape[0]), lower=True, overwrite_b=True, check_finite=False)
        mup = np.dot(LSigp.dot(LSigp.T), np.dot(Sig0inv, th0) + np.dot(Siginv, xw))
    return mup, LSigp, LSigpInv


def logistic_newton_pass(dz, theta, w=None, hessian=True, diag=False, comm=None, ctx=None):
    """The logistic log-likelihood sum_n w_n ll_n of resident rows z = y*x (no y column, model_lr.py:29) at `theta`, and its
    derivatives, from one streaming pass over the rows (K5) plus, for the Hessian, one weighted Gram (K4):
    (value, grad, H or None, diag or None) with H = sum_n w_n c_n z_n z_n^T and diag its diagonal -- MINUS the likelihood's
    Hessian, c = p (1 - p).  The N(0, I) prior is not included.  `dz`: a DeviceData (an ndarray is uploaded first); `w`: n_rows
    host weights, a DeviceData of n_rows x 1 (upload once, pass many times), or None = all ones.  With `comm` the rows are this
    rank's shard and the four parts are summed over ranks in rank order (the same bits on every rank)."""
    if not isinstance(dz, DeviceData):
        if isinstance(dz, np.ndarray) and dz.dtype == np.float32 and dz.ndim == 2:
            dz = DeviceData(dz, ctx=ctx, dtype=np.float32)      # float32 rows are uploaded as they are (the same bits, half the bytes)
        else:
            dz = DeviceData(np.atleast_2d(np.asarray(dz, dtype=np.float64)), ctx=ctx)
    n, d = dz.shape
    th = np.ascontiguousarray(theta, dtype=np.float64)
    if th.shape != (d,):
        raise ValueError('theta must have %d entries (one per column of the rows), got shape %r' % (d, th.shape))
    wd = _weights_on_device(w, n, dz.ctx)
    val = C.c_double()
    g = np.empty(d)
    dg = np.empty(d) if diag else None
    H = np.empty((d, d)) if hessian else None
    N.call('bc_logistic_newton_pass', dz.ctx.h, dz.h, wd.h if wd is not None else None, _ptr(th), C.byref(val), _ptr(g),
           _ptr(dg), _ptr(H))
    value = val.value
    if comm is not None and comm.world > 1:
        parts = [np.array([value]), g] + ([dg] if diag else []) + ([H.ravel()] if hessian else [])
        tot = comm.sum_in_rank_order(np.concatenate(parts))
        value, g = float(tot[0]), tot[1:1 + d]
        o = 1 + d
        if diag:
            dg, o = tot[o:o + d], o + d
        if hessian:
            H = tot[o:o + d * d].reshape(d, d)
    return value, g, H, dg


def _weights_on_device(w, n, ctx):
    """n host weights -> a DeviceData of n x 1 (None stays None: all ones)."""
    if w is None or isinstance(w, DeviceData):
        if w is not None and w.shape != (n, 1):
            raise ValueError('w must be a DeviceData of %d x 1, got %r' % (n, w.shape))
        return w
    w = np.ascontiguousarray(w, dtype=np.float64)
    if w.shape != (n,):
        raise ValueError('w must have one weight per row (%d), got shape %r' % (n, w.shape))
    return DeviceData(w.reshape(n, 1), ctx=ctx)


HMC_MAX_CHAINS, HMC_MAX_DIM = 64, 256      # the limits of the multi-chain rows pass (include/beta_cores_hmc.h)


def check_hmc_problem(shape, n_chains, comm=None, ctx=None, rows_ctx=None):
    """The argument checks shared by logistic_logjoint_batch and samplers.logistic_hmc, before anything reaches the device."""
    if comm is not None and comm.world > 1:
        raise NotImplementedError('the multi-chain logistic pass serves one device: row shards (comm.world > 1) are not implemented')
    if ctx is not None and ctx is not rows_ctx:
        raise ValueError('ctx must be the context the rows live on')
    if not 1 <= int(n_chains) <= HMC_MAX_CHAINS:
        raise ValueError('1 .. %d chains are served, got %d' % (HMC_MAX_CHAINS, int(n_chains)))
    if len(shape) != 2 or not 1 <= shape[1] <= HMC_MAX_DIM:
        raise ValueError('the rows must be n x D with 1 <= D <= %d, got shape %r' % (HMC_MAX_DIM, tuple(shape)))


def logistic_logjoint_batch(dz, thetas, w=None, comm=None, ctx=None, value=True):
    """The weighted logistic log-joint with the N(0, I) prior (model_lr.py:88-93) of resident rows z = y*x at C parameter
    vectors at once, and its gradients: (values [C], grads [C, D]) from ONE pass over the rows (k_lr_rows_mc: both contractions
    on the fp64 matrix cores, 16 chains per tile).  `dz`: a DeviceData (an ndarray is uploaded first; float32 rows stay
    float32); `thetas`: C x D with 1 <= C <= 64, D <= 256; `w`: n_rows host weights, a DeviceData of n_rows x 1, or None = all
    ones.  value=False: the gradient-only pass the inner leapfrog steps of the HMC run use, (None, grads).  The bits of one theta's
    results do not depend on the others in the batch."""
    if not isinstance(dz, DeviceData):
        if isinstance(dz, np.ndarray) and dz.dtype == np.float32 and dz.ndim == 2:
            dz = DeviceData(dz, ctx=ctx, dtype=np.float32)
        else:
            dz = DeviceData(np.atleast_2d(np.asarray(dz, dtype=np.float64)), ctx=ctx)
    n, d = dz.shape
    th = np.ascontiguousarray(np.atleast_2d(thetas), dtype=np.float64)
    check_hmc_problem(dz.shape, th.shape[0], comm=comm, ctx=ctx, rows_ctx=dz.ctx)
    if th.ndim != 2 or th.shape[1] != d:
        raise ValueError('thetas must be C x %d (one column per column of the rows), got shape %r' % (d, th.shape))
    wd = _weights_on_device(w, n, dz.ctx)
    vals = np.empty(th.shape[0]) if value else None
    grads = np.empty(th.shape)
    N.call('bc_logistic_logjoint_batch', dz.ctx.h, dz.h, wd.h if wd is not None else None, _ptr(th), int(th.shape[0]), _ptr(vals),
           _ptr(grads))
    return vals, grads
