"""Projectors: data rows -> row-centred (beta-)log-likelihood vectors Phi (N x S).

Two families, one protocol (bayesiancoresets/coreset/projector.py:5-66:
`project(pts, grad=False)`, `project_f(pts, beta, grad=False)`, `update(wts, pts)`):

* BlackBoxProjector / BetaBlackBoxProjector -- the reference's classes: arbitrary host
  callables produce the N x S array, which the device solvers then upload.
* DeviceProjector / DeviceBetaProjector -- K1 on the GPU: the likelihood is one of the
  models in beta_cores_amd.likelihoods, the contraction Z.Theta^T, the formula, the
  row-centring, the row norms and the column sums run in one kernel and Phi never
  leaves HBM (a DevicePhi is returned).
"""
import ctypes as C

import numpy as np

from .. import _native as N
from .._runs import device_ms, run_chunks, step_draws
from ..device import DeviceData, _as_rows, _ptr, default_context, upload_slot
from ..likelihoods import GaussianLocation, LinearRegression, LogisticRegression
from ..util import numpy_bits
from ..util.opt import adam_step_arrays
from .residency import _BIG_ROWS, _PIPE_ROWS, _SMALL_ROWS, Pin, WeakIdMap, _PhiPool, _resident_dtype      # noqa: F401 (names kept importable from here)


class Projector(object):
    def project(self, pts, grad=False):
        raise NotImplementedError

    def update(self, wts, pts):
        raise NotImplementedError


class BlackBoxProjector(Projector):
    """projector.py:12-37"""

    def __init__(self, sampler, projection_dimension, loglikelihood, grad_loglikelihood=None, **kwargs):
        self.projection_dimension = projection_dimension
        self.sampler = sampler
        self.loglikelihood = loglikelihood
        self.grad_loglikelihood = grad_loglikelihood
        self.update(np.array([]), np.array([]))
        self.encoder = kwargs.get('nl', None)      # optional learned feature map

    def project(self, pts, grad=False):
        args = (pts, self.samples) + ((self.encoder,) if self.encoder else ())
        lls = self.loglikelihood(*args)
        lls -= lls.mean(axis=1)[:, np.newaxis]
        if not grad:
            return lls
        if self.grad_loglikelihood is None:
            raise ValueError('grad_loglikelihood was requested but not initialized in BlackBoxProjector.project')
        glls = self.grad_loglikelihood(pts, self.samples)
        glls -= glls.mean(axis=2)[:, :, np.newaxis]
        return lls, glls

    def update(self, wts, pts):
        self.samples = self.sampler(self.projection_dimension, wts, pts)


class BetaBlackBoxProjector(Projector):
    """projector.py:39-66"""

    def __init__(self, sampler, projection_dimension, beta_likelihood, loglikelihood, beta_gradient, **kwargs):
        self.projection_dimension = projection_dimension
        self.sampler = sampler
        self.beta_likelihood = beta_likelihood
        self.loglikelihood = loglikelihood
        self.beta_gradient = beta_gradient
        self.update(np.array([]), np.array([]))
        self.encoder = kwargs.get('nl', None)

    def project_f(self, pts, beta, grad=False):
        args = (pts, self.samples, beta) + ((self.encoder,) if self.encoder else ())
        bls = self.beta_likelihood(*args)
        bls -= bls.mean(axis=1)[:, np.newaxis]
        if not grad:
            return bls
        if self.beta_gradient is None:
            raise ValueError('grad_loglikelihood was requested but not initialized in BlackBoxProjector.project')
        glls = self.beta_gradient(pts, self.samples, beta)
        glls -= glls.mean(axis=1)[:, np.newaxis]
        return bls, glls

    def update(self, wts, pts):
        self.samples = self.sampler(self.projection_dimension, wts, pts)


# limits of the native gradient entry points (bc_vi_gradient, bc_vi_optimize: csrc/bc_vigrad.hip, csrc/bc_viopt.hip)
VI_MAX_SAMPLES = 256           # one pass of the store-free K1
VI_MAX_CORE_DOUBLES = 60000    # m * (dz + 1): the coreset rows and their weights fit the native staging area
PSVI_MAX_ROW_DOUBLES = 3840    # bc_psvi_gradient: widest point row (csrc/bc_psvi_dev.h: BC_PSVI_MAX_DZ, the kernel's LDS work space)
VI_OPT_MAX_DIM = 128          # bc_vi_optimize: the factor and its inverse share one work-group's LDS (BC_VI_MAX_DIM)


class _DeviceProjectorBase(Projector):
    def __init__(self, sampler, projection_dimension, model, ctx=None, encoder=None, pass_cols=1, encoded_dtype=np.float32):
        self.projection_dimension = projection_dimension
        self.sampler = sampler
        self.model = model
        self.ctx = ctx or default_context()
        # optional device feature encoder (encoders.MLPEncoder; the `nl` of the black-box classes): every route that turns
        # `pts` into device rows encodes them first, so callers keep speaking RAW rows [x, pass-through]
        self.encoder = encoder
        self.pass_cols = int(pass_cols)
        self.encoded_dtype = np.dtype(encoded_dtype)
        self._enc_cache = WeakIdMap()   # resident rows -> (encoder version, encoded DeviceData)
        self._enc_out = None       # the one re-used output buffer for transient rows
        self.encode_launches = 0   # bulk encodes this projector has issued (a cache hit issues none)
        self.vi_optimize_calls = 0 # weight optimisations that ran on the device (vi_optimize)
        if encoder is not None and encoder.ctx is not self.ctx:
            raise ValueError('the encoder lives on another context than the projector')
        self._pins = WeakIdMap(strong=True)      # ndarray -> residency.Pin: arrays the caller pinned (see pin())
        self._slots = {}           # dz -> DeviceData slot for small transient inputs
        self._pool = _PhiPool(self.ctx)
        # constant rows whose value holds an np.exp: on a host whose NumPy is not the one the library restates they are
        # evaluated on the host (util/numpy_bits.py); `_key_cache`: the y's of the all-zero-feature rows of large inputs
        self._host_constants = numpy_bits.warn_if_constant_bits_differ(model) and getattr(model, 'host_constants', None) is not None
        self._key_cache = WeakIdMap()
        self.constant_rows_from_host = 0      # how many (y, value) pairs the last beta-projection handed to the kernel
        self.update(np.array([]), np.array([]))

    def update(self, wts, pts):
        self.samples = self.sampler(self.projection_dimension, wts, pts)

    # -- data residency.  Default: like projector.py:24, every project() reads the LIVE host array (it is uploaded
    # for that call).  A large array projected over and over (BetaCoreset's full-data gradient loop) can be pinned:
    # uploaded once, served from HBM afterwards, read-only on the host until unpinned.
    def pin(self, pts):
        """Keep a device copy of `pts` for later project() calls; returns the DeviceData.  `pts` becomes read-only
        (ndarray.flags.writeable = False) until unpin(pts) / forget(), or until the projector dies."""
        if isinstance(pts, DeviceData):
            return pts
        hit = self._pins.get(pts)
        if hit is not None:
            hit.count += 1
            return hit.data
        if isinstance(pts, np.ndarray) and pts.base is not None:
            # a view: edits through its base array would go unseen by the device copy (the read-only flag only guards
            # the view itself), so views are not pinned -- they are uploaded per call like any live array
            raise ValueError('pin(): the array is a view of another array; pin the base array or pass a copy')
        arr = np.atleast_2d(pts)
        dd = DeviceData(arr, ctx=self.ctx, dtype=_resident_dtype(arr))      # a float32 array keeps a float32 device copy
        return self._pins.put(pts, Pin(self, pts, dd)).data

    def pinned(self, pts):
        """The DeviceData of an array the caller has pinned on this projector (pin()), or None."""
        hit = self._pins.get(pts)
        return hit.data if hit is not None else None

    def unpin(self, pts):
        hit = self._pins.get(pts)
        if hit is None:
            return
        hit.count -= 1
        if hit.count <= 0:
            self._pins.pop(pts)
            self._enc_cache.pop(hit.data)      # the encoded copy of the pinned rows goes with them
            hit.drop()

    def forget(self, pts=None):
        """Drop the pinned device copy of `pts` (or of everything) and the spare Phi buffers."""
        if pts is not None:
            self.unpin(pts)
            return
        for hit in self._pins:
            hit.drop()
        self._pins.clear()
        self._enc_cache.clear()
        self._pool.clear()

    def device_data(self, pts):
        """(DeviceData, transient) of what K1 reads: with an encoder the ENCODED rows of `pts`, otherwise its rows."""
        dd, transient = self._raw_device_data(pts)
        if self.encoder is None:
            return dd, transient
        return self._encoded(dd, transient or dd._transient), transient

    def _encoded(self, dd, transient):
        """Raw device rows -> encoded device rows.  Resident rows: cached per (rows, encoder version), re-encoded when the
        version has moved.  Transient rows (a slot, a take(out=) buffer): into the projector's one re-used output buffer."""
        enc = self.encoder
        if dd.shape[1] != enc.widths[0] + self.pass_cols:
            raise ValueError('data rows have %d columns, the encoder takes %d + %d pass-through'
                             % (dd.shape[1], enc.widths[0], self.pass_cols))
        if transient:
            self.encode_launches += 1
            self._enc_out = dd.encode(enc, pass_cols=self.pass_cols, dtype=self.encoded_dtype, out=self._enc_out, transient=True)
            return self._enc_out
        version, out = self._enc_cache.get(dd, (None, None))
        if version != enc.version:
            self.encode_launches += 1
            out = dd.encode(enc, pass_cols=self.pass_cols, dtype=self.encoded_dtype)
            self._enc_cache.put(dd, (enc.version, out))
        return out

    def _raw_device_data(self, pts):
        """(DeviceData, transient): transient inputs live in a re-used upload slot that the next call overwrites."""
        if isinstance(pts, DeviceData):
            return pts, False
        dd = self.pinned(pts)
        if dd is not None:
            return dd, False
        pts = np.atleast_2d(pts)
        if pts.shape[0] < _SMALL_ROWS:
            return upload_slot(self._slots, pts.shape[1], self.ctx).update(pts), True
        return DeviceData(pts, ctx=self.ctx, dtype=_resident_dtype(pts)), False      # live array, uploaded for this call

    def _zero_feature_keys(self, pts, d, encoded=False):
        """Sorted unique y of the rows of `pts` whose d features are all zero (host array: NumPy; resident rows: one device scan).
        With an encoder the ENCODED features are what counts (ReLU features are all zero for whole regions of x): host rows
        go through enc(pts) -- the device's bits --, device rows are encoded first; `encoded`: `pts` already holds features.
        Cached per resident DeviceData and per large ndarray; a buffer that take(out=) refills in place is scanned every time."""
        if self.encoder is not None and not encoded:      # what holds the features: the encoded device copy, or enc(host rows)
            if isinstance(pts, DeviceData) or self.pinned(pts) is not None:
                pts = self.device_data(pts)[0]
            else:
                pts = self.encoder(np.atleast_2d(pts), pass_cols=self.pass_cols, dtype=self.encoded_dtype)
        on_device = isinstance(pts, DeviceData)
        cached = not pts._transient if on_device else isinstance(pts, np.ndarray) and np.atleast_2d(pts).shape[0] >= _SMALL_ROWS
        keys = self._key_cache.get(pts) if cached else None
        if keys is None:
            keys = self._scan_device(pts, d) if on_device else self._scan_host(pts, d)
            if cached:
                self._key_cache.put(pts, keys)
        return keys

    @staticmethod
    def _scan_device(dd, d):
        cap = 65536
        out, n = np.empty(cap), C.c_int64()
        N.call('bc_data_zero_feature_keys', dd.h, int(d), cap, _ptr(out), C.byref(n))
        if n.value > cap:
            raise ValueError('%d data rows have all-zero features: more than the %d the host route for constant rows handles'
                             % (n.value, cap))
        return np.unique(out[:n.value])

    @staticmethod
    def _scan_host(pts, d):
        arr = np.atleast_2d(np.asarray(pts))
        if arr.dtype != np.float32 or arr.shape[0] < _SMALL_ROWS:      # (a large float32 array is scanned as it is: the zero test
            arr = np.atleast_2d(np.asarray(pts, dtype=np.float64))     # is exact in either type, the few keys are widened below)
        return np.unique(arr[~arr[:, :d].any(axis=1), d].astype(np.float64))

    def _stage_host_constants(self, pts, model_id, params, more=None):
        """Before a beta-projection on a host whose NumPy the library does not restate: the constants of the all-zero-feature
        rows of `pts` (and of `more`, a second row set projected by the same native call), evaluated here, go to the kernel
        (bc_ctx_set_constant_row_values).  No-op everywhere else."""
        if not self._host_constants or model_id != self.model.beta_model_id:
            return
        params = np.ascontiguousarray(params, dtype=np.float64)
        d = self.model.data_width(np.atleast_2d(self.samples).shape[1]) - 1
        keys = self._zero_feature_keys(pts, d)
        if more is not None:
            keys = np.union1d(keys, self._zero_feature_keys(more, d, encoded=True))      # (vi_gradient has encoded them)
        vals = np.ascontiguousarray(self.model.host_constants(keys, params[1]), dtype=np.float64) if keys.size else np.zeros(0)
        self.constant_rows_from_host = int(keys.size)
        N.call('bc_ctx_set_constant_row_values', self.ctx.h, int(model_id), _ptr(params), int(params.shape[0]),
               _ptr(np.ascontiguousarray(keys)), _ptr(vals), int(keys.size))

    def _theta(self, shape):
        """(Theta as K1 reads it, S) for data rows of `shape` (a DeviceData's or a host array's)."""
        theta = self.model.theta_for_device(self.samples)
        if shape[1] != self.model.data_width(theta.shape[1]):
            raise ValueError('data rows have %d columns, model expects %d for %d-dimensional samples'
                             % (shape[1], self.model.data_width(theta.shape[1]), theta.shape[1]))
        return theta, int(theta.shape[0])

    def _run_from_host(self, pts, model_id, params, keep=False):
        """project(ndarray) for a LARGE live host array: upload and K1 pipelined in one native call (bc_project_from_host;
        Phi, norms and column sums are the resident path's bit for bit).  Returns (DevicePhi, DeviceData of the uploaded
        rows); the latter is dropped by the caller unless it wants the rows to stay in HBM."""
        self._stage_host_constants(pts, model_id, params)
        f32 = _resident_dtype(pts) is not None       # a float32 array goes up as it is: no float64 host copy, half the bytes
        pts = _as_rows(np.atleast_2d(pts), np.dtype(np.float32 if f32 else np.float64), 'data')
        theta, S = self._theta(pts.shape)
        params = np.ascontiguousarray(params, dtype=np.float64)
        rows = []

        def fill(h):
            dh = C.c_void_p()
            N.call('bc_project_from_host_f32' if f32 else 'bc_project_from_host', self.ctx.h, _ptr(pts), int(pts.shape[0]), int(pts.shape[1]), int(model_id), _ptr(theta), S,
                   _ptr(params), int(params.shape[0]), 0, C.byref(dh), C.byref(h))
            rows.append(DeviceData._adopt(dh, pts.shape, self.ctx))
        return self._pool.lend(pts.shape[0], S, fill), rows[0]

    def _run(self, pts, model_id, params):
        if (self.encoder is None and isinstance(pts, np.ndarray) and pts.ndim == 2 and pts.shape[0] >= _PIPE_ROWS
                and self.pinned(pts) is None):
            return self._run_from_host(pts, model_id, params)[0]      # (with an encoder: upload, encode, bc_project -- below)
        self._stage_host_constants(pts, model_id, params)
        dd, transient = self.device_data(pts)
        theta, S = self._theta(dd.shape)
        params = np.ascontiguousarray(params, dtype=np.float64)
        return self._pool.lend(dd.shape[0], S, lambda h: N.call(
            'bc_project', self.ctx.h, dd.h, int(model_id), _ptr(theta), S, _ptr(params), int(params.shape[0]),
            0 if transient else int(dd.row_offset), C.byref(h)))

    # -- the store-free paths of the gradient loop (bcores.py:141-146, sparsevi.py:129-134): of the N x S projection of
    # the data rows only the S column sums are needed there, so K1 keeps its column partials and writes no Phi
    def _ids(self, beta):
        """(model id, its parameters as the native calls take them) of the plain (beta None) or the beta-likelihood."""
        model_id, params = (self.model.model_id, self.model.params()) if beta is None \
            else (self.model.beta_model_id, self.model.params(beta=beta))
        return model_id, np.ascontiguousarray(params, dtype=np.float64)

    def colsum(self, pts, beta=None, comm=None):
        """`project(pts).sum(axis=0)` (beta None) / `project_f(pts, beta).sum(axis=0)` without materialising the
        projection: bc_project_colsum, bit-identical to the column sums of the materialised Phi.  `comm`: a native
        communicator handle (ShardComm.native_comm) -- the sum then runs over all ranks' shards.  Returns None when the
        store-free kernel does not cover the request (S > 256); the caller projects and sums instead."""
        dd, _ = self.device_data(pts)
        theta, S = self._theta(dd.shape)
        if S > 256:
            return None
        model_id, params = self._ids(beta)
        self._stage_host_constants(pts, model_id, params)
        out = np.empty(S)
        N.call('bc_project_colsum', self.ctx.h, dd.h, int(model_id), _ptr(theta), S, _ptr(params), int(params.shape[0]),
               comm, _ptr(out))
        return out

    def vi_gradient(self, data, core_pts, w, sum_scaling=1., beta=None, comm=None, want_resid=False, overlap=None,
                    want_beta_grad=False):
        """One gradient of the greedy-VI weight optimisation in one native call (bc_vi_gradient): with the current
        samples, -corevecs.dot(sum_scaling * vecs.sum(axis=0) - w.dot(corevecs)) / S for vecs = projection of `data`
        (resident DeviceData, pinned array, or a live array that is uploaded for this call like project() does) and
        corevecs = projection of `core_pts`.  None if not covered (S > 256, no coreset rows, or a coreset too large
        for the staging area).  `overlap`: a callable run on the host between the enqueue and the wait (bc_vi_gradient_begin /
        _end), i.e. beside the GPU -- the samplers' `prefetch` (drawing the next sample matrix's normals) goes there.
        `want_beta_grad` (learn_beta, needs `beta` and a model with a beta-gradient): the same call through
        bc_vi_beta_gradient -- the same bits in grad and resid -- which also projects the coreset rows' row-centred beta-gradient
        G and returns (grad, beta_dots[, resid]) with beta_dots = G.dot(resid) (bcores.py:134-137)."""
        if want_beta_grad and (beta is None or self.model.beta_grad_model_id is None):
            raise ValueError('beta-gradient was requested but this model has none')
        dd, _ = self.device_data(data)
        core = np.ascontiguousarray(np.atleast_2d(core_pts), dtype=np.float64)
        if self.encoder is not None and core.size:      # the coreset rows arrive raw: the device's own features of them
            core = np.ascontiguousarray(self.encoder(core, pass_cols=self.pass_cols, dtype=self.encoded_dtype))
        m = int(core.shape[0])
        theta, S = self._theta(dd.shape)
        if S > VI_MAX_SAMPLES or m == 0 or m * (core.shape[1] + 1) > VI_MAX_CORE_DOUBLES:      # (also keeps 2 m + S within the native staging area)
            return None
        if core.shape[1] != dd.shape[1]:
            raise ValueError('coreset rows have %d columns, data rows %d' % (core.shape[1], dd.shape[1]))
        w = np.ascontiguousarray(w, dtype=np.float64)
        if w.shape != (m,):
            raise ValueError('one weight per coreset row')
        model_id, params = self._ids(beta)
        self._stage_host_constants(data, model_id, params, more=core)
        entry, out = 'bc_vi_gradient', [np.empty(m)]
        if want_beta_grad:
            if N.load().bc_model_beta_grad(int(model_id)) != int(self.model.beta_grad_model_id):
                raise ValueError('model %d is not the beta-gradient of model %d' % (self.model.beta_grad_model_id, model_id))
            entry = 'bc_vi_beta_gradient'
            out.append(np.empty(m))      # beta_dots
        N.call(entry + '_begin', self.ctx.h, dd.h, _ptr(core), m, int(model_id), _ptr(theta), S, _ptr(params),
               int(params.shape[0]), _ptr(w), float(sum_scaling), comm)
        resid = np.empty(S) if want_resid else None
        try:
            if overlap is not None:
                overlap()
        finally:
            N.call(entry + '_end', self.ctx.h, *[_ptr(a) for a in out + [resid]])
        if want_resid:
            out.append(resid)
        return tuple(out) if len(out) > 1 else out[0]

    def vi_optimize(self, data, core_pts, w0, opt_itrs, step_sched, n_subsample=None, n_total=None, beta=None, chunk_steps=0,
                    want_trace=False, timings=None):
        """The whole weight optimisation of one greedy-VI step -- `nn_opt(w0, grd, opt_itrs, step_sched)` with a fresh posterior
        draw and a fresh (sub-sampled) projection per gradient (bcores.py:141-150) -- enqueued on the device in chunks of steps
        (bc_vi_optimize_begin / _chunk_begin / _chunk_end / _end): the draw (k_vi_sampler, or k_vi_laplace for a
        LogisticLaplaceSampler(solver='newton'), whose `_mode` afterwards is the last step's mode), both projections, the M x S algebra
        and the ADAM update never leave the GPU, the host waits once per chunk.  Returns the new weights (with `want_trace`:
        (weights, opt_itrs x m weights after every step)), equal to the host loop's to rounding, or None when the run is not
        covered: rows that are not resident, an encoder, a sampler without `device_spec()`, D > 128, S > 256, a coreset too
        large for the staging area, a model that does not go with the sampler, opt_itrs <= 0 (the host's nn_opt then returns
        w0, and so does the caller's host loop).

        The random numbers are the HOST's, in the reference's order, step by step: the sampler's S x D normals (`_normals`: a
        prefetched block first, an injected rng honoured), then `np.random.randint(n_total, size=n_subsample)`.  The next chunk
        is drawn while the device runs the current one; nothing is drawn past the last step.  A posterior precision matrix
        that is not positive definite raises np.linalg.LinAlgError, as LAPACK does in the host loop.
        Two things differ from the host loop and are not papered over: after such a LinAlgError the streams have advanced by
        every chunk drawn so far (the failing step's whole chunk and the one drawn beside it), where the host loop stops at
        the failing step; and `self.samples` is NOT the last step's Theta afterwards -- that never leaves the device -- but
        what the last `update()` left (GreedyVICoreset calls update() before it reads samples, in _select).
        `timings` (a dict): receives 'draw_s' (host seconds spent drawing) and 'device_ms' (GPU time of the chunks' steps)."""
        spec = getattr(self.sampler, 'device_spec', None)
        if spec is None or self.encoder is not None or not isinstance(data, DeviceData) or data._transient:
            return None
        spec = spec()
        if spec is None:                # (a sampler the device cannot restate as configured: the logistic one with BFGS)
            return None
        kind, sp = spec
        sp = np.ascontiguousarray(sp, dtype=np.float64)
        D = int(self.sampler._dim())
        S = int(self.projection_dimension)
        core = np.ascontiguousarray(np.atleast_2d(core_pts), dtype=np.float64)
        m = int(core.shape[0])
        model_id, params = self._ids(beta)
        model_cls = (LinearRegression, GaussianLocation, LogisticRegression)[kind]      # the likelihood each sampler kind is the posterior of
        if not isinstance(self.model, model_cls) or int(model_id) not in (self.model.model_id, self.model.beta_model_id):
            return None
        if opt_itrs <= 0 or D > VI_OPT_MAX_DIM or S > VI_MAX_SAMPLES or m == 0 or m * (core.shape[1] + 1) > VI_MAX_CORE_DOUBLES \
                or data.shape[1] != self.model.data_width(D) or core.shape[1] != data.shape[1]:
            return None
        w0 = np.ascontiguousarray(w0, dtype=np.float64)
        if w0.shape != (m,):
            raise ValueError('one weight per coreset row')
        n_sub = 0 if n_subsample is None else int(n_subsample)
        n_total = int(data.shape[0] if n_total is None else n_total)
        self._stage_host_constants(data, model_id, params, more=core)
        steps = np.ascontiguousarray(adam_step_arrays(int(opt_itrs), step_sched))
        lib = N.load()
        chunk = int(chunk_steps) if chunk_steps else int(lib.bc_vi_optimize_auto_chunk(S, D, n_sub))
        draw_s, h = [0.], self.ctx.h
        N.call('bc_vi_optimize_begin', self.ctx.h, data.h, _ptr(core), m, int(model_id), _ptr(params), int(params.shape[0]),
               int(kind), _ptr(sp), S, _ptr(w0), int(opt_itrs), _ptr(steps), n_sub,
               float(n_total) / n_sub if n_sub else 1., 1 if want_trace else 0)
        out = np.empty(m)
        trace = np.empty((int(opt_itrs), m)) if want_trace else None

        def chunk_begin(drawn):
            E, idx = drawn
            N.call('bc_vi_optimize_chunk_begin', h, _ptr(E), _ptr(idx) if idx is not None else None, int(E.shape[0]))
            return E.shape[0]

        def chunk_end():
            status = lib.bc_vi_optimize_chunk_end(h)
            if status == N.BC_NUMERICAL_PRECISION:
                raise np.linalg.LinAlgError(N.last_error())
            return status
        run_chunks(opt_itrs, chunk, step_draws(self.sampler, S, D, n_total, n_sub, seconds=draw_s), chunk_begin, chunk_end,
                   close=lambda: lib.bc_vi_optimize_end(h, None, None),
                   finish=lambda: N.call('bc_vi_optimize_end', h, _ptr(out), _ptr(trace) if want_trace else None))
        if timings is not None:
            timings['draw_s'], timings['device_ms'] = draw_s[0], device_ms('bc_vi_optimize_device_ms', self.ctx)
        self.vi_optimize_calls += 1
        if kind == 2:
            # the mode the last step ended at: where the sampler's next call -- on the host or in the next run -- starts
            self.sampler._mode = self.vi_last_mode()['mode']
        return (out, trace) if want_trace else out

    def vi_last_draw(self):
        """What the last posterior draw of the most recent `vi_optimize` run on this projector's context left on the device
        (bc_vi_optimize_last_draw; a seam for tests, nothing is launched): a dict of `theta` (S x D, what K1 read: for the
        Gaussian sampler Theta . Siginv^T), `saux` (S) and `raw` (S x D) -- the Gaussian sampler's theta^T Siginv theta and its
        draw before Siginv is applied, zeros for the linear-regression sampler -- and `pad_max`, the largest magnitude left
        in the zero padding of the block K1 reads (anything but 0.0 is a defect).  After a run whose first step raised
        LinAlgError everything reads 0.  Raises when the context's last run was not one of this projector's shape (S, D)."""
        S, D = int(self.projection_dimension), int(self.sampler._dim())
        theta, saux, raw, pad = np.empty((S, D)), np.empty(S), np.empty((S, D)), C.c_double()
        N.call('bc_vi_optimize_last_draw', self.ctx.h, S, D, _ptr(theta), _ptr(saux), _ptr(raw), C.byref(pad))
        return dict(theta=theta, saux=saux, raw=raw, pad_max=pad.value)


    def vi_last_mode(self):
        """What the last Laplace fit of the most recent `vi_optimize` run with the logistic sampler left on the device
        (bc_vi_laplace_last_mode; a seam for tests, nothing is launched): a dict of `mode` (D), `newton` (the Newton steps of
        that fit), `halvings` (of its last line search) and `newton_total` (the Newton steps of the whole run).  Raises when
        the context's last run was of another sampler kind or dimension."""
        D = int(self.sampler._dim())
        mode, counts = np.empty(D), np.zeros(3, dtype=np.int32)
        N.call('bc_vi_laplace_last_mode', self.ctx.h, D, _ptr(mode), _ptr(counts))
        return dict(mode=mode, newton=int(counts[0]), halvings=int(counts[1]), newton_total=int(counts[2]))


def is_device_projector(prj):
    """True for the projectors whose input may be a DeviceData (K1 on the GPU): what decides whether a coreset sub-samples
    resident rows on the device (DeviceData.take) or hands host rows to a black-box callable."""
    return isinstance(prj, _DeviceProjectorBase)


class DeviceProjector(_DeviceProjectorBase):
    """GPU counterpart of BlackBoxProjector: `project(pts)` returns a DevicePhi."""

    def project(self, pts, grad=False):
        """projector.py:23-32.  With `grad` also the x-gradient tensor of the log-likelihood at `pts` (M x S x W host
        array, centred over its last axis as the reference does it): bc_project_grad_x, meant for the coreset's
        pseudo-points (BatchPSVICoreset, bpsvi.py:39-40)."""
        lls = self._run(pts, self.model.model_id, self.model.params())
        if not grad:
            return lls
        return lls, self._grad_x(pts)

    def _grad_x(self, pts):
        if not self.model.has_grad_x:
            raise ValueError('grad_loglikelihood was requested but this model has none')
        if self.encoder is not None:
            raise ValueError('grad_loglikelihood was requested but there is no x-gradient through a feature encoder')
        dd, _ = self.device_data(pts)
        theta = self.model.theta_for_device(self.samples)
        params = np.ascontiguousarray(self.model.params(), dtype=np.float64)
        out = np.empty((dd.shape[0], int(theta.shape[0]), dd.shape[1]))
        N.call('bc_project_grad_x', self.ctx.h, dd.h, int(self.model.model_id), _ptr(theta), int(theta.shape[0]),
               _ptr(params), int(params.shape[0]), _ptr(out))
        return out

    def psvi_gradient(self, data, pts, w, sum_scaling=1., want_resid=False, overlap=None):
        """BatchPSVICoreset's gradient (bpsvi.py:47-57) in one native call (bc_psvi_gradient): with the current samples,
        resid = sum_scaling * project(data).sum(axis=0) - w.dot(corevecs), g_w = -corevecs.dot(resid) / S and
        g_p = -(w[:, None, None] * pgrads * resid[None, :, None]).sum(axis=1) / S for (corevecs, pgrads) =
        project(pts, grad=True) -- without the M x S x W tensor `pgrads`: only the M x W result comes back, in the same download
        as g_w.  g_w and resid carry the bits of vi_gradient on the same inputs.  Returns (g_w, g_p[, resid]), or None when the
        call is not covered: S > 256, no points, points too many or too wide for the staging area, a model without an
        x-gradient, an encoder.  `overlap`: as in vi_gradient."""
        if self.encoder is not None or not self.model.has_grad_x:
            return None
        dd, _ = self.device_data(data)
        core = np.ascontiguousarray(np.atleast_2d(pts), dtype=np.float64)
        m = int(core.shape[0])
        theta, S = self._theta(dd.shape)
        if S > VI_MAX_SAMPLES or core.size == 0 or m * (core.shape[1] + 1) > VI_MAX_CORE_DOUBLES or core.shape[1] > PSVI_MAX_ROW_DOUBLES:
            return None
        if core.shape[1] != dd.shape[1]:
            raise ValueError('points have %d columns, data rows %d' % (core.shape[1], dd.shape[1]))
        w = np.ascontiguousarray(w, dtype=np.float64)
        if w.shape != (m,):
            raise ValueError('one weight per point')
        model_id, params = self._ids(None)
        self._stage_host_constants(data, model_id, params, more=core)
        N.call('bc_psvi_gradient_begin', self.ctx.h, dd.h, _ptr(core), m, int(model_id), _ptr(theta), S, _ptr(params),
               int(params.shape[0]), _ptr(w), float(sum_scaling))
        g_w, g_p = np.empty(m), np.empty(core.shape)
        resid = np.empty(S) if want_resid else None
        try:
            if overlap is not None:
                overlap()
        finally:
            N.call('bc_psvi_gradient_end', self.ctx.h, _ptr(g_w), _ptr(g_p), _ptr(resid))
        return (g_w, g_p, resid) if want_resid else (g_w, g_p)


class DeviceBetaProjector(_DeviceProjectorBase):
    """GPU counterpart of BetaBlackBoxProjector: `project_f(pts, beta)` returns a DevicePhi.
    Also offers `project` (plain log-likelihood), which the reference's class lacks."""

    def project(self, pts, grad=False):
        if grad:
            raise NotImplementedError
        return self._run(pts, self.model.model_id, self.model.params())

    def project_f(self, pts, beta, grad=False):
        bls = self._run(pts, self.model.beta_model_id, self.model.params(beta=beta))
        if not grad:
            return bls
        if self.model.beta_grad_model_id is None:
            raise ValueError('beta-gradient was requested but this model has none')
        g = self._run(pts, self.model.beta_grad_model_id, self.model.params(beta=beta))
        return bls, g
