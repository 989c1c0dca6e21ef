"""BatchPSVICoreset (bayesiancoresets/coreset/bpsvi.py:6-65): a pseudo-coreset -- `sz` points initialised on data
rows and then MOVED, together with their weights, by `opt_itrs` projected-ADAM steps.

Every gradient needs (bpsvi.py:27-57)
  * the projection of the data (all rows, or `n_subsample_opt` random ones) and its column sums: K1 + K2 on the GPU
    with a DeviceProjector, only the S-vector comes back;
  * the projection of the `sz` pseudo-points and the x-gradient tensor of their log-likelihoods (sz x S x W,
    projector.py:27-32): bc_project / bc_project_grad_x on the points, which live on the host between steps because
    the optimiser (util/opt.py partial_nn_opt) updates them there.
With a BlackBoxProjector the reference's NumPy expressions run on whatever the callables return and the N-row column
sum still runs on the GPU."""
import numpy as np

from .. import _native as N
from .._runs import device_ms, pack_problems, run_chunks, step_draws
from ..device import DeviceData, DevicePhi, _ptr
from ..likelihoods import GaussianLocation, LogisticRegression
from ..util.opt import adam_step_arrays, partial_nn_opt
from .coreset import Coreset
from .residency import keep_resident, pin_for, resident_copy_of_view, sub_rows

# limits of the batched run (include/beta_cores_psvi_many.h)
PSVI_MANY_MAX_DIM, PSVI_MANY_MAX_SAMPLES, PSVI_MANY_MAX_SUB = 128, 256, 262144
PSVI_MANY_MAX_PROBLEMS, PSVI_MANY_MAX_POINTS, PSVI_MANY_MAX_WORK_DOUBLES = 4096, 4096, 1 << 27
_SAMPLER_GAUSS, _SAMPLER_LOGISTIC = 1, 2          # BC_VI_SAMPLER_GAUSS, BC_VI_SAMPLER_LOGISTIC


class PSVICurve(list):
    """What BatchPSVICoreset.build_many returns: one `(wts, pts, idcs)` per size, as `get()` gives it after `build(1, m)` (None for
    a marked size).  `route`: 'batched' or 'each'; `marked`: the positions in `sizes` whose problem met a weight, value, gradient
    or pivot that is not finite (batched route); `device_ms`: GPU time of the run's steps (0.0 on the 'each' route)."""

    def __init__(self, entries, route, marked=(), device_ms=0.):
        super().__init__(entries)
        self.route, self.marked, self.device_ms = route, list(marked), float(device_ms)


def psvi_many_run(data, pts, wts, S, opt_itrs, steps, draw, n_sub, n_total=None, start=None, diag=False, chunk_steps=0,
                  model_id=None, sampler_kind=_SAMPLER_LOGISTIC, on_chunk=None, model_params=None, sampler_params=None):
    """The native batched run (bc_psvi_many_begin / _chunk_begin / _chunk_end / _end) on resident rows `data` (a DeviceData):
    problem p starts at points `pts[p]` (m_p x D) with weights `wts[p]` and takes `opt_itrs` joint projected-ADAM steps of sizes
    `steps[p]` (opt_itrs values); all problems share each step's draws.  `draw(k)` returns the next k steps' (normals k x S x D,
    row numbers k x n_sub); it is called for chunk i + 1 while the device runs chunk i, and never past the last step.
    `on_chunk(done)`: called after every chunk has been waited for (tests read the seam there).
    The default is the logistic kind (N(0, I) prior, `start`, `diag`).  The Gaussian-location kind: `model_id` of
    likelihoods.GaussianLocation, `sampler_kind=1`, `model_params` = the model's `params()` ({logdetSig, Siginv}) and
    `sampler_params` = GaussianPosteriorSampler.device_spec()[1] (mu0 | Sig0inv | Siginv); no `start`, no `diag` (bc_psvi_curve_begin).
    Returns a dict: `w`, `pts` (lists; None for a marked problem), `modes` (P x D), `status` (P), `marked`, `device_ms`."""
    lib = N.load()
    P = len(pts)
    if int(opt_itrs) < 1:
        raise ValueError('psvi_many_run: opt_itrs must be at least 1, got %d' % opt_itrs)
    D = int(data.shape[1])
    pk, wk, row_ptr = pack_problems([(np.atleast_2d(p), np.atleast_1d(w)) for p, w in zip(pts, wts)], width=D)
    R = int(row_ptr[-1])
    if pk.shape != (R, D) or wk.shape != (R,):
        raise ValueError('points must have %d columns and one weight each' % D)
    steps = np.ascontiguousarray(steps, dtype=np.float64)
    if steps.shape != (P, int(opt_itrs)):
        raise ValueError('steps must be P x opt_itrs')
    moments = np.ascontiguousarray(adam_step_arrays(int(opt_itrs), lambda i: 0.)[1:])
    st = None if start is None else np.ascontiguousarray(start, dtype=np.float64)
    if st is not None and st.shape != (P, D):
        raise ValueError('start must be P x D')
    n_total = int(data.shape[0] if n_total is None else n_total)
    model_id = LogisticRegression().model_id if model_id is None else model_id
    ctx = data.ctx
    begin = (ctx.h, data.h, int(model_id), int(sampler_kind), 1 if diag else 0, _ptr(pk), _ptr(wk), _ptr(row_ptr), P,
             _ptr(st) if st is not None else None, int(S), int(opt_itrs), _ptr(steps), _ptr(moments), int(n_sub),
             float(n_total) / n_sub if n_sub else 1.)
    if model_params is None and sampler_params is None and int(sampler_kind) == _SAMPLER_LOGISTIC:
        N.call('bc_psvi_many_begin', *begin)
    else:
        mp = np.ascontiguousarray(np.zeros(0) if model_params is None else model_params, dtype=np.float64).ravel()
        sp = np.ascontiguousarray(np.zeros(0) if sampler_params is None else sampler_params, dtype=np.float64).ravel()
        N.call('bc_psvi_curve_begin', *begin, _ptr(mp) if mp.size else None, int(mp.size), _ptr(sp) if sp.size else None, int(sp.size))
    chunk = int(chunk_steps) if chunk_steps else int(lib.bc_psvi_many_auto_chunk(int(S), D, int(n_sub)))
    ow, op, om, ost = np.full(R, np.nan), np.full((R, D), np.nan), np.full((P, D), np.nan), np.zeros(P, dtype=np.int32)

    def chunk_begin(drawn):
        E = np.ascontiguousarray(drawn[0], dtype=np.float64)
        idx = np.ascontiguousarray(drawn[1], dtype=np.int64)
        k = int(E.shape[0])
        if E.shape != (k, int(S), D) or idx.shape != (k, int(n_sub)):
            raise ValueError('draw(k) must return k x S x D normals and k x n_sub row numbers')
        N.call('bc_psvi_many_chunk_begin', ctx.h, _ptr(E), _ptr(idx), k)
        return k
    run_chunks(opt_itrs, chunk, draw, chunk_begin, lambda: lib.bc_psvi_many_chunk_end(ctx.h, None),
               close=lambda: lib.bc_psvi_many_end(ctx.h, None, None, None, None),
               finish=lambda: N.call('bc_psvi_many_end', ctx.h, _ptr(ow), _ptr(op), _ptr(om), _ptr(ost)), on_chunk=on_chunk)
    ok = ost == N.BC_OK
    return dict(w=[ow[row_ptr[p]:row_ptr[p + 1]] if ok[p] else None for p in range(P)],
                pts=[op[row_ptr[p]:row_ptr[p + 1]] if ok[p] else None for p in range(P)], modes=om, status=ost,
                marked=[p for p in range(P) if not ok[p]], device_ms=device_ms('bc_psvi_many_device_ms', ctx))


def psvi_many_last_step(ctx, sizes, D, S):
    """What the last executed step of the most recent batched run on `ctx` left on the device (bc_psvi_many_last_step; a seam for
    tests, nothing is launched): a dict of packed arrays -- `w_before`, `pts_before`, `mode`, `theta`, `target`, `resid`, `gw`,
    `gp`, `w`, `pts`, `mom1_w`, `mom1_p`, `mom2_w`, `mom2_p`, `newton` (P x 2: Newton steps of the last fit | of the run), `flag`
    (P) -- and `row_ptr`.  Gaussian kind: `mode` is the posterior mean, `theta` the draw itself (not Siginv-multiplied), `newton` 0."""
    P, R = len(sizes), int(np.sum(sizes))
    row_ptr = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    shapes = dict(w_before=(R,), pts_before=(R, D), mode=(P, D), theta=(P, S, D), target=(P, S), resid=(P, S), gw=(R,), gp=(R, D),
                  w=(R,), pts=(R, D), mom1_w=(R,), mom1_p=(R, D), mom2_w=(R,), mom2_p=(R, D))
    out = {k: np.empty(v) for k, v in shapes.items()}
    out['newton'], out['flag'] = np.zeros((P, 2), dtype=np.int32), np.zeros(P, dtype=np.int32)
    N.call('bc_psvi_many_last_step', ctx.h, R, P, int(D), int(S), *[_ptr(out[k]) for k in list(shapes) + ['newton', 'flag']])
    out['row_ptr'] = row_ptr
    return out


class BatchPSVICoreset(Coreset):
    def __init__(self, data, ll_projector, opt_itrs, n_subsample_opt=None, step_sched=lambda m: lambda i: 1. / (1. + i),
                 mup=None, Zmean=None, SigpInv=None, diagnostics=False, comm=None, pin_data=True, fused_gradient=False, **kw):
        if comm is not None and comm.world > 1:
            raise NotImplementedError('BatchPSVICoreset initialises its points from rows of the whole data set; '
                                      'row shards are not supported')
        self.data, self.ll_projector = data, ll_projector
        self.opt_itrs, self.step_sched = opt_itrs, step_sched
        self.mup, self.SigpInv = mup, SigpInv
        n = data.shape[0]
        self.n_subsample_opt = n_subsample_opt if n_subsample_opt is None else min(n, n_subsample_opt)   # bpsvi.py:11
        # opt-in: the whole gradient in one native call (DeviceProjector.psvi_gradient) where the projector offers it and covers
        # the shape; every other gradient takes the path below it.  fused_gradient_calls counts those that took it.
        self.fused_gradient, self.fused_gradient_calls, self._grad_calls = bool(fused_gradient), 0, 0
        self._sub_buf = None         # sub-samples of resident rows are taken into this one device buffer
        # every full-data gradient re-projects ALL rows: keep them in HBM (pinned: read-only on the host; a view: copied once)
        self._resident = keep_resident(self, data, ll_projector, pin_data and self.n_subsample_opt is None)
        super().__init__(**kw)

    # ---- bpsvi.py:17-25: a fresh random initialisation of all `sz` points, then the optimisation (itrs is unused)
    def _build(self, itrs, sz):
        n = self.data.shape[0]
        self.idcs = np.random.choice(n, size=sz, replace=False)
        self.pts = self.data[self.idcs]
        self.wts = np.full(sz, n / sz)
        self._optimize()

    # ---- bpsvi.py:27-43.  Of the data's projection the gradient only uses its column sums (bpsvi.py:52), so that
    # S-vector (K2, on the device) is what this returns, already scaled to the whole data set.
    def _rows(self):
        """(the rows this gradient projects, their scale to the whole data set): all rows, or a fresh random sub-sample"""
        m = self.n_subsample_opt
        if m is None:
            return (self._resident if self._resident is not None else self.data), 1.
        sub_idcs, scale = np.random.randint(self.data.shape[0], size=m), self.data.shape[0] / m
        rows = sub_rows(self.data, sub_idcs, self.ll_projector, out=self._sub_buf)      # resident rows stay in HBM
        if isinstance(rows, DeviceData):
            self._sub_buf = rows
        return rows, scale

    def _data_term(self, rows=None, scale=None):
        if rows is None:
            rows, scale = self._rows()
        if hasattr(self.ll_projector, 'colsum'):       # device projector: store-free K1, the bits of project().sum(axis=0)
            b = self.ll_projector.colsum(rows)
            if b is not None:
                return scale * b
        vecs = self.ll_projector.project(rows)
        if not isinstance(vecs, DevicePhi):            # black-box projector: a host array, reduced on the device
            ctx = getattr(self.ll_projector, 'ctx', None)
            vecs = DevicePhi.from_host(np.ascontiguousarray(vecs, dtype=np.float64), ctx=ctx)
        return scale * vecs.sum(axis=0)

    def _point_terms(self, p, n_samples):
        if p.size == 0:
            return np.zeros((0, n_samples)), np.zeros((0, n_samples, p.shape[1]))
        lls, glls = self.ll_projector.project(p, grad=True)
        return np.asarray(lls), np.asarray(glls)

    def _gradient(self, x, sz, d):
        """bpsvi.py:47-57: d/d(weights, points) of the squared tangent-space residual, estimated over the S samples"""
        w, p = x[:sz], x[sz:].reshape(sz, d)
        self.ll_projector.update(w, p)                  # new Theta first (bpsvi.py:29), then the RNG draws of _rows
        rows, scale = self._rows()
        self._grad_calls += 1
        fused = getattr(self.ll_projector, 'psvi_gradient', None) if self.fused_gradient else None
        if fused is not None:
            # one native call: only g_w and the sz x d point-gradient come back.  A sampler that can draw its next normals ahead
            # of time does so beside the GPU -- except after the LAST gradient of an _optimize(): what follows that one is not
            # this loop's next sampler call (GreedyVICoreset._optimize)
            prefetch = getattr(getattr(self.ll_projector, 'sampler', None), 'prefetch', None)
            g = fused(rows, p, w, scale, overlap=prefetch if self._grad_calls < self.opt_itrs else None)
            if g is not None:
                self.fused_gradient_calls += 1
                return np.concatenate((g[0], g[1].ravel()))
        target = self._data_term(rows, scale)           # (declined, or not asked for: the same Theta, the same rows)
        corevecs, pgrads = self._point_terms(p, target.shape[0])
        resid = target - w.dot(corevecs)
        S = corevecs.shape[1]
        g_w = -corevecs.dot(resid) / S
        g_p = -(w[:, np.newaxis, np.newaxis] * pgrads * resid[np.newaxis, :, np.newaxis]).sum(axis=1) / S
        return np.concatenate((g_w, g_p.ravel()))

    def _optimize(self):
        sz, d = self.wts.shape[0], self.pts.shape[1]
        x0 = np.concatenate((self.wts, self.pts.ravel()))
        self._grad_calls = 0
        x = partial_nn_opt(x0, lambda v: self._gradient(v, sz, d), np.arange(sz), self.opt_itrs, step_sched=self.step_sched(sz))
        self.wts, self.pts = x[:sz].copy(), x[sz:].reshape(sz, d).copy()

    # ---- the whole evaluation curve: every size of `sizes` built from ONE stream state (what forked workers of the reference
    # drivers' Pool get: zellner_logreg/main.py:173-186)
    def _uncovered(self):
        """Why the batched native run does not cover this coreset's configuration (None: it does)."""
        from .projector import DeviceProjector      # (projector.py imports this package's residency module)
        prj = self.ll_projector
        if not isinstance(prj, DeviceProjector):
            return 'the projector is not a DeviceProjector'
        gauss = isinstance(prj.model, GaussianLocation)
        if not gauss and not isinstance(prj.model, LogisticRegression):
            return 'the likelihood is %s, only LogisticRegression() is covered (the linear-regression and Gaussian-location ' \
                   'kinds take the loop of single builds)' % type(prj.model).__name__
        if prj.encoder is not None:
            return 'the projector has a feature encoder'
        spec = getattr(prj.sampler, 'device_spec', None)
        spec = spec() if spec is not None else None
        if gauss:
            if spec is None or spec[0] != _SAMPLER_GAUSS:
                return 'the sampler is not a GaussianPosteriorSampler (a plain closure cannot be evaluated on the device)'
            if not np.array_equal(np.asarray(prj.sampler.Siginv, dtype=np.float64), prj.model.Siginv):
                return "the sampler's Siginv is not the model's (GaussianLocation.Siginv)"
        elif spec is None or spec[0] != _SAMPLER_LOGISTIC:
            return "the sampler is not a LogisticLaplaceSampler(solver='newton') (the reference's BFGS search stays on the host)"
        if self.n_subsample_opt is None:
            return 'n_subsample_opt is None (all rows every step, for every size its own Theta)'
        if self.opt_itrs < 1:
            return 'opt_itrs is not positive'
        if not isinstance(self.data, (DeviceData, np.ndarray)) or (isinstance(self.data, DeviceData) and self.data._transient):
            return 'the data rows are neither resident nor an array that can be uploaded once'
        return None

    def _over_limit(self, sizes):
        """A documented limit of the native run this request exceeds (None: none) -- 'auto' then takes the loop."""
        prj = self.ll_projector
        D, S = int(self.data.shape[1]), int(prj.projection_dimension)
        if not sizes:
            return 'no sizes'
        kind = _SAMPLER_GAUSS if isinstance(prj.model, GaussianLocation) else _SAMPLER_LOGISTIC
        work = N.load().bc_psvi_curve_work_doubles(int(np.sum(sizes)), len(sizes), D, S, int(self.n_subsample_opt), int(self.opt_itrs), kind)
        if work < 0 or work > PSVI_MANY_MAX_WORK_DOUBLES or max(sizes) > PSVI_MANY_MAX_POINTS:
            return 'a limit of include/beta_cores_psvi_many.h is exceeded'
        return None

    def _stream_state(self):
        smp = getattr(self.ll_projector, 'sampler', None)
        rng = getattr(smp, '_rng', None)
        return (np.random.get_state(), rng.get_state() if rng is not None else None,
                [(k, getattr(smp, k)) for k in ('_ahead', '_shape', '_mode') if hasattr(smp, k)])

    def _set_stream_state(self, st):
        smp = getattr(self.ll_projector, 'sampler', None)
        np.random.set_state(st[0])
        if st[1] is not None:
            smp._rng.set_state(st[1])
        for k, v in st[2]:
            setattr(smp, k, None if v is None else np.copy(v) if isinstance(v, np.ndarray) else v)

    def build_many(self, sizes, route='auto'):
        """The pseudo-coresets of every size in `sizes` as a PSVICurve.  Entry m is what `build(1, m)` gives when started from the
        stream state at entry (the sampler's stream for the normals, np.random for the permutation and the row numbers); on
        return the streams stand where ONE such build leaves them.  With NumPy's legacy stream `choice(n, m, replace=False)`
        consumes the same amount for every m and its result is a prefix of a larger m's, so all sizes see the same permutation
        and, step by step, the same S x D normals and the same sub-sample: common random numbers.
        route='each': that definition as code, a loop of single builds.  route='batched': all sizes stepped in lock-step in one
        device run (bc_psvi_many_*); needs a DeviceProjector with either LogisticRegression() and a
        LogisticLaplaceSampler(solver='newton'), or GaussianLocation and a GaussianPosteriorSampler whose Siginv equals the
        model's (full covariance, D <= 128, S <= 256); n_subsample_opt, opt_itrs >= 1 and no encoder; raises NotImplementedError
        naming the reason otherwise.  'auto': batched when covered and within the limits of include/beta_cores_psvi_many.h.
        This object's own wts / pts / idcs are left as they were; so is the sampler's `_mode`."""
        if route not in ('auto', 'batched', 'each'):
            raise ValueError("route must be 'auto', 'batched' or 'each'")
        sizes = [int(m) for m in sizes]
        n = self.data.shape[0]
        if any(m < 1 or m > n for m in sizes):
            raise ValueError('every size must be within 1 .. %d' % n)
        if route != 'each':
            why = self._uncovered()
            if route == 'batched' and why is not None:
                raise NotImplementedError("build_many(route='batched'): " + why)
            route = 'each' if (why is not None or (route == 'auto' and self._over_limit(sizes) is not None)) else 'batched'
        if not sizes:
            return PSVICurve([], route)
        return self._many_each(sizes) if route == 'each' else self._many_batched(sizes)

    def _many_each(self, sizes):
        mine = (self.wts, self.pts, self.idcs, self.reached_numeric_limit)
        st0, end, entries = self._stream_state(), None, []
        try:
            for m in sizes:
                self._set_stream_state(st0)
                self._clear()
                self.build(1, m)
                entries.append(self.get())
                end = self._stream_state()
        finally:
            self.wts, self.pts, self.idcs, self.reached_numeric_limit = mine
        mode0 = [kv for kv in st0[2] if kv[0] == '_mode']
        self._set_stream_state((end[0], end[1], [kv for kv in end[2] if kv[0] != '_mode'] + mode0))      # (the sampler's _mode is left alone)
        return PSVICurve(entries, 'each')

    def _many_rows(self):
        """The resident rows of the batched run: the caller's DeviceData, or this coreset's array uploaded once."""
        if isinstance(self.data, DeviceData):
            return self.data
        if getattr(self, '_many_resident', None) is None:
            if self._resident is not None:
                self._many_resident = self._resident
            elif self.data.base is not None:
                self._many_resident = resident_copy_of_view(self.data, self.ll_projector, stacklevel=4)
            else:
                self._many_resident = pin_for(self, self.data, self.ll_projector)
        return self._many_resident

    def _many_batched(self, sizes):
        prj = self.ll_projector
        smp = prj.sampler
        S, n, n_sub = int(prj.projection_dimension), int(self.data.shape[0]), int(self.n_subsample_opt)
        rows = self._many_rows()
        D = int(rows.shape[1])
        if D != int(smp._dim()):
            raise ValueError('data rows have %d columns, the sampler draws %d-dimensional samples' % (D, smp._dim()))
        kind, sp = smp.device_spec()
        sp = np.asarray(sp, dtype=np.float64)
        perm = np.random.choice(n, size=max(sizes), replace=False)      # (size m's choice is its first m entries)
        base = np.asarray(self.data[perm], dtype=np.float64)
        steps = np.array([[self.step_sched(m)(i) for i in range(self.opt_itrs)] for m in sizes], dtype=np.float64).reshape(len(sizes), self.opt_itrs)
        if kind == _SAMPLER_GAUSS:
            how = dict(model_id=prj.model.model_id, sampler_kind=_SAMPLER_GAUSS, model_params=prj.model.params(), sampler_params=sp)
        else:
            how = dict(start=np.tile(sp[:D], (len(sizes), 1)), diag=bool(sp[D]))
        res = psvi_many_run(rows, [base[:m] for m in sizes], [np.full(m, n / m) for m in sizes], S, self.opt_itrs, steps,
                            step_draws(smp, S, D, n, n_sub), n_sub, n_total=n, **how)
        entries = []
        for p, m in enumerate(sizes):
            if res['w'][p] is None:
                entries.append(None)
                continue
            keep = res['w'][p] > 0
            entries.append((res['w'][p][keep], res['pts'][p][keep, :], perm[:m][keep]))
        return PSVICurve(entries, 'batched', res['marked'], res['device_ms'])

    def error(self):
        return 0.          # bpsvi.py:64-65 leaves the KL estimate unimplemented
