"""Thin RAII wrappers over the C-ABI handles: one Context per process/GPU, data rows
resident on the device (DeviceData) and the tiled Phi matrix (DevicePhi).

DevicePhi quacks enough like the N x S ndarray `vecs` of hilbert.py:11-17 /
bcores.py:44 for the drop-in classes to work without copying it to the host:
`.shape`, `.T` (what the solvers take as A), `.sum(axis=0)` (= b), `np.asarray()`.
"""
import ctypes as C
import os
import weakref

import numpy as np

from . import _native as N

_default_ctx = None


def _as_f64(a, what):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if not a.flags['C_CONTIGUOUS']:
        raise ValueError(what + ' must be convertible to a C-contiguous float64 array')
    return a


def _storage_dtype(z, dtype):
    """The dtype a DeviceData of host rows `z` is STORED in.  dtype=None: float64, whatever `z` holds (a float32 array is
    widened on the host, as it always was).  dtype=np.float32: `z` must already BE float32 -- the library never rounds the
    caller's data -- and is uploaded as it is.  Needs no GPU."""
    if dtype is None:
        return np.dtype(np.float64)
    dt = np.dtype(dtype)
    if dt == np.float64:
        return dt
    if dt != np.float32:
        raise ValueError('DeviceData stores float64 or float32 rows, not %s' % dt)
    if getattr(z, 'dtype', None) != np.float32:
        raise ValueError('dtype=float32 takes a float32 array (got %s): the library never rounds the caller\'s data; '
                         'pass z.astype(np.float32) if that rounding is intended' % getattr(z, 'dtype', type(z).__name__))
    return dt


def _as_rows(a, dt, what):
    """C-contiguous 2-D rows of storage dtype `dt` (float32 input stays float32 when dt is float32: no float64 copy)."""
    if dt == np.float32:
        a = np.ascontiguousarray(a)
        if a.dtype != np.float32:
            raise ValueError(what + ' must be a float32 array')
        return a
    return _as_f64(a, what)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


class Context:
    """One GPU, one stream.  `stream`: integer hipStream_t handle to launch on (pass
    torch.cuda.current_stream().cuda_stream when collectives issued through
    torch.distributed must order with the kernels); None = library-owned stream."""

    def __init__(self, device=None, stream=None):
        if device is None:
            device = int(os.environ.get('LOCAL_RANK', '0')) if os.environ.get('BC_DEVICE') is None \
                else int(os.environ['BC_DEVICE'])
        h = C.c_void_p()
        N.call('bc_ctx_create', int(device), C.c_void_p(stream) if stream else None, C.byref(h))
        self.h = h
        self.device = int(device)
        self.stream_handle = int(stream) if stream else None    # None: library-owned stream
        self._fin = weakref.finalize(self, N.load().bc_ctx_destroy, h)

    def sync(self):
        N.call('bc_ctx_sync', self.h)

    def enable_timing(self, on=True):
        """on: False/0 = off, True/1 = time every launch of the dominant kernels, n > 1 = every n-th launch."""
        N.call('bc_ctx_enable_timing', self.h, int(on))

    def timing_classes(self, mask):
        """Which kernel classes enable_timing applies to (bit i = class i); default 0x7.  Classes 3-5 are the other stages of
        a greedy step (rescoring / local winner, candidate all-gather, step finish): for diagnostic passes."""
        N.call('bc_ctx_timing_classes', self.h, int(mask))

    def kernel_time(self, which):
        """(total_ms, launches) of kernel class `which` (0 = K3 sweep, 1 = K1 projection, 2 = K4 gram + reduce, 3 = rescoring /
        local winner, 4 = candidate all-gather, 5 = step finish)."""
        ms, n = C.c_double(), C.c_int64()
        N.call('bc_ctx_kernel_time', self.h, int(which), C.byref(ms), C.byref(n))
        return ms.value, n.value

    def kernel_time_reset(self):
        N.call('bc_ctx_kernel_time_reset', self.h)

    VI_PHASES = ('upload', 'k1_core_rows', 'k1_data_rows', 'colsum_reduce', 'algebra_download')

    def phase_times(self, reset=True):
        """({phase: total GPU ms}, timed calls) of the bc_vi_gradient calls made while timing was on."""
        out = np.zeros(len(self.VI_PHASES))
        n = C.c_int64()
        N.call('bc_ctx_phase_times', self.h, _ptr(out), len(self.VI_PHASES), C.byref(n), 1 if reset else 0)
        return dict(zip(self.VI_PHASES, out.tolist())), n.value


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context()
    return _default_ctx


def set_default_context(ctx):
    global _default_ctx
    _default_ctx = ctx


class DeviceData:
    """Data rows Z (n x dz, row-major) resident in HBM, stored as float64 (default) or float32.

    dtype=np.float32 keeps a float32 array as it is: half the bytes on the host link and half the HBM.  Only the storage is
    float32 -- every kernel widens the rows in registers (exact) and computes in float64, so all results have the bits the
    float64 path gives on `z.astype(np.float64)`.  rows() / [] return float64 host rows either way; take() keeps the chosen
    rows on the device."""

    _transient = False      # True once take(out=this) has refilled the rows in place: nothing about them may be cached

    def __init__(self, z=None, ctx=None, device_ptr=None, shape=None, keepalive=None, row_offset=0, dtype=None):
        if device_ptr is None:
            z = np.atleast_2d(z)
            dt = _storage_dtype(z, dtype)            # (before any context exists: a wrong dtype needs no GPU to be refused)
        else:
            dt = np.dtype(np.float64 if dtype is None else dtype)
            if dt not in (np.float64, np.float32):
                raise ValueError('DeviceData stores float64 or float32 rows, not %s' % dt)
        f32 = dt == np.float32
        self.ctx = ctx or default_context()
        self.row_offset = int(row_offset)     # global index of row 0 when the rows are one shard of a larger set
        h = C.c_void_p()
        if device_ptr is not None:
            n, dz = shape
            N.call('bc_data_from_device_f32' if f32 else 'bc_data_from_device', self.ctx.h, C.c_void_p(device_ptr), int(n), int(dz),
                   C.byref(h))
            self._keep = keepalive
        else:
            z = _as_rows(z, dt, 'data')
            n, dz = z.shape
            N.call('bc_data_from_host_f32' if f32 else 'bc_data_from_host', self.ctx.h, _ptr(z), int(n), int(dz), C.byref(h))
        self.h = h
        self.shape = (int(n), int(dz))
        self.dtype = dt
        self._fin = weakref.finalize(self, N.load().bc_data_destroy, h)

    @property
    def nbytes(self):
        """Bytes of HBM the rows take."""
        return self.shape[0] * self.shape[1] * self.dtype.itemsize

    @classmethod
    def _adopt(cls, handle, shape, ctx):
        """Wrap a bc_data handle a native call allocated (bc_project_from_host); this object owns it from here on."""
        self = cls.__new__(cls)
        self.ctx = ctx or default_context()
        self.row_offset = 0
        self.h = handle
        self.shape = (int(shape[0]), int(shape[1]))
        nb = C.c_int32()
        N.call('bc_data_elem_bytes', handle, C.byref(nb))
        self.dtype = np.dtype(np.float32 if nb.value == 4 else np.float64)
        self._fin = weakref.finalize(self, N.load().bc_data_destroy, handle)
        return self

    @classmethod
    def slot(cls, dz, cap_rows=256, ctx=None):
        """A re-usable device buffer for small row sets that change every call (coreset points,
        sub-samples): allocate once, then `update(z)` in place."""
        self = cls.__new__(cls)
        self.ctx = ctx or default_context()
        self.row_offset = 0
        h = C.c_void_p()
        N.call('bc_data_create', self.ctx.h, int(cap_rows), int(dz), C.byref(h))
        self.h = h
        self.shape = (0, int(dz))
        self.dtype = np.dtype(np.float64)       # slots hold the small transient row sets: always float64
        self._fin = weakref.finalize(self, N.load().bc_data_destroy, h)
        return self

    def update(self, z):
        z = _as_f64(np.atleast_2d(z), 'data')
        if z.shape[1] != self.shape[1]:
            raise ValueError('slot holds rows of %d columns, got %d' % (self.shape[1], z.shape[1]))
        N.call('bc_data_upload', self.h, _ptr(z), int(z.shape[0]))
        self.shape = (int(z.shape[0]), self.shape[1])
        self._transient = True      # refilled in place: nothing about these rows may be cached
        return self

    def rows(self, local_idx):
        """Rows by LOCAL index, on the host (m x dz float64, whatever the storage dtype)."""
        idx = np.ascontiguousarray(local_idx, dtype=np.int64).ravel()
        out = np.empty((idx.shape[0], self.shape[1]))
        N.call('bc_data_gather_rows', self.h, _ptr(idx), int(idx.shape[0]), _ptr(out))
        return out

    def take(self, local_idx, out=None, transient=False):
        """Rows by LOCAL index, kept on the device: a DeviceData of shape (m, dz), the same dtype and row_offset 0
        (bc_data_take_rows: words are copied, never converted; repeats allowed; any integer array).  `out`: a DeviceData an
        earlier take() returned (or a slot) of the same context, column count and dtype -- it is refilled, resized and
        returned, and marked transient: nothing may be cached about its rows, the next take(out=) replaces them.
        `transient=True` marks a fresh result the same way (the first fill of a buffer that will be refilled)."""
        out_given = out is not None
        idx = np.asarray(local_idx)
        if idx.size and not np.issubdtype(idx.dtype, np.integer):
            raise TypeError('take() wants integer row numbers, got %s' % idx.dtype)
        idx = np.ascontiguousarray(idx, dtype=np.int64).ravel()
        if out is not None and not isinstance(out, DeviceData):
            raise TypeError('take(out=...) wants a DeviceData')
        h = C.c_void_p(out.h.value) if out is not None else C.c_void_p()
        try:
            N.call('bc_data_take_rows', self.h, _ptr(idx), int(idx.shape[0]), C.byref(h))
        except RuntimeError:                # a HIP failure (not a refusal, which leaves `out` as it was): `out` holds 0 rows now
            if out is not None:
                out.shape = (0, out.shape[1])
            raise
        if out is None:
            out = DeviceData._adopt(h, (idx.shape[0], self.shape[1]), self.ctx)
        else:
            out.shape = (int(idx.shape[0]), self.shape[1])
            out.row_offset = 0
        out._transient = transient or out_given
        return out

    def encode(self, enc, pass_cols=1, dtype=np.float32, out=None, transient=False):
        """These rows `[x, pass-through]` through a device feature encoder (encoders.MLPEncoder), kept on the device: a
        DeviceData of shape (n, enc.widths[-1] + pass_cols) and storage `dtype` (bc_data_encode: float64 arithmetic; float32
        storage rounds each feature once; the last `pass_cols` columns -- the neural-linear model's y -- are carried over).
        The row_offset is kept.  `out` / `transient`: as in take() -- an earlier result (or a slot) of the same context, width
        and dtype is refilled, resized, returned and marked transient."""
        dt = np.dtype(dtype)
        if dt not in (np.float64, np.float32):
            raise ValueError('DeviceData stores float64 or float32 rows, not %s' % dt)
        if out is not None and not isinstance(out, DeviceData):
            raise TypeError('encode(out=...) wants a DeviceData')
        out_given = out is not None
        h = C.c_void_p(out.h.value) if out is not None else C.c_void_p()
        try:
            N.call('bc_data_encode', enc.h, self.h, int(pass_cols), int(dt.itemsize), C.byref(h))
        except RuntimeError:                # a HIP failure (not a refusal, which leaves `out` as it was): `out` holds 0 rows now
            if out is not None:
                out.shape = (0, out.shape[1])
            raise
        enc.launches += 1
        shape = (self.shape[0], enc.widths[-1] + int(pass_cols))
        if out is None:
            out = DeviceData._adopt(h, shape, self.ctx)
        else:
            out.shape = shape
        out.row_offset = self.row_offset
        out._transient = transient or out_given
        return out

    def __getitem__(self, idx):
        if isinstance(idx, tuple) and len(idx) == 2 and idx[1] == slice(None):      # data[rows, :], as the grouped selection writes it
            idx = idx[0]
        if isinstance(idx, (int, np.integer)):
            return self.rows([idx])[0]
        return self.rows(idx)

    def __len__(self):
        return self.shape[0]

    @classmethod
    def from_torch(cls, t, ctx=None, row_offset=0):
        """Borrow a contiguous float64 or float32 CUDA tensor (kept alive by this object; a float32 tensor is borrowed as
        float32 rows, see DeviceData).

        The tensor's producer kernels run on torch's current stream; unless this library launches on
        that same stream (Context(stream=...)), wait for them here -- otherwise our first kernel could
        read rows torch has not finished writing."""
        assert t.is_cuda and t.is_contiguous() and str(t.dtype) in ('torch.float64', 'torch.float32') and t.dim() == 2
        dt = np.float32 if str(t.dtype) == 'torch.float32' else np.float64
        import torch
        cur = torch.cuda.current_stream(t.device)
        c = ctx or default_context()
        if c.stream_handle is None or c.stream_handle != cur.cuda_stream:
            cur.synchronize()
        return cls(ctx=ctx, device_ptr=t.data_ptr(), shape=tuple(t.shape), keepalive=t, row_offset=row_offset, dtype=dt)


def upload_slot(slots, dz, ctx):
    """The DeviceData.slot for small transient row sets of `dz` columns on `ctx`, kept in the owner's map `slots` and created
    on first use.  (One map per owner: two owners sharing a slot would overwrite each other's rows between their calls.)"""
    slot = slots.get(dz)
    if slot is None:
        slot = slots[dz] = DeviceData.slot(dz, cap_rows=256, ctx=ctx)
    return slot


class _PhiT:
    """`vecs.T`: the S x N view handed to the solvers as A (hilbert.py:17)."""

    def __init__(self, phi):
        self.phi = phi
        self.shape = (phi.shape[1], phi.shape[0])
        self.size = phi.shape[0] * phi.shape[1]

    @property
    def T(self):
        return self.phi

    def __array__(self, dtype=None, copy=None):
        return np.asarray(self.phi).T


class DevicePhi:
    """N x S matrix of row-centred (beta-)log-likelihoods in the tiled HBM layout."""

    def __init__(self, handle, ctx, owner=True, release=None):
        self.h = handle
        self.ctx = ctx
        self.refresh()
        if release is not None:
            self._fin = weakref.finalize(self, release, handle)      # hand the buffers back to a pool
        else:
            self._fin = weakref.finalize(self, N.load().bc_phi_destroy, handle) if owner else None

    def refresh(self):
        n, s, off = C.c_int64(), C.c_int32(), C.c_int64()
        N.call('bc_phi_shape', self.h, C.byref(n), C.byref(s), C.byref(off))
        self.shape = (n.value, s.value)
        self.row_offset = off.value
        self.size = n.value * s.value

    # -- construction
    @classmethod
    def from_host(cls, phi, ctx=None, row_offset=0):
        ctx = ctx or default_context()
        phi = np.atleast_2d(phi)
        phi = _as_f64(phi, 'Phi')
        h = C.c_void_p()
        N.call('bc_phi_from_host', ctx.h, _ptr(phi), int(phi.shape[0]), int(phi.shape[1]), int(row_offset), C.byref(h))
        return cls(h, ctx)

    # -- ndarray-like surface
    @property
    def T(self):
        return _PhiT(self)

    def sum(self, axis=None):
        if axis != 0:
            raise NotImplementedError('DevicePhi.sum supports axis=0 only (b = Phi^T 1)')
        return self.colsum()

    def __array__(self, dtype=None, copy=None):
        return self.to_host()

    def __len__(self):
        return self.shape[0]

    # -- device queries
    def colsum(self):
        out = np.empty(self.shape[1])
        N.call('bc_phi_colsum', self.h, _ptr(out))
        return out

    def colsum_all(self, native_comm):
        """Column sums over ALL ranks' shards, added in rank order on the device (bc_phi_colsum_all)."""
        out = np.empty(self.shape[1])
        N.call('bc_phi_colsum_all', self.h, native_comm, _ptr(out))
        return out

    def norms(self):
        out = np.empty(self.shape[0])
        N.call('bc_phi_norms', self.h, _ptr(out))
        return out

    def norm_stats(self):
        z, s = C.c_int64(), C.c_double()
        N.call('bc_phi_norm_stats', self.h, C.byref(z), C.byref(s))
        return z.value, s.value

    def to_host(self):
        out = np.empty(self.shape)
        N.call('bc_phi_to_host', self.h, _ptr(out))
        return out

    def rows(self, local_idx):
        idx = np.ascontiguousarray(local_idx, dtype=np.int64).ravel()
        out = np.empty((idx.shape[0], self.shape[1]))
        N.call('bc_phi_gather_rows', self.h, _ptr(idx), int(idx.shape[0]), _ptr(out))
        return out

    def group_sum(self, groups):
        """DevicePhi whose row g is the sum of this matrix's rows groups[g] (local indices), accumulated in the
        order given -- `np.array([vecs[g].sum(axis=0) for g in groups])` without leaving the device
        (grouped selection, bcores.py:46-50, 56-61)."""
        sizes = [len(g) for g in groups]
        offsets = np.zeros(len(groups) + 1, dtype=np.int64)
        np.cumsum(sizes, out=offsets[1:])
        members = (np.concatenate([np.asarray(g, dtype=np.int64).ravel() for g in groups]) if offsets[-1] > 0
                   else np.zeros(0, dtype=np.int64))
        members = np.ascontiguousarray(members, dtype=np.int64)
        h = C.c_void_p()
        N.call('bc_phi_group_sum', self.h, _ptr(members) if members.size else None, _ptr(offsets), len(groups), C.byref(h))
        return DevicePhi(h, self.ctx)

    def matvec(self, v):
        v = _as_f64(v, 'v')
        out = np.empty(self.shape[0])
        N.call('bc_phi_matvec', self.h, _ptr(v), _ptr(out))
        return out

    def argmax(self, v, mode, post_div=1.0):
        """One fused K3 sweep. mode 0: v = (S,2) [cdir, xw] -> GIGA score; mode 1: v = (S,) -> Phi.v/norm/post_div.
        Returns (global row index or -1, score)."""
        v = _as_f64(v, 'v')
        best, score = C.c_int64(), C.c_double()
        N.call('bc_phi_argmax', self.h, int(mode), _ptr(v), float(post_div), C.byref(best), C.byref(score))
        return best.value, score.value
