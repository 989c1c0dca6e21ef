"""Keeping rows on the device, in one place for the projectors and the coresets: the identity-keyed weak map behind every
per-array cache (WeakIdMap), the read-only guard and the record of a pinned array (Pin), the pool of Phi buffers, the row-count
thresholds, and the coresets' decisions -- pin or copy (keep_resident), sub-sample on the device or the host (sub_rows)."""
import ctypes as C
import os
import warnings
import weakref

import numpy as np

from .. import _native as N
from ..device import DeviceData, DevicePhi

_SMALL_ROWS = 4096     # below this an input is treated as transient (coreset points, sub-samples)
_PIPE_ROWS = 65536     # live host arrays from this size on are uploaded and projected in one pipelined call
_BIG_ROWS = 65536      # Phi buffers above this are not hoarded: at most one free buffer per S is kept


class WeakIdMap:
    """id(obj) -> value without keeping obj alive.  An entry is trusted only while its weakref still points at the object asked
    about (ids are recycled once an object dies), and an object's death removes the slot only if it still holds that object's
    entry.  `strong`: what happens to objects that cannot be weakly referenced -- held strongly (True) or not stored (False)."""

    def __init__(self, strong=False):
        self._d = {}      # id -> (ref, value)
        self._strong = strong

    def get(self, obj, default=None):
        ent = self._d.get(id(obj))
        return ent[1] if ent is not None and ent[0]() is obj else default

    def put(self, obj, value):
        key = id(obj)

        def gone(ref, d=self._d):
            if key in d and d[key][0] is ref:
                del d[key]
        try:
            ref = weakref.ref(obj, gone)
        except TypeError:
            if not self._strong:
                return value
            ref = lambda: obj
        self._d[key] = (ref, value)
        return value

    def pop(self, obj):
        value = self.get(obj)
        if value is not None:
            del self._d[id(obj)]
        return value

    def clear(self):
        self._d.clear()

    def __len__(self):
        return len(self._d)

    def __iter__(self):
        return iter([ent[1] for ent in self._d.values()])


# ---- host arrays pinned on the device.  While an ndarray is pinned its device copy is what gets projected, so an
# in-place edit of the array would go unseen; the array is therefore made read-only for as long as any pin holds it
# (NumPy then raises on assignment instead of the device silently serving stale rows).
_pin_guard = WeakIdMap(strong=True)      # ndarray -> _Guard, counted over all projectors


class _Guard:
    __slots__ = ('count', 'was_writeable', 'ref')

    def __init__(self, arr):
        self.count, self.was_writeable, self.ref = 0, bool(arr.flags.writeable), weakref.ref(arr)
        try:
            arr.flags.writeable = False
        except ValueError:
            pass


def _guard_acquire(arr):
    """Make `arr` read-only while pinned; returns the guard to hand to _guard_release."""
    g = _pin_guard.get(arr) or _pin_guard.put(arr, _Guard(arr))
    g.count += 1
    return g


def _guard_release(g):
    """Drop one pin of the array this GUARD holds (not whatever array carries the same id() today)."""
    g.count -= 1
    arr = g.ref()
    if g.count <= 0 and arr is not None:
        if g.was_writeable:
            try:
                arr.flags.writeable = True
            except ValueError:
                pass
        _pin_guard.pop(arr)      # (g itself: a guard stays in the map for as long as it counts a pin)


class Pin:
    """One projector's pin of one host array: the device copy, how often it was pinned (pins nest: the copy goes when the last
    holder unpins), the array's read-only guard, and the finalizer through which a dying `owner` lets go of the guard."""
    __slots__ = ('data', 'count', 'guard', 'finalizer')

    def __init__(self, owner, arr, data):
        self.data, self.count, self.guard = data, 1, _guard_acquire(arr)
        self.finalizer = weakref.finalize(owner, _guard_release, self.guard)

    def drop(self):
        self.finalizer.detach()
        _guard_release(self.guard)


def _resident_dtype(arr):
    """Storage dtype of the device copy of a host array: a float32 ndarray of _SMALL_ROWS rows or more stays float32 (results
    are bit-identical to the widened rows', only the upload time and the memory change); everything else is float64 (None)."""
    if isinstance(arr, np.ndarray) and arr.dtype == np.float32 and arr.ndim == 2 and arr.shape[0] >= _SMALL_ROWS:
        return np.float32
    return None


def _destroy_free(state, alive=True):
    """Destroy the buffers nobody holds; `alive=False` (the pool has died): and every buffer that comes back from now on."""
    state['alive'] = alive
    destroy = N.load().bc_phi_destroy
    for lst in state['free'].values():
        for _, h in lst:
            destroy(h)
    state['free'].clear()


class _PhiPool:
    """Phi buffers recycled instead of hipMalloc'ed / hipFree'd per projection.
    A handle is lent to exactly one DevicePhi wrapper; when that wrapper is garbage collected the
    handle comes back -- so two live results never alias: a solver that still holds the Phi of an
    earlier project() keeps its buffer, and the next project() gets another one (the reference
    returns a fresh array per call, projector.py:24).  Handles still on loan when the pool dies
    stay valid and are destroyed by their wrapper."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.state = {'alive': True, 'free': {}}     # shared with the release callbacks
        self._fin = weakref.finalize(self, _destroy_free, self.state, False)

    def acquire(self, n_rows, s):
        lst = self.state['free'].setdefault(s, [])
        best = None
        for i, (cap, h) in enumerate(lst):
            if cap >= n_rows and (best is None or cap < lst[best][0]):
                best = i
        if best is not None and (n_rows < _BIG_ROWS or lst[best][0] <= 2 * n_rows):
            return lst.pop(best)
        if n_rows < _BIG_ROWS:
            cap = max(256, 1 << int(np.ceil(np.log2(max(n_rows, 1)))))
        else:
            cap = ((n_rows + N.TILE_ROWS - 1) // N.TILE_ROWS) * N.TILE_ROWS      # large shards: no power-of-two slack
        h = C.c_void_p()
        N.call('bc_phi_create', self.ctx.h, int(cap), int(s), C.byref(h))
        return cap, h

    def releaser(self, cap, s):
        state = self.state      # (not the pool: a handle may come back after the pool has died)

        def release(handle):
            lst = state['free'].setdefault(s, [])
            # one spare large buffer per S is enough for a gradient loop
            if not state['alive'] or (cap >= _BIG_ROWS and any(c >= _BIG_ROWS for c, _ in lst)):
                N.load().bc_phi_destroy(handle)
            else:
                lst.append((cap, handle))
        return release

    def lend(self, n_rows, s, fill):
        """A buffer for n_rows x s that `fill(handle)` has written, as a DevicePhi that hands it back when it dies; a `fill`
        that raises hands it back at once."""
        cap, h = self.acquire(n_rows, s)
        release = self.releaser(cap, s)
        try:
            fill(h)
        except Exception:
            release(h)
            raise
        return DevicePhi(h, self.ctx, release=release)

    def clear(self):
        _destroy_free(self.state)


# ---- the coresets' side: which data sets stay in HBM, and how their rows are sub-sampled
def is_sharded(comm):
    """BC_FORCE_EXCHANGE=1 keeps a 1-rank group on the collective paths (rehearsal of the RCCL code on one GPU)."""
    return comm is not None and (comm.world > 1 or os.environ.get('BC_FORCE_EXCHANGE') == '1')


def resident_copy_of_view(data, ll_projector, stacklevel=3):
    """A VIEW (Z[:n], a reshaped or memory-mapped array: `data.base is not None`) cannot be guarded against in-place edits
    the way a pinned array is -- writes through its base would go unseen -- so it is not pinned.  Left at that, every
    full-data gradient would upload all N x Dz rows again (~10 GB per gradient at the headline size).  Instead the rows are
    copied to the device ONCE into a DeviceData this coreset owns, and the caller is told: later edits of the host array
    are not seen (pin_data=False keeps the reference's read-the-live-array-every-time behaviour, bcores.py:44)."""
    warnings.warn('data is a view of another array: its %d rows were copied to the GPU once for this coreset; in-place edits of '
                  'the host array after construction are not seen (pass pin_data=False to re-read it on every projection)'
                  % data.shape[0], UserWarning, stacklevel=stacklevel)
    f32 = data.dtype == np.float32             # float32 rows stay float32 on the device (bit-identical results, half the bytes)
    return DeviceData(np.ascontiguousarray(data, dtype=np.float32 if f32 else np.float64), ctx=getattr(ll_projector, 'ctx', None),
                      dtype=np.float32 if f32 else None)


def pin_for(owner, data, ll_projector):
    """Pin `data` on the projector for as long as `owner` lives (nests on a pin the caller already holds)."""
    dd = ll_projector.pin(data)
    owner._unpin = weakref.finalize(owner, ll_projector.unpin, data)
    return dd


def keep_resident(owner, data, ll_projector, wanted):
    """The device copy a coreset that re-projects ALL rows of `data` per gradient (`wanted`) keeps instead of uploading them
    every time, or None.  An owning ndarray is pinned -- read-only on the host while `owner` lives, so an in-place edit
    raises instead of going unseen --, a view is copied once with a warning (resident_copy_of_view); small or non-ndarray
    data and projectors without pin() are left alone."""
    if not (wanted and hasattr(ll_projector, 'pin') and isinstance(data, np.ndarray) and data.ndim == 2
            and data.shape[0] >= _SMALL_ROWS):
        return None
    if data.base is not None:
        return resident_copy_of_view(data, ll_projector, stacklevel=4)      # (the line that constructs the coreset)
    return pin_for(owner, data, ll_projector)


def sub_rows(rows, idx, ll_projector, out=None, transient=True, host=None):
    """rows[idx] as the input of a projection.  Resident rows that go to a device projector are gathered on the device (the
    same rows and row count, hence the same K1 and the same bits as the host detour) -- `out`, `transient`: as in
    DeviceData.take, a caller that sub-samples per gradient hands its last result back --; anything else is indexed on the
    host, in `host` where the caller's own array is not `rows`."""
    from .projector import is_device_projector      # (projector.py imports this module)
    if isinstance(rows, DeviceData) and is_device_projector(ll_projector):
        return rows.take(idx, out=out, transient=transient)
    return (rows if host is None else host)[idx]
