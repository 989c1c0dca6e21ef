"""coreset/residency.py without a GPU and without the native library: the identity-keyed weak map, the read-only guard of
pinned arrays, the Phi buffer pool (against a counting fake of bc_phi_create / bc_phi_destroy) and keep_resident (against a
stub projector that records pin / unpin)."""
import gc
import warnings

import numpy as np
import pytest

from beta_cores_amd import _native, device
from beta_cores_amd.coreset import residency as R


# ------------------------------------------------------------------ WeakIdMap
def test_weak_map_drops_dead_keys_and_trusts_identity_only():
    m = R.WeakIdMap()
    a, b = np.zeros((3, 2)), np.zeros((3, 2))
    assert m.put(a, 'A') == 'A' and m.get(a) == 'A' and len(m) == 1 and list(m) == ['A']
    assert m.get(b) is None and m.get(b, 7) == 7 and m.pop(b) is None      # same shape, same contents: another object
    m.put(b, 'B')
    assert len(m) == 2 and sorted(m) == ['A', 'B']
    del a
    gc.collect()
    assert len(m) == 1 and list(m) == ['B']
    assert m.pop(b) == 'B' and len(m) == 0 and m.get(b) is None
    m.put(b, 'B')
    m.clear()
    assert len(m) == 0


def test_weak_map_late_callback_of_an_earlier_entry_leaves_the_slot_alone():
    """ids are recycled: the death callback of an object that once sat under this id must not remove its successor's entry."""
    m = R.WeakIdMap()
    a = np.zeros(4)
    m.put(a, 'old')
    old_ref = m._d[id(a)][0]
    m.put(a, 'new')                      # the slot now holds another entry under the same id
    old_ref.__callback__(old_ref)        # ... and the earlier entry's callback fires late
    assert m.get(a) == 'new' and len(m) == 1
    new_ref = m._d[id(a)][0]
    new_ref.__callback__(new_ref)        # the slot's own callback does remove it
    assert len(m) == 0


def test_weak_map_policies_for_keys_without_weak_references():
    key = [1, 2, 3]                      # a list cannot be weakly referenced
    m = R.WeakIdMap()
    assert m.put(key, 'v') == 'v' and m.get(key) is None and len(m) == 0
    s = R.WeakIdMap(strong=True)
    s.put(key, 'v')
    assert s.get(key) == 'v' and s.get([1, 2, 3]) is None and len(s) == 1
    assert s.pop(key) == 'v' and len(s) == 0


# ------------------------------------------------------------------ the guard
class Owner:
    pass


def test_guard_counts_pins_over_owners():
    a = np.zeros((2, 3))
    o1, o2 = Owner(), Owner()
    p1 = R.Pin(o1, a, 'dd1')
    assert not a.flags.writeable and (p1.data, p1.count) == ('dd1', 1)
    with pytest.raises(ValueError):
        a[0, 0] = 1.
    p2 = R.Pin(o2, a, 'dd2')
    assert p2.guard is p1.guard and p1.guard.count == 2
    p1.drop()
    assert not a.flags.writeable
    del o2                               # a dying owner lets go of its pin
    gc.collect()
    assert a.flags.writeable and len(R._pin_guard) == 0


def test_guard_keeps_an_array_read_only_that_was_so_before():
    a = np.zeros((2, 3))
    a.flags.writeable = False
    owner = Owner()
    R.Pin(owner, a, None).drop()
    assert not a.flags.writeable and len(R._pin_guard) == 0


def test_guard_of_a_dead_array_releases_to_nothing():
    a = np.zeros((2, 3))
    g = R._guard_acquire(a)
    del a
    gc.collect()
    assert len(R._pin_guard) == 0
    R._guard_release(g)
    assert len(R._pin_guard) == 0


# ------------------------------------------------------------------ the pool
class FakeNative:
    """Stands in for _native.call / _native.load: hands out numbered Phi handles and counts what is destroyed."""

    def __init__(self):
        self.created, self.destroyed = [], []

    def call(self, name, *args):
        if name == 'bc_phi_create':
            args[-1]._obj.value = len(self.created) + 1
            self.created.append((args[-1]._obj.value, args[1], args[2]))      # (handle, capacity, S)

    def load(self):
        return self

    def bc_phi_destroy(self, h):
        self.destroyed.append(h.value)

    def __getattr__(self, name):         # every other export: a no-op
        return lambda *a: 0


class Ctx:
    h = None


@pytest.fixture
def native(monkeypatch):
    fake = FakeNative()
    monkeypatch.setattr(_native, 'call', fake.call)
    monkeypatch.setattr(_native, 'load', fake.load)
    monkeypatch.setattr(device, '_default_ctx', Ctx())
    return fake


def free_handles(pool, s):
    return sorted((cap, h.value) for cap, h in pool.state['free'].get(s, []))


def test_pool_lend_hands_the_buffer_back_when_fill_raises(native):
    pool = R._PhiPool(Ctx())

    def boom(h):
        raise RuntimeError('K1 failed')
    with pytest.raises(RuntimeError, match='K1 failed'):
        pool.lend(10, 4, boom)
    assert free_handles(pool, 4) == [(256, 1)] and native.destroyed == []
    seen = []
    phi = pool.lend(10, 4, lambda h: seen.append(h.value))
    assert seen == [1] and len(native.created) == 1 and free_handles(pool, 4) == []
    del phi
    assert free_handles(pool, 4) == [(256, 1)]
    pool.clear()


def test_pool_best_fit_below_big_rows(native):
    pool = R._PhiPool(Ctx())
    small, large = pool.lend(10, 4, lambda h: None), pool.lend(1000, 4, lambda h: None)
    del large, small
    assert free_handles(pool, 4) == [(256, 1), (1024, 2)]
    got = []
    phi = pool.lend(200, 4, lambda h: got.append(h.value))          # the smallest buffer that holds 200 rows
    assert got == [1] and free_handles(pool, 4) == [(1024, 2)]
    other = pool.lend(300, 4, lambda h: got.append(h.value))        # 1024 >= 300: re-used although four times too large
    assert got == [1, 2] and len(native.created) == 2
    wide = pool.lend(10, 5, lambda h: got.append(h.value))          # another S: a list of its own
    assert got == [1, 2, 3]
    del phi, other, wide
    pool.clear()


def test_pool_keeps_one_spare_large_buffer_per_s(native):
    pool = R._PhiPool(Ctx())
    n = R._BIG_ROWS
    a, b = pool.lend(n, 4, lambda h: None), pool.lend(n + 1, 4, lambda h: None)
    assert [c[1] for c in native.created] == [n, n + _native.TILE_ROWS]      # whole tiles, no power-of-two slack
    del a
    assert free_handles(pool, 4) == [(n, 1)] and native.destroyed == []
    del b
    assert free_handles(pool, 4) == [(n, 1)] and native.destroyed == [2]
    c = pool.lend(3 * n, 4, lambda h: None)                                 # the spare one is too small: a new buffer
    assert len(native.created) == 3
    del c
    assert native.destroyed == [2, 3]
    pool.clear()


def test_pool_handle_released_after_the_pool_died_is_destroyed(native):
    pool = R._PhiPool(Ctx())
    phi, spare = pool.lend(10, 4, lambda h: None), pool.lend(10, 4, lambda h: None)
    del spare
    state = pool.state
    del pool
    gc.collect()
    assert native.destroyed == [2] and state['free'] == {}      # the free one went with the pool, the lent one is still valid
    del phi
    assert native.destroyed == [2, 1] and not any(state['free'].values())


def test_pool_clear_and_finalizer_destroy_each_free_handle_once(native):
    pool = R._PhiPool(Ctx())
    held = [pool.lend(10, 4, lambda h: None), pool.lend(600, 4, lambda h: None), pool.lend(10, 7, lambda h: None)]
    del held
    pool.clear()
    assert sorted(native.destroyed) == [1, 2, 3] and not any(pool.state['free'].values())
    phi = pool.lend(10, 4, lambda h: None)                       # the pool goes on working after clear()
    del phi
    assert free_handles(pool, 4) == [(256, 4)]
    del pool
    gc.collect()
    assert sorted(native.destroyed) == [1, 2, 3, 4]


# ------------------------------------------------------------------ keep_resident
class StubProjector:
    ctx = None

    def __init__(self):
        self.calls = []

    def pin(self, a):
        self.calls.append(('pin', id(a)))
        return 'device copy'

    def unpin(self, a):
        self.calls.append(('unpin', id(a)))


class StubCoreset:
    def __init__(self, data, prj, wanted=True):
        self.resident = R.keep_resident(self, data, prj, wanted)


def test_keep_resident_pins_from_small_rows_on_and_unpins_with_the_owner():
    prj = StubProjector()
    Z = np.zeros((R._SMALL_ROWS, 2))
    alg = StubCoreset(Z, prj)
    assert alg.resident == 'device copy' and prj.calls == [('pin', id(Z))]
    del alg
    gc.collect()
    assert prj.calls == [('pin', id(Z)), ('unpin', id(Z))]
    prj.calls.clear()
    assert StubCoreset(Z[:-1].copy(), prj).resident is None                 # one row short
    assert StubCoreset(Z, prj, wanted=False).resident is None
    assert StubCoreset(Z.ravel(), prj).resident is None and StubCoreset(Z.tolist(), prj).resident is None
    assert prj.calls == []


def test_keep_resident_leaves_projectors_without_pin_alone():
    assert StubCoreset(np.zeros((R._SMALL_ROWS, 2)), object()).resident is None


def test_keep_resident_copies_a_view_once_and_warns_at_the_callers_line(native):
    prj = StubProjector()
    base = np.zeros((R._SMALL_ROWS + 1, 2), dtype=np.float32)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        alg = StubCoreset(base[:-1], prj)
    assert [(w.category, w.filename) for w in caught] == [(UserWarning, __file__)]
    assert 'view' in str(caught[0].message) and '%d rows' % R._SMALL_ROWS in str(caught[0].message)
    assert isinstance(alg.resident, device.DeviceData) and alg.resident.shape == (R._SMALL_ROWS, 2)
    assert alg.resident.dtype == np.float32 and prj.calls == [] and base.flags.writeable
    del alg
