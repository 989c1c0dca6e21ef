"""The draw-ahead loop over a chunked run's chunks (beta_cores_amd/_runs.py), driven through psvi_many_run with a stand-in for
the native library: what is called in which order, what an exception leaves behind, and the packing of problems."""
import numpy as np
import pytest

from beta_cores_amd import _native, _runs
from beta_cores_amd.coreset import bpsvi

D, S, N_SUB, ROWS = 3, 2, 4, 10


class FakeNative:
    """Stands in for _native.call / _native.load: records every entry point of the run in `events`."""

    def __init__(self):
        self.events, self.chunk_end_status = [], []

    def call(self, name, *args):
        if name == 'bc_psvi_many_chunk_begin':
            self.events.append(('chunk_begin', int(args[-1])))
        elif name == 'bc_psvi_many_end':
            self.events.append(('end', 'fetch'))
        else:
            self.events.append((name,))

    def load(self):
        return self

    def bc_psvi_many_chunk_end(self, h, marked):
        self.events.append(('chunk_end',))
        return self.chunk_end_status.pop(0) if self.chunk_end_status else 0

    def bc_psvi_many_end(self, h, *outs):
        self.events.append(('end', 'close'))
        return 0

    def bc_last_error(self):
        return b'the stand-in refused'

    def __getattr__(self, name):         # every other export: a no-op
        return lambda *a: 0


class Data:
    shape, h = (ROWS, D), None

    class ctx:
        h = None


@pytest.fixture
def native(monkeypatch):
    fake = FakeNative()
    monkeypatch.setattr(_native, 'call', fake.call)
    monkeypatch.setattr(_native, 'load', fake.load)
    return fake


def run(native, itrs, chunk, fail_draw_at=None, on_chunk=None):
    def draw(k):
        native.events.append(('draw', k))
        if fail_draw_at is not None and sum(1 for e in native.events if e[0] == 'draw') == fail_draw_at:
            raise KeyError('the draw failed')
        return np.zeros((k, S, D)), np.zeros((k, N_SUB), dtype=np.int64)
    return bpsvi.psvi_many_run(Data(), [np.zeros((1, D)), np.zeros((2, D))], [np.ones(1), np.ones(2)], S, itrs, np.ones((2, itrs)), draw, N_SUB,
                               chunk_steps=chunk, on_chunk=on_chunk)


def test_the_next_chunk_is_drawn_beside_the_device_and_never_past_the_last_step(native):
    seen = []
    res = run(native, 5, 2, on_chunk=seen.append)
    assert native.events == [('bc_psvi_many_begin',), ('draw', 2), ('chunk_begin', 2), ('draw', 2), ('chunk_end',), ('chunk_begin', 2),
                             ('draw', 1), ('chunk_end',), ('chunk_begin', 1), ('chunk_end',), ('end', 'fetch'), ('bc_psvi_many_device_ms',)]
    assert seen == [2, 4, 5] and sum(e[1] for e in native.events if e[0] == 'draw') == 5 and res['marked'] == []


def test_one_chunk_draws_once(native):
    run(native, 3, 8)
    assert native.events[1:-2] == [('draw', 3), ('chunk_begin', 3), ('chunk_end',)]


def test_an_exception_from_draw_ends_the_pending_chunk_then_closes_the_run(native):
    with pytest.raises(KeyError, match='the draw failed'):
        run(native, 5, 2, fail_draw_at=2)
    assert native.events == [('bc_psvi_many_begin',), ('draw', 2), ('chunk_begin', 2), ('draw', 2), ('chunk_end',), ('end', 'close')]


def test_an_exception_from_the_first_draw_closes_the_run(native):
    with pytest.raises(KeyError):
        run(native, 5, 2, fail_draw_at=1)
    assert native.events == [('bc_psvi_many_begin',), ('draw', 2), ('end', 'close')]


@pytest.mark.parametrize('status,error', [(_native.BC_INVALID_ARGUMENT, ValueError), (_native.BC_NUMERICAL_PRECISION, _native.NumericalPrecisionError),
                                          (7, RuntimeError)])
def test_a_failing_chunk_end_closes_the_run_and_raises(native, status, error):
    native.chunk_end_status = [0, status]
    seen = []
    with pytest.raises(error, match='the stand-in refused'):
        run(native, 6, 2, on_chunk=seen.append)
    assert native.events[-4:] == [('chunk_begin', 2), ('draw', 2), ('chunk_end',), ('end', 'close')] and seen == [2]


def test_step_draws_keep_the_host_loops_order_of_random_numbers():
    class Sampler:
        def __init__(self):
            self.rng = np.random.RandomState(3)

        def _normals(self, s, d):
            return self.rng.randn(s, d)
    np.random.seed(5)
    seconds = [0.]
    E, idx = _runs.step_draws(Sampler(), S, D, ROWS, N_SUB, seconds=seconds)(3)
    rng = np.random.RandomState(3)
    np.random.seed(5)
    for t in range(3):
        assert np.array_equal(E[t], rng.randn(S, D)) and np.array_equal(idx[t], np.random.randint(ROWS, size=N_SUB))
    assert idx.dtype == np.int64 and seconds[0] > 0.
    state = np.random.get_state()[1].copy()
    E, idx = _runs.step_draws(Sampler(), S, D, ROWS, 0)(2)
    assert idx is None and E.shape == (2, S, D) and np.array_equal(np.random.get_state()[1], state)      # n_sub = 0 draws no row numbers


def test_pack_problems():
    rows, w, row_ptr = _runs.pack_problems([(np.ones((1, D)), np.ones(1)), (np.full((2, D), 2, dtype=np.float32), np.array([3, 4]))])
    assert rows.dtype == w.dtype == np.float64 and row_ptr.dtype == np.int64 and rows.flags.c_contiguous
    assert row_ptr.tolist() == [0, 1, 3] and w.tolist() == [1., 3., 4.] and rows[:, 0].tolist() == [1., 2., 2.]
    rows, w, row_ptr = _runs.pack_problems([], width=D)
    assert rows.shape == (0, D) and w.shape == (0,) and row_ptr.tolist() == [0]
