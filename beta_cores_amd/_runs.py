"""What the chunked device runs and the packed batches of small problems share in the Python layer: the draw-ahead loop over a
run's chunks, the draws of a chunk of steps, a unit's device clock, the packing into rows | w | row_ptr (natively: csrc/bc_run.h,
csrc/bc_batch.h)."""
import ctypes as C
import time

import numpy as np

from . import _native as N


def run_chunks(total, chunk, draw, chunk_begin, chunk_end, close, finish=None, on_chunk=None):
    """The chunks of a run that has been begun.  `draw(k)` makes the next k steps' random numbers; `chunk_begin(drawn)` enqueues
    them and returns how many steps they were; `chunk_end()` waits and returns the native status.  Chunk i + 1 is drawn between
    `chunk_begin` and `chunk_end` of chunk i -- beside the GPU -- and nothing past step `total`; a pending chunk is always ended.
    `on_chunk(done)`: after every chunk that ended well.  `finish()`: the run's _end with its outputs.  Any exception calls
    `close()` -- the run's _end without outputs, a no-op status where the run is closed already -- and goes on."""
    total, chunk = int(total), int(chunk)
    try:
        done = 0
        nxt = draw(min(chunk, total))
        while done < total:
            done += int(chunk_begin(nxt))
            try:
                nxt = draw(min(chunk, total - done)) if done < total else None      # beside the GPU
            finally:
                status = chunk_end()
            N.check(status)
            if on_chunk is not None:
                on_chunk(done)
        return finish() if finish is not None else None
    except BaseException:
        close()
        raise


def step_draws(sampler, S, D, n_total, n_sub, seconds=None):
    """`draw(k)` of k steps in the host loop's order, step by step: the sampler's S x D normals (`_normals`), then
    `np.random.randint(n_total, size=n_sub)` (`n_sub = 0`: none drawn, None returned).  `seconds[0]` += the time spent drawing."""
    def draw(k):
        t0 = time.perf_counter()
        E = np.empty((k, S, D))
        idx = np.empty((k, n_sub), dtype=np.int64) if n_sub else None
        for t in range(k):
            E[t] = sampler._normals(S, D)
            if n_sub:
                idx[t] = np.random.randint(n_total, size=n_sub)
        if seconds is not None:
            seconds[0] += time.perf_counter() - t0
        return E, idx
    return draw


def device_ms(entry, ctx):
    """GPU milliseconds of a unit's last run on `ctx`, from its `entry` (bc_*_device_ms)."""
    ms = C.c_double()
    N.call(entry, ctx.h, C.byref(ms))
    return ms.value


def pack_problems(pairs, width=0):
    """[(rows n_p x D, weights n_p)] -> (rows, w, row_ptr): float64, C-contiguous, int64 row_ptr; `width`: D of an empty list.
    (No per-problem conversions: the batched Laplace fit of 101 tiny problems takes under a millisecond, packing included.)"""
    row_ptr = np.concatenate(([0], np.cumsum([z.shape[0] for z, _ in pairs]))).astype(np.int64)
    rows = np.ascontiguousarray(np.concatenate([z for z, _ in pairs], axis=0) if pairs else np.zeros((0, width)), dtype=np.float64)
    w = np.ascontiguousarray(np.concatenate([w for _, w in pairs]) if pairs else np.zeros(0), dtype=np.float64)
    return rows, w, row_ptr
