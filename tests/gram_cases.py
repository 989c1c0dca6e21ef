"""Inputs, reference, bound and shapes for the tests of K4, the weighted Gram (beta_cores_amd/csrc/bc_gram.hip); no test in here.
tests/test_gram_cases_cpu.py holds the lists against the split arithmetic of csrc/bc_gram_plan.h (compiled for the host) and the
bound against NumPy and four mutants; tests/test_gpu_gram.py runs them on the device.

THE BOUND.  An element of G = X^T diag(w) X is a sum of n terms w_i x_ia x_ib.  Computing it in float64 costs one rounding for
w_i * x_ia, one for each product (none where the product is fused into the addition) and n - 1 for the additions, in WHATEVER
order they are associated: every term passes through at most 1 + 1 + (n - 1) = n + 1 roundings of relative size u = 2^-53 on
its way into the sum, so

    |G - Gr|  <=  ((1 + u)^(n + 1) - 1) * SG,      SG = |X|^T diag(|w|) |X|

whether the sum is an fma chain over the rows (k_gram_small), 4-row MFMA k-steps into an accumulator (k_gram, k_gram_dma) or
those followed by sums over row splits (k_gram_reduce1 / 2) -- a split sum only re-associates the n - 1 additions.  The
reference below is computed in np.longdouble (64-bit mantissa, u' = 2^-64) in chunks of 1024 rows, so its own error is at most
(2 + 1023 + n / 1024) * 2^-64 * SG: under one unit of u * SG up to a million rows.  One more unit covers the second-order
terms of (1 + u)^(n + 1) (n^2 u^2 / 2 < u up to n = 1e8).  Hence (n + 3) * 2^-53 * SG, plus 1e-300 so that 0 <= 0 holds where
SG is 0.  X^T (w * y) likewise with Sv = |X|^T (|w| * |y|).  Derived, not tuned: a result outside it is a finding.
"""
import functools

import numpy as np

U = 2.0 ** -53
LONGDOUBLE_OK = bool(np.finfo(np.longdouble).eps <= 2.0 ** -63)
LONGDOUBLE_WHY = ('np.longdouble has eps = %g > 2^-63 on this platform: no reference more precise than float64 to hold K4 against'
                  % float(np.finfo(np.longdouble).eps))

KINDS = ('plain', 'wide')


# ------------------------------------------------------------------ inputs
def inputs(n, dz, kind):
    """(Z [n x dz float64], w [n]) seeded by (n, dz, kind).  'plain': standard normal.  'wide': the same, rows scaled by
    10^[-6 .. 6] and columns by 10^[-3 .. 3] (|w x x| stays within 1e-22 .. 1e23: nothing under- or overflows), so that small
    entries sit next to large ones.  w in [0, 2) with a quarter of the rows at exactly 0; the LAST row's weight is positive, so
    that a kernel which drops or repeats the last row is seen by the weighted cases too."""
    assert kind in KINDS
    rng = np.random.RandomState((1000003 * n + 101 * dz + KINDS.index(kind)) % (2 ** 31))
    Z = rng.randn(n, dz)
    if kind == 'wide':
        Z *= 10.0 ** rng.uniform(-6., 6., size=(n, 1))
        Z *= 10.0 ** rng.uniform(-3., 3., size=(1, dz))
    w = rng.rand(n) * 2.
    if n > 1:
        w[rng.permutation(n - 1)[:n // 4]] = 0.
    w[-1] = 0.5 + w[-1] / 2.
    return Z, w


# ------------------------------------------------------------------ reference and bound
CHUNK = 1024


def _ld_tdot(A, B):
    """A^T B in np.longdouble, the rows summed in chunks of CHUNK (keeps the reference's own error under one unit of 2^-53)"""
    out = np.zeros((A.shape[1],) + B.shape[1:], dtype=np.longdouble)
    for i in range(0, A.shape[0], CHUNK):
        out += A[i:i + CHUNK].T.dot(B[i:i + CHUNK])
    return out


def reference(Z, w):
    """(Gr, vr, SG, Sv) in np.longdouble; w = None: all ones.  NaN / inf propagate as they do in NumPy."""
    assert LONGDOUBLE_OK, LONGDOUBLE_WHY
    X = Z[:, :-1].astype(np.longdouble)
    y = Z[:, -1].astype(np.longdouble)
    wl = np.ones(Z.shape[0], dtype=np.longdouble) if w is None else np.asarray(w).astype(np.longdouble)
    WX = wl[:, None] * X                                  # (one rounding of 2^-64: counted in the module docstring)
    with np.errstate(invalid='ignore'):
        Gr, vr = _ld_tdot(WX, X), _ld_tdot(WX, y)
        SG, Sv = _ld_tdot(np.abs(WX), np.abs(X)), _ld_tdot(np.abs(WX), np.abs(y))
    return Gr, vr, SG, Sv


@functools.lru_cache(maxsize=32)
def case(n, dz, kind, weighted):
    """(Z, w or None, (Gr, vr, SG, Sv)) of a listed case: shared by the checks of one test, read-only."""
    Z, w = inputs(n, dz, kind)
    w = w if weighted else None
    ref = reference(Z, w)
    for a in (Z, w) + ref:
        if a is not None:
            a.setflags(write=False)
    return Z, w, ref


def bound(n, S):
    return (n + 3) * np.longdouble(U) * S + np.longdouble(1e-300)


def ratio(G, v, n, ref):
    """Worst |error| / bound over the finite reference entries of G and v (<= 1: inside the bound)."""
    Gr, vr, SG, Sv = ref
    with np.errstate(invalid='ignore'):
        rg = np.abs(G.astype(np.longdouble) - Gr) / bound(n, SG)
        rv = np.abs(v.astype(np.longdouble) - vr) / bound(n, Sv)
    r = np.concatenate((rg[np.isfinite(Gr)].ravel(), rv[np.isfinite(vr)].ravel(), [0.]))
    return float('inf') if np.isnan(r).any() else float(r.max())


# ------------------------------------------------------------------ the split plan of run_gram, restated
SEG = 16          # BC_GRAM_SEG
DMA_MIN_ROWS = 4096
SMALL_ROWS = 512  # BC_GRAM_SMALL_ROWS
HOST_DOUBLES = 60000


def plan(n_rows, ntri, n_cu, slots, waves, kr):
    """(rows_per_split, splits, nruns): bc_gram_plan (csrc/bc_gram_plan.h) restated; held against the header by the CPU test"""
    want = (n_cu * slots * (waves if waves > 0 else 1) + ntri - 1) // ntri
    most = (n_rows + 2 * kr - 1) // (2 * kr)
    splits = max(1, min(want, most))
    rps = (n_rows + splits - 1) // splits
    rps = max(kr, (rps + kr - 1) // kr * kr)
    splits = max(1, (n_rows + rps - 1) // rps)
    return rps, splits, (splits + SEG - 1) // SEG


def route(n, d, weighted, n_cu=256, f32=False, dma_env=1):
    """What run_gram does with n rows [x (d), y]: dict(bt, kr, ntri, dma, rps, splits, nruns, last) -- last = rows of the last
    split.  (While the row count, not the device, limits the splits -- every case here: n <= 2 * kr * n_cu * slots / ntri --
    the plan is the same for every n_cu; the CPU test checks 128 .. 304.)"""
    bt = 128 if d > 64 else 64
    nt = (d + bt - 1) // bt
    ntri = nt * (nt + 1) // 2
    dma = bt == 128 and ntri == 1 and not weighted and d + 1 >= 128 and dma_env != 0 and n >= DMA_MIN_ROWS and not f32
    kr = 16 if dma or bt == 128 else 32
    slots = 4 if dma else (3 if bt == 64 else 2)
    rps, splits, nruns = plan(n, ntri, n_cu, slots, 1 if ntri == 1 else 8, kr)
    return dict(bt=bt, kr=kr, ntri=ntri, dma=dma, slots=slots, waves=1 if ntri == 1 else 8, rps=rps, splits=splits, nruns=nruns,
                last=n - (splits - 1) * rps)


# ------------------------------------------------------------------ the case lists: (n, dz), dz = D + 1
# k_gram_small (n <= 512, host entry): row counts around its 128-row LDS trips; dz around its 16-column blocks (17, 18: the
# second block carries y alone / y and one x column; 33, 65, 101, 116: block pairs ta < tb with x * x entries) and the samplers'
SMALL = [(n, dz) for n in (1, 2, 127, 128, 129, 255, 256, 257, 511, 512) for dz in (2, 3, 16, 17, 18, 33, 65, 101, 116)] \
    + [(200, 244), (245, 243), (1, 244)]
# the host entry past 512 rows: run_gram<64 / 128> on a view of the staging buffer
HOST_BIG = [(513, 2), (513, 9), (513, 65), (600, 65), (880, 66), (900, 65), (513, 101), (590, 100), (3000, 18), (20000, 2)]
# resident rows, fewer than a few slabs: (n, D)
RESIDENT_FEW = [(n, d) for n in (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 129) for d in (1, 5, 63, 64, 65, 127, 128, 129, 200, 257)]
RESIDENT_F32_D = (5, 64, 65, 129)

SPLIT_COUNTS = (1, 2, 7, 8, 9, 15, 16, 17, 33, 129)
SPLIT_D = {64: 8, 128: 65}


def _split_edges():
    """For each tile size and each split count s of SPLIT_COUNTS: the largest n that the plan cuts into s splits (all of them
    full: n is a multiple of rows_per_split) and its n + 1 (one more split, of one row); for s = 2 and 17 also the n whose last
    split is exactly one slab."""
    out = []
    for bt, d in sorted(SPLIT_D.items()):
        for s in SPLIT_COUNTS:
            n = 1
            while route(n + 1, d, True)['splits'] <= s:
                n += 1
            assert route(n, d, True)['splits'] == s
            out += [(n, d), (n + 1, d)]
        for s in (2, 17):
            n = 1
            while not (route(n, d, True)['splits'] == s and route(n, d, True)['last'] == route(n, d, True)['kr']):
                n += 1
            out.append((n, d))
    return out


SPLIT_EDGES = _split_edges()      # (n, D)
