"""Inputs, reference, bound and case lists for the tests of K3, the fused score + argmax sweep (beta_cores_amd/csrc/bc_sweep_dev.h,
bc_sweep.hip) and the two strided reducers of its per-block candidates (k_local_winner, 256 threads, and dev_pick_blocks in the
fused finish kernels, 512; the step-wise select() runs k_local_winner and k_pick reads its one record); no test in here.
tests/test_sweep_cases_cpu.py holds the lists against the grid arithmetic of csrc/bc_sweep_plan.h (compiled for the host), the
planted problems against np.longdouble, and a NumPy model of the sweep's structure against nine mutants;
tests/test_gpu_sweep.py runs the cases on the device.

THE PLANTED PROBLEM.  Background rows scale * (g + a cdir + b xw), g a unit vector orthogonal to the sweep vectors, a in
[-1, 0.5]: their exact score is a / sqrt(1 + a^2) <= 0.4473 in both modes.  The winner 3.7 cdir scores 1, the largest value the
formula takes; runners-up 0.2 (0.999 cdir + sqrt(1 - 0.999^2) g) score 0.999 and sit where an indexing error would land (the
other half of the lane's double2, the neighbouring lane, the same lane of the next tile, row 0, row n - 1): a sweep that loses
the winner returns one of them.

THE VALUE BOUND.  u = 2^-53.  For a row x with device norm nr and a sweep vector v the kernel computes
    a^ = fma chain of the S terms x_k v_k          |a^ - a|  <= gamma_S T,   T = sum |x_k v_k|,  gamma_S = S u / (1 - S u)
    nr = sqrt(fma chain of the S squares x_k^2)    nr = |x| (1 + e),  |e| <= gamma_S / 2 + u   (all terms positive)
and then divides.  Mode 1: score^ = a^ / nr / post_div, two more roundings:

    |score^ - score|  <=  S u T / (|x| post_div)  +  (S / 2 + 3) u |score|        (first order)

One more unit of u on each term covers the second order ((S u)^2 < 1e-10 u for S <= 600) and the error of the np.longdouble
reference itself (S 2^-64 T < u T): c1(S) = S + 1, c2(S) = S / 2 + 4.
Mode 0: s0 and s1 (one division each) lie within d_j = (S + 1) u T_j / |x| + (S / 2 + 3) u |s_j| of their exact values.  The
epilogue computes c^ = fl(1 - fl(s1^2)); with a = |s1| + d1, |c^ - c| <= dc = 2 a d1 + 2 u (both roundings act on numbers <= 1).
On the box c >= c_lo = c - dc (the bound is infinite where c_lo <= 0), and by the mean-value theorem
|1 / sqrt(c^) - 1 / sqrt(c)| <= dc / (2 c_lo^(3/2)), so before the last two roundings (sqrt, divide)

    E = d0 / sqrt(c_lo) + |s0| dc / (2 c_lo^(3/2))          ( = d0 / sqrt(c) + |s0| a d1 / c^(3/2) to first order )

and the bound is E + 3 u (|score| + E): two roundings and one unit for the second order and the reference.  Where s1 is 1e-14
from -1 (the mask's threshold) c is 2e-14 and the second term is large -- by derivation.  Derived, not tuned: a result outside
it is a finding.
"""
import functools

import numpy as np

U = 2.0 ** -53
LD = np.longdouble
LONGDOUBLE_OK = bool(np.finfo(np.longdouble).eps <= 2.0 ** -63)
LONGDOUBLE_WHY = ('np.longdouble has eps = %g > 2^-63 on this platform: no reference more precise than float64 to hold K3 against'
                  % float(np.finfo(np.longdouble).eps))

TILE = 128        # BC_TILE: rows per tile, two per lane
WAVES = 4         # BC_SWEEP_WAVES: tiles per block and grid stride
UNROLL = 10       # BC_SWEEP_U
PICK_THREADS = {'k_local_winner': 256, 'dev_pick_blocks': 512}
WIN, RUN = 3.7, 0.2
RUN_COS = 0.999


# ------------------------------------------------------------------ the grid of bc_sweep_grid, restated
def sweep_grid(ntiles, s, n_cu, per_cu_env=0):
    """bc_sweep_plan (csrc/bc_sweep_plan.h) restated; held against the header by the CPU test"""
    per_cu = 1 if s >= 64 else (2 if s >= 24 else 4)
    if per_cu_env > 0:
        per_cu = per_cu_env
    return max(1, min((ntiles + WAVES - 1) // WAVES, n_cu * per_cu))


def ntiles_of(n):
    return (n + TILE - 1) // TILE


def locate(r, grid):
    """where the sweep meets local row r: dict(tile, lane, half, wave, block, stride)"""
    t = r // TILE
    return dict(tile=t, lane=(r % TILE) // 2, half=r % 2, wave=t % WAVES, block=(t // WAVES) % grid, stride=(t // WAVES) // grid)


def row_at(block, stride, wave, lane, half, grid):
    return ((block + stride * grid) * WAVES + wave) * TILE + 2 * lane + half


# ------------------------------------------------------------------ the planted problem
def _seed(n, S, mode, seed):
    return (1000003 * n + 7919 * S + 31 * mode + seed) % (2 ** 31)


@functools.lru_cache(maxsize=8)
def background(n, S, mode, seed=0):
    """(phi [n x S], v, g_run): background rows only, read-only.  v: mode 1 a unit [S]; mode 0 [S x 2] orthonormal (cdir, xw)."""
    assert S >= (3 if mode == 0 else 2), 'no unit vector orthogonal to the sweep vectors'
    rng = np.random.RandomState(_seed(n, S, mode, seed))
    nv = 2 if mode == 0 else 1
    Q = np.linalg.qr(rng.randn(S, nv + 1))[0]
    V, g_run = Q[:, :nv], Q[:, nv]
    G = rng.randn(n, S)
    for _ in range(2):                                   # (twice: orthogonal to 1e-16 also where S - nv is 1)
        G -= G.dot(V).dot(V.T)
    G /= np.sqrt((G ** 2).sum(axis=1))[:, None]
    a = rng.uniform(-1., 0.5, size=n)
    b = rng.uniform(-1., 1., size=n) if mode == 0 else np.zeros(n)
    scale = 10.0 ** rng.uniform(-3., 3., size=n)
    phi = G + a[:, None] * V[:, 0][None, :]
    if mode == 0:
        phi += b[:, None] * V[:, 1][None, :]
    phi *= scale[:, None]
    v = np.ascontiguousarray(V if mode == 0 else V[:, 0])
    for arr in (phi, v, g_run):
        arr.setflags(write=False)
    return phi, v, g_run


def special_rows(v, g_run, mode):
    cdir = v[:, 0] if mode == 0 else v
    return WIN * cdir, RUN * (RUN_COS * cdir + np.sqrt(1. - RUN_COS ** 2) * g_run)


def runner_positions(n, winners):
    p = min(winners)
    return sorted(set(q for q in (p - 1, p + 1, p - 2, p + 2, p - TILE, p + TILE, 0, n - 1) if 0 <= q < n) - set(winners))


def planted(n, S, mode, winners, seed=0):
    """(phi, v, runners): a fresh Phi with the winning row at every index of `winners` (more than one: exact duplicates, a tie)
    and runners-up around the lowest of them."""
    bg, v, g_run = background(n, S, mode, seed)
    win, run = special_rows(v, g_run, mode)
    phi = bg.copy()
    runners = runner_positions(n, winners)
    phi[runners] = run
    phi[list(winners)] = win
    return phi, v, runners


def runners_alone(n, S, mode, p, seed=0):
    """(phi, v, expected index): the planted problem with a runner-up in the winner's place too -- equal rows, so the lowest of
    them wins, and the value returned is the runner-up's (0.999, a row with a component off the sweep vector)"""
    phi, v, runners = planted(n, S, mode, (p,), seed)
    phi[p] = phi[runners[0]]
    if p > TILE + 2:                                      # (row 0 back to the background: the lowest runner-up is p - 128)
        phi[0] = background(n, S, mode, seed)[0][0]
        runners = [q for q in runners if q != 0]
    return phi, v, min(runners + [p])


# ------------------------------------------------------------------ oracle, reference and bound
def numpy_scores(phi, v, mode, post_div=1.):
    """The reference's expressions in float64 NumPy (giga.py:31-38, frankwolfe.py:16-17): -inf where the row's norm is zero.
    np.argmax of it is the oracle for WHICH index wins (first NaN, first of equal maxima).  The dot products are row-wise sums,
    not BLAS calls: a gemv blocks its rows, and equal rows must get equal bits here as they do in the kernel."""
    n = phi.shape[0]
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        nrm = np.sqrt((phi ** 2).sum(axis=1))
        ok = nrm != 0.
        sc = np.full(n, -np.inf)
        if mode == 1:
            sc[ok] = (phi[ok] * v[None, :]).sum(axis=1) / nrm[ok] / post_div
        else:
            An = phi[ok] / nrm[ok][:, None]
            s0, s1 = (An * v[None, :, 0]).sum(axis=1), (An * v[None, :, 1]).sum(axis=1)
            good = np.logical_and(s1 > -1. + 1e-14, 1. - s1 ** 2 > 0.)
            den = np.where(good, np.sqrt(np.abs(1. - s1 ** 2)), np.inf)
            sc[ok] = s0 / den
    return sc


def _ld_parts(rows, v, mode):
    x = np.atleast_2d(rows).astype(LD)
    nr = np.sqrt((x * x).sum(axis=1))
    V = (v if mode == 0 else v[:, None]).astype(LD)
    dots = x.dot(V)                                       # [m x nv]
    T = np.abs(x).dot(np.abs(V))
    return nr, dots, T


def ref_score(rows, v, mode, post_div=1.):
    """exact-formula scores of non-zero, unmasked rows in np.longdouble from the float64 inputs"""
    assert LONGDOUBLE_OK, LONGDOUBLE_WHY
    nr, dots, _ = _ld_parts(rows, v, mode)
    if mode == 1:
        return dots[:, 0] / nr / LD(post_div)
    s0, s1 = dots[:, 0] / nr, dots[:, 1] / nr
    return s0 / np.sqrt(1 - s1 * s1)


def c1(S):
    return S + 1


def c2(S):
    return S / 2. + 4.


def bound(rows, v, mode, post_div=1.):
    """the module docstring's bound on |device score - ref_score|, one per row (np.longdouble; inf where c_lo <= 0)"""
    assert LONGDOUBLE_OK, LONGDOUBLE_WHY
    S = np.atleast_2d(rows).shape[1]
    u = LD(U)
    nr, dots, T = _ld_parts(rows, v, mode)
    if mode == 1:
        return c1(S) * u * T[:, 0] / (nr * LD(post_div)) + c2(S) * u * np.abs(dots[:, 0] / nr / LD(post_div))
    s = dots / nr[:, None]
    d = c1(S) * u * T / nr[:, None] + (S / 2. + 3.) * u * np.abs(s)
    s0, s1, d0, d1 = s[:, 0], s[:, 1], d[:, 0], d[:, 1]
    c = 1 - s1 * s1
    dc = 2 * (np.abs(s1) + d1) * d1 + 2 * u
    c_lo = c - dc
    out = np.full(s0.shape, np.inf, dtype=LD)
    okc = c_lo > 0
    E = d0[okc] / np.sqrt(c_lo[okc]) + np.abs(s0[okc]) * dc[okc] / (2 * c_lo[okc] ** LD(1.5))
    out[okc] = E + 3 * u * (np.abs(s0[okc] / np.sqrt(c[okc])) + E)
    return out


def ratio(val, row, v, mode, post_div=1.):
    """|val - reference| / bound for one row (<= 1: inside); inf for a NaN"""
    if np.isnan(val):
        return float('inf')
    return float(np.abs(LD(val) - ref_score(row, v, mode, post_div)[0]) / bound(row, v, mode, post_div)[0])


# ------------------------------------------------------------------ planted cases that do not depend on the device
N_ODD, N_EVEN = 1445, 1446        # 12 tiles in 3 blocks; the last tile ragged with its last row in half .x / .y
S_FULL = (4, 11)                  # every position
S_ALL = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 19, 20, 21, 30, 100, 257, 600)
TINY_N = (1, 2, 127, 128, 129)


def small_positions(n):
    """{label: p} over the n rows of N_ODD / N_EVEN (grid 3), derived from the kernel's structure"""
    g = sweep_grid(ntiles_of(n), 4, 128)
    assert g == 3
    pos = {}
    for lane in (0, 63):
        for half in (0, 1):
            pos['tile 0 lane %d half %d' % (lane, half)] = row_at(0, 0, 0, lane, half, g)
    for w in range(WAVES):
        pos['block 0 wave %d' % w] = row_at(0, 0, w, 17 + w, w % 2, g)
    pos['block 1 first tile first row'] = row_at(1, 0, 0, 0, 0, g)
    pos['block 1 first tile'] = row_at(1, 0, 0, 38, 1, g)
    pos['last block first tile'] = row_at(2, 0, 0, 5, 0, g)
    pos['last block last tile first row'] = row_at(2, 0, 3, 0, 0, g)
    pos['last row'] = n - 1
    pos['last row but one'] = n - 2
    return pos


SHORT = ('last row', 'block 0 wave 1', 'block 1 first tile', 'tile 0 lane 63 half 1')


def modes_of(S):
    return [m for m in (0, 1) if S >= (3 if m == 0 else 2)]


def small_cases(S, mode):
    """[(label, n, winners)] at this S: every position at S in S_FULL (both n, and the tiny n), the SHORT ones otherwise"""
    out = []
    if S in S_FULL:
        for n in (N_ODD, N_EVEN):
            out += [('n %d %s' % (n, k), n, (p,)) for k, p in small_positions(n).items()]
        for n in TINY_N:
            out += [('n %d row %d' % (n, p), n, (p,)) for p in sorted(set((0, n // 2, n - 1)))]
    else:
        pos = small_positions(N_ODD)
        out += [('n %d %s' % (N_ODD, k), N_ODD, (pos[k],)) for k in SHORT]
    return out


def small_ties(n=N_ODD):
    """[(label, n, winners)]: exact duplicates of the winning row, pairwise; the lowest index must win"""
    g = 3
    return [('two halves of a lane', n, (row_at(1, 0, 2, 40, 0, g), row_at(1, 0, 2, 40, 1, g))),
            ('two lanes of a wave', n, (row_at(0, 0, 1, 5, 0, g), row_at(0, 0, 1, 45, 0, g))),
            ('two lanes of a wave, the first in half y', n, (row_at(0, 0, 1, 5, 1, g), row_at(0, 0, 1, 6, 0, g))),
            ('two waves of a block', n, (row_at(0, 0, 1, 30, 1, g), row_at(0, 0, 3, 2, 0, g))),
            ('two blocks', n, (row_at(0, 0, 2, 9, 0, g), row_at(2, 0, 1, 9, 0, g))),
            ('every row of three tiles', 300, tuple(range(300)))]


OFFSETS = (0, 12345, 2 ** 31 - 64, 2 ** 32 - 64, 2 ** 33 + 5)
OFFSET_POSITIONS = (58, 63, 64, 65, 200, N_ODD - 1)        # offset + 64 is 2^31 / 2^32: the shard's indices cross it inside the Phi


# ------------------------------------------------------------------ cases whose n follows the device's CU count
def stride_case(n_cu, S=4):
    """BC_SWEEP_BLOCKS_PER_CU=1: grid = n_cu, three grid strides; the last tile (last block, third stride, wave 3) ragged.
    dict(n, grid, per_cu, positions {label: p}, ties [(label, winners)])"""
    G = n_cu
    n = 3 * WAVES * TILE * G - 51
    assert sweep_grid(ntiles_of(n), S, n_cu, 1) == G
    pos = {'block 0 second stride': row_at(0, 1, 1, 20, 1, G), 'block 0 third stride': row_at(0, 2, 2, 63, 0, G),
           'last block second stride': row_at(G - 1, 1, 0, 0, 0, G), 'last block third stride': row_at(G - 1, 2, 3, 7, 1, G),
           'last row': n - 1, 'block 1 first stride': row_at(1, 0, 3, 11, 0, G)}
    ties = [('block 0 second stride against block 1', (row_at(1, 0, 3, 11, 0, G), row_at(0, 1, 2, 11, 0, G))),
            ('last block second stride against block 0 third stride', (row_at(G - 1, 1, 0, 3, 1, G), row_at(0, 2, 0, 3, 1, G)))]
    return dict(n=n, S=S, grid=G, per_cu=1, positions=pos, ties=ties)


def second_stride_case(n_cu, S=11):
    """BC_SWEEP_BLOCKS_PER_CU=1, a wider Phi: one full stride, then blocks 0 and 1 a second time (block 1's last tile ragged)"""
    G = n_cu
    n = WAVES * TILE * G + WAVES * TILE + 3 * TILE + 77
    assert sweep_grid(ntiles_of(n), S, n_cu, 1) == G
    pos = {'block 0 second stride': row_at(0, 1, 3, 33, 0, G), 'block 1 second stride last row': n - 1,
           'last block': row_at(G - 1, 0, 3, 63, 1, G)}
    ties = [('block 0 second stride against block 1', (row_at(1, 0, 3, 11, 0, G), row_at(0, 1, 2, 11, 0, G)))]
    return dict(n=n, S=S, grid=G, per_cu=1, positions=pos, ties=ties)


def wide_case(n_cu, S=4):
    """No override, S < 24: grid = 4 n_cu blocks (1024 on 256 CUs) and 300 rows more, so that block 0 walks a second stride.
    Candidates beyond 256 and 512 take the second and third trip of a 256-thread reducer, beyond 512 the second of a
    512-thread one."""
    G = 4 * n_cu
    n = WAVES * TILE * G + 300
    assert sweep_grid(ntiles_of(n), S, n_cu, 0) == G
    pos = {'block 3': row_at(3, 0, 1, 9, 1, G), 'last block last tile': row_at(G - 1, 0, 3, 63, 1, G),
           'block 0 second stride': row_at(0, 1, 1, 2, 0, G), 'last row': n - 1}
    ties = []
    for k in (256, 512):
        if k + 3 < G:
            pos['block %d' % (k + 3)] = row_at(k + 3, 0, 2, 31, 0, G)
            ties.append(('blocks 3 and %d' % (k + 3), (row_at(3, 0, 2, 31, 0, G), row_at(k + 3, 0, 2, 31, 0, G))))
    ties.append(('block 0 second stride against the last block', (row_at(G - 1, 0, 0, 1, 1, G), row_at(0, 1, 0, 1, 1, G))))
    return dict(n=n, S=S, grid=G, per_cu=0, positions=pos, ties=ties)


# ------------------------------------------------------------------ ties decided without a planted winner
def sign_case(S=1):
    """S = 1 (or 2: a zero second column): every score is exactly +1 or -1 -- sqrt(fl(x^2)) is |x| -- and the winner is the first
    positive row, after leading negative rows and zero rows.  (phi, v for mode 1, v for mode 0, winner)"""
    rng = np.random.RandomState(77)
    n = 700
    x = -np.abs(rng.randn(n)) * 10.0 ** rng.uniform(-3, 3, size=n)
    x[[0, 5, 127, 128, 300]] = 0.
    first = 389                                           # tile 3, lane 2, half 1
    later = rng.permutation(np.arange(first + 1, n))[:150]
    x[later] = np.abs(x[later]) + 1e-3
    x[first] = 0.37
    phi = np.zeros((n, S))
    phi[:, 0] = x
    v1 = np.zeros(S)
    v1[0] = 1.
    v0 = np.zeros((S, 2))
    v0[0, 0] = 1.
    if S > 1:
        v0[1, 1] = 1.
    return phi, v1, v0, first


# ------------------------------------------------------------------ NaN
def nan_cases():
    """[(label, phi, v, mode, expected index)]: NumPy's rule -- NaN beats everything, the first NaN wins.  n = N_ODD, S = 5."""
    out = []
    for mode in (1, 0):
        for label, p, bad in (('a NaN row after the winner', 300, (900,)), ('a NaN row before the winner', 900, (300,)),
                              ('two NaN rows in two blocks', 700, (1300, 300)), ('two NaN rows in one lane', 700, (1101, 1100)),
                              ('a NaN in the last row', 10, (N_ODD - 1,))):
            phi, v, _ = planted(N_ODD, 5, mode, (p,))
            for i, r in enumerate(bad):
                phi[r, (2 + i) % 5] = np.nan
            out.append(('mode %d: %s' % (mode, label), phi, v, mode, min(bad)))
    phi, v, _ = planted(N_ODD, 5, 1, (640,))
    phi[:2] = 0.
    vn = v.copy()
    vn[3] = np.nan
    out.append(('a NaN in v: the first row with a non-zero norm', phi, vn, 1, 2))
    out.append(('all rows zero', np.zeros((300, 5)), v, 1, -1))
    return out


def nan_stride_case(n_cu):
    """two NaN rows, the higher index in the lower block (block 0's second stride against block 1): the first NaN row wins"""
    c = second_stride_case(n_cu)
    lo, hi = c['ties'][0][1]
    phi, v, _ = planted(c['n'], c['S'], 1, (c['positions']['last block'],))
    phi[hi, 1] = np.nan
    phi[lo, 4] = np.nan
    return dict(c, phi=phi, v=v, expect=lo)


# ------------------------------------------------------------------ the GIGA validity mask
MASK_S = 4
MASK_CDIR_SCALE = 1e15


def mask_vectors():
    v = np.zeros((MASK_S, 2))
    v[1, 0] = MASK_CDIR_SCALE       # cdir = 1e15 e1 (the kernel does not ask for a unit vector): a masked row's s0 is huge
    v[0, 1] = 1.                    # xw = e0
    return v


def masked_rows(n, seed=5):
    """rows (c, d, 0, 0) with c = +-2^k and |d| <= 2^-40 |c|: c^2 + d^2 rounds to c^2, the norm is |c| and s1 = +-1 EXACTLY, so
    every row is masked whichever test catches it, and scores s0 / inf = +-0 with the sign of d; s0 = 1e15 d / |c| is 200 .. 900."""
    rng = np.random.RandomState(seed)
    c = np.where(rng.rand(n) < 0.5, -1., 1.) * 2.0 ** rng.randint(-8, 9, size=n)
    d = np.where(rng.rand(n) < 0.5, -1., 1.) * np.abs(c) * 2.0 ** -40 * rng.uniform(0.25, 1., size=n)
    phi = np.zeros((n, MASK_S))
    phi[:, 0], phi[:, 1] = c, d
    return phi


def mask_cases():
    """[(label, phi, v, expected index)] -- exact arithmetic wherever the side of a threshold matters"""
    v = mask_vectors()
    out = []
    phi = masked_rows(300)
    phi[0, :2] = (-2., 2.0 ** -41)           # s1 = -1: masked by the first test under any reading of the second
    phi[1, :2] = (4., 2.0 ** -41)            # s1 = +1, s0 > 0: 1 - s1^2 is exactly 0
    out.append(('all rows masked: row 0', phi, v, 0))
    phi = masked_rows(300)
    phi[0, :2] = (2., -2.0 ** -41)           # scores -0.0
    phi[1, :2] = (2., 2.0 ** -41)            # scores +0.0: equal, the lower index wins
    out.append(('a -0.0 score before a +0.0 score', phi, v, 0))
    phi = masked_rows(300)
    phi[:, 1] = -np.abs(phi[:, 1])           # every masked row scores -0.0 ...
    phi[211] = (0.5, 3e-16, 0.5, 0.5)        # ... and one modest unmasked row a positive 0.35 / sqrt(1 - 1/3)
    out.append(('all masked but one modest row', phi, v, 211))
    phi = masked_rows(300)
    phi[:, 1] = -np.abs(phi[:, 1])
    below, above = threshold_rows()
    phi[100], phi[200] = below, above
    out.append(('s1 on either side of -1 + 1e-14', phi, v, 200))
    return out


THRESH = -1. + 1e-14
THRESH_MARGIN = 20 * U


def threshold_rows():
    """(masked row, unmasked row): (-1, d1, d2, 0) with s1 = -1 / sqrt(1 + d1^2 + d2^2) at least 20 * 2^-53 below / above
    -1 + 1e-14 in float64 and in np.longdouble alike (asserted here, at generation time, and by the CPU test).  The unmasked row
    scores s0 / 2.4e-7 = 0.5e15; the masked one would score 1e15 if the threshold let it through."""
    rows = []
    for d1, d2, want_masked in ((1.0e-7, 0., True), (1.2e-7, 1.2e-7 * np.sqrt(3.), False)):
        row = np.array([-1., d1, d2, 0.])
        s1_64, s1_ld = threshold_s1(row)
        for s1 in (s1_64, s1_ld):
            assert (s1 <= THRESH) == want_masked and abs(s1 - LD(THRESH)) >= THRESH_MARGIN, (d1, d2, s1)
        rows.append(row)
    return rows


def threshold_s1(row):
    s64 = row[0] / np.sqrt((row ** 2).sum())
    x = row.astype(LD)
    return s64, x[0] / np.sqrt((x * x).sum())
