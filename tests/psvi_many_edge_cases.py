"""Shared by tests/test_psvi_many_edges_cpu.py and tests/test_gpu_psvi_many_edges.py (no test collects from this file): the
batched BatchPSVI run (include/beta_cores_psvi_many.h, include/beta_cores_psvi_curve.h) at the edges of its tiles and at its
limits.  Two tables of shapes, one per kind, chosen from the branches of csrc/bc_psvi_many_dev.h, csrc/bc_psvi_many.hip and
csrc/bc_vi_laplace_dev.h; the recipe of the runs (what tests/test_gpu_psvi_many.py and tests/test_gpu_psvi_many_gauss.py build,
with the number of data rows as an argument); one runner for both kinds; and the check of every stage of a run's last step.
No tolerance is new: every stage is held to the long-double restatements and derived bounds of tests/psvi_many_cases.py and
tests/psvi_many_gauss_cases.py, which take any shape, and ADAM to util/opt.py's statements.

What a row reaches (16 = BC_PM_TILE, 256 = BC_PM_BLOCK, 512 = BC_VIL_BLOCK = BC_PM_POST_BLOCK):
  S      bc_pm_tile deals ceil(S / 16) sample tiles to 4 waves: S <= 16 leaves three waves idle, 64 is one tile per wave, 65 opens
         a second round of one column, 255 / 256 are the ragged and the full last round (256: a sample per thread of
         bc_pm_tile_colsum and bc_pm_resid); S = 1 makes a row's mean its only value.  bc_pm_post_products (Gaussian kind) deals
         them to 8 waves: 128 is one per wave, 129 a second round of one sample.
  D      the k-loop of bc_pm_tile steps by 4: D = 1, 2 are less than one step, 5, 65, 127 leave a partial one.  bc_vil_gram slices
         the rows over the waves for D < 32 (BC_VIL_PART_DOUBLES): 31 / 32.  bc_pm_post_products walks ceil(D / 16) coordinate
         tiles with a triangular k-range: 15, 16, 17, 127.
  m      ceil(m / 16) point tiles: 16, 32 are full, 33 has a third tile of one row; bc_pm_resid and bc_pm_adam stride by 256
         threads (255 / 257), bc_vil_value by 512 (513); the fit at m (D + 1) > 60000, where k_vi_laplace's own tests end.
  n_sub  bc_pm_resid adds ceil(n_sub / 16) partial sums in tile order: 1, 15, 16, 17 are the one-tile edges, 4097 is 257 sums
         with one row in the last, BC_PSVI_MANY_MAX_SUB is 16384 sums."""
import os
import re

import numpy as np

import psvi_many_cases as pm
import psvi_many_gauss_cases as pg

ROOT = pm.ROOT
LOGISTIC, GAUSS = 'logistic', 'gauss'
SAMPLER_KIND = {GAUSS: 1, LOGISTIC: 2}      # BC_VI_SAMPLER_GAUSS, BC_VI_SAMPLER_LOGISTIC
N_ROWS = 600

# (D, m, S, n_sub, diag, n_rows)
LOGISTIC_TABLE = [
    (1, 16, 1, 1, 0, 600),             # the exact case: one full point tile, one gathered row
    (2, 33, 16, 15, 1, 600),           # half a k-step; one full sample tile; a ragged gathered tile; a third point tile of one row
    (5, 257, 65, 17, 0, 600),          # a partial k-step; a second wave round of one column; m > 256
    (64, 64, 64, 16, 0, 600),          # everything exactly full: one tile per wave, 4 point tiles, 1 row tile
    (65, 65, 255, 4097, 0, 600),       # 257 partial sums, the last of one row; a ragged 16th sample tile
    (31, 32, 17, 16, 1, 600),          # the last D with the sliced Gram product
    (32, 513, 256, 33, 0, 600),        # the first D without it; m > 512; S at its limit
    (127, 255, 15, 1, 0, 600),         # ragged everything at a large D
    (128, 513, 256, 17, 1, 600),       # D and S at their limits together
    (128, 1024, 16, 16, 0, 1024),      # the fit beyond m (D + 1) <= 60000
    (16, 4096, 7, 37, 0, 4096),        # m at its limit with the sliced Gram product
    (33, 4096, 17, 17, 1, 4096),       # m at its limit without it
    (1, 4096, 16, 16, 0, 4096),        # m at its limit, D = 1
    (128, 4096, 7, 16, 0, 4096),       # m and D at their limits
    (3, 17, 7, 262144, 0, 600),        # n_sub at its limit: 16384 partial sums
]
# the same; diag is always 0
GAUSS_TABLE = [
    (1, 16, 1, 1, 0, 600),             # the exact case
    (2, 33, 16, 15, 0, 600),           # as above
    (15, 257, 17, 17, 0, 600),         # one ragged coordinate tile; m > 256
    (16, 32, 128, 16, 0, 600),         # one full coordinate tile; one sample tile per wave of the posterior block
    (17, 64, 255, 4097, 0, 600),       # a second coordinate tile of one column (the triangular k-range); a ragged last round
    (127, 65, 256, 16, 0, 600),        # a ragged 8th coordinate tile; S at its limit
    (128, 513, 129, 33, 0, 600),       # a second round of one sample; 132 KiB of LDS
    (3, 4096, 7, 37, 0, 4096),         # m at its limit
    (3, 17, 7, 262144, 0, 600),        # n_sub at its limit
]
TABLES = {LOGISTIC: LOGISTIC_TABLE, GAUSS: GAUSS_TABLE}


def row_id(row):
    return 'D%d-m%d-S%d-nsub%d-diag%d' % tuple(row[:5])


def header_constants():
    """the limits as include/beta_cores_psvi_many.h (and the header it takes the largest D from) state them"""
    src = open(os.path.join(ROOT, 'include', 'beta_cores_psvi_many.h')).read() + open(os.path.join(ROOT, 'include', 'beta_cores_viopt.h')).read()
    out = {name: int(re.search(r'#define %s (\d+)\b' % name, src).group(1))
           for name in ('BC_PSVI_MANY_MAX_SAMPLES', 'BC_PSVI_MANY_MAX_SUB', 'BC_PSVI_MANY_MAX_PROBLEMS', 'BC_PSVI_MANY_MAX_POINTS', 'BC_VI_MAX_DIM')}
    out['BC_PSVI_MANY_MAX_WORK_DOUBLES'] = 1 << int(re.search(r'#define BC_PSVI_MANY_MAX_WORK_DOUBLES \(1ll << (\d+)\)', src).group(1))
    return out


def check_tables():
    """What the two tables as a whole must hold, read against the header's constants (and the block sizes the kernels state)."""
    from beta_cores_amd import _native as N
    H = header_constants()
    dev = open(os.path.join(ROOT, 'beta_cores_amd', 'csrc', 'bc_psvi_many_dev.h')).read()
    fit = open(os.path.join(ROOT, 'beta_cores_amd', 'csrc', 'bc_vi_laplace_dev.h')).read()
    run = open(os.path.join(ROOT, 'beta_cores_amd', 'csrc', 'bc_psvi_many.hip')).read()
    tile = int(re.search(r'#define BC_PM_TILE (\d+)\b', dev).group(1))
    block = int(re.search(r'#define BC_PM_BLOCK (\d+)\b', dev).group(1))
    fit_block = int(re.search(r'#define BC_VIL_BLOCK (\d+)\b', fit).group(1))
    post_block = int(re.search(r'#define BC_PM_POST_BLOCK (\d+)\b', run).group(1))
    assert (tile, block, fit_block, post_block) == (16, 256, 512, 512)      # (what the literals below are derived from)
    assert re.search(r'#define BC_VIL_PART_DOUBLES\(d\) \(\(d\) < 32 \?', fit)
    smax, nmax, mmax, dmax = H['BC_PSVI_MANY_MAX_SAMPLES'], H['BC_PSVI_MANY_MAX_SUB'], H['BC_PSVI_MANY_MAX_POINTS'], H['BC_VI_MAX_DIM']
    lo, ga = LOGISTIC_TABLE, GAUSS_TABLE
    assert set(r[2] for r in lo) >= {1, tile, block // 4, block // 4 + 1, smax - 1, smax} and smax == block
    assert set(r[2] for r in ga) >= {1, tile, post_block // 4, post_block // 4 + 1, smax - 1, smax}
    assert set(r[1] for r in lo) >= {tile, 2 * tile, block - 1, block + 1, fit_block + 1, mmax}
    assert set(r[1] for r in ga) >= {tile, 2 * tile, 2 * tile + 1, block + 1, fit_block + 1, mmax}
    for table in (lo, ga):
        assert set(r[3] for r in table) >= {1, tile - 1, tile, tile + 1, tile * block + 1, nmax}
    assert set(r[0] for r in lo) >= {1, 2, 31, 32, dmax - 1, dmax}
    assert set(r[0] for r in ga) >= {1, 2, tile - 1, tile, tile + 1, dmax - 1, dmax}
    assert any(r[1] * (r[0] + 1) > 60000 for r in lo) and (dmax, mmax) in set(r[:2] for r in lo)
    assert set(r[4] for r in lo) == {0, 1} and set(r[4] for r in ga) == {0}
    assert lo[0][:4] == ga[0][:4] == (1, 16, 1, 1)                          # the exact case comes first
    lib = N.load()
    for kind, table in TABLES.items():
        assert len(set(table)) == len(table)
        for d, m, s, n_sub, diag, n_rows in table:
            assert 1 <= d <= dmax and 1 <= m <= min(mmax, n_rows) and 1 <= s <= smax and 1 <= n_sub <= nmax
            need = lib.bc_psvi_curve_work_doubles(m, 1, d, s, n_sub, 2, SAMPLER_KIND[kind])
            assert 0 < need < H['BC_PSVI_MANY_MAX_WORK_DOUBLES'], (kind, d, m, s, n_sub, need)
    return H


# ---------------------------------------------------------------- the recipe
_host_rows = {}


def host_rows(kind, d, n_rows=N_ROWS):
    """n_rows rows of width d, values a float32 holds (both storages carry the same rows), once per process.  Logistic kind:
    z = y * x as tests/test_gpu_psvi_many.py draws them; Gaussian kind: psvi_many_gauss_cases.make_rows."""
    if (kind, d, n_rows) not in _host_rows:
        if kind == LOGISTIC:
            rng = np.random.RandomState(4100 + d)
            x = rng.randn(n_rows, d)
            y = np.where(rng.rand(n_rows) < 1. / (1. + np.exp(-x.dot(rng.randn(d)) / np.sqrt(d))), 1., -1.)
            z = (y[:, None] * x).astype(np.float32).astype(np.float64)
        else:
            z = pg.make_rows(np.random.RandomState(4300 + d), n_rows, d)
        z.setflags(write=False)
        _host_rows[kind, d, n_rows] = z
    return _host_rows[kind, d, n_rows]


def recipe(kind, d, s, n_sub, itrs, sizes=None, n_rows=N_ROWS, starts=None):
    """What a run is made of, on the host: nested initial points rows[perm[:m]] (or rows[starts[p]]), weights n_rows / m, steps
    1 / (1 + i), seeded normals E (itrs x S x D) and row numbers idx (itrs x n_sub), the Gaussian kind's model."""
    z = host_rows(kind, d, n_rows)
    perm = np.random.RandomState(9).permutation(n_rows)
    rng = np.random.RandomState(1000 + d + s)
    E, idx = rng.randn(itrs, s, d), rng.randint(n_rows, size=(itrs, n_sub))
    starts = [perm[:m] for m in sizes] if starts is None else [np.asarray(a) for a in starts]
    sizes = [len(a) for a in starts]
    return dict(kind=kind, z=z, perm=perm, E=E, idx=idx, d=d, s=s, n_sub=n_sub, itrs=itrs, n_rows=n_rows, sizes=sizes, starts=starts,
                pts0=[z[a] for a in starts], w0=[np.full(m, float(n_rows) / m) for m in sizes],
                steps=np.array([[1. / (1. + i) for i in range(itrs)] for _ in sizes]).reshape(len(sizes), itrs),
                mdl=pg.make_model(d) if kind == GAUSS else None)


def first_step(kind, row):
    """One row of a table as ONE step of the matching host harness from the run's initial state: the points, weights, gathered
    rows and normals of step 0 of the recipe, zero moments, step_i = 0."""
    d, m, s, n_sub, diag, n_rows = row
    rc = recipe(kind, d, s, n_sub, 1, [m], n_rows)
    st = dict(d=d, m=m, s=s, n_sub=n_sub, scale=float(n_rows) / n_sub, pts=rc['pts0'][0], w=rc['w0'][0], E=rc['E'][0], rows=rc['z'][rc['idx'][0]],
              step_i=0, step=1., c1=1. - pm.B1, c2=1. - pm.B2, m1w=np.zeros(m), m1p=np.zeros((m, d)), m2w=np.zeros(m), m2p=np.zeros((m, d)))
    if kind == LOGISTIC:
        st.update(diag=bool(diag), start=np.zeros(d))
    else:
        st.update({k: v for k, v in rc['mdl'].items() if k != 'd'})
    return st


def state(w, pts):
    return np.concatenate((np.asarray(w), np.asarray(pts).ravel()))


def check_stages(kind, label, pts, w, E, rows, scale, diag, mdl, out):
    """Mode (or mean) and draw, target, resid, g_w and g_p of one problem's step under the existing bounds, on the step's own
    inputs; `out`: what the build under test gave (mode, theta, target, resid, gw, gp).  Returns the worst error / bound per stage."""
    if kind == LOGISTIC:
        r_m, r_d = pm.check_mode_and_draw(label, pts, w, E, diag, out['mode'], out['theta'])
        r_t, r_r, r_g = pm.check_stage34(label, rows, scale, pts, w, out['theta'], out['target'], out['resid'], out['gw'])
        r_p = pm.check_point_grad(label, pts, w, out['theta'], out['resid'], out['gp'])
    else:
        r_m, r_d = pg.check_mean_and_draw(label, pts, w, E, mdl, out['mode'], out['theta'])
        r_t, r_r, r_g = pg.check_stage34(label, rows, scale, pts, w, out['theta'], mdl, out['target'], out['resid'], out['gw'])
        r_p = pg.check_point_grad(label, pts, w, out['theta'], out['resid'], mdl, out['gp'])
    return {'mode': float(r_m), 'draw': float(r_d), 'target': r_t, 'resid': r_r, 'gw': r_g, 'gp': r_p}


def check_host_step(kind, label, st, r):
    """A host harness result: the stages against long double, ADAM against util/opt.py's statements bit for bit."""
    assert r['status'] == 0, label
    ratios = check_stages(kind, label, st['pts'], st['w'], st['E'], st['rows'], st['scale'], st.get('diag', False), st if kind == GAUSS else None, r)
    m = st['m']
    x, m1, m2 = pm.adam_step(state(st['w'], st['pts']), state(r['gw'], r['gp']), state(st['m1w'], st['m1p']), state(st['m2w'], st['m2p']),
                             st['step'], st['step_i'], np.arange(m))
    for name, got, want in (('x', state(r['w'], r['pts']), x), ('mom1', state(r['m1w'], r['m1p']), m1), ('mom2', state(r['m2w'], r['m2p']), m2)):
        assert np.array_equal(got, want), (label, name)
    return ratios


# ---------------------------------------------------------------- the runner (GPU)
_device_rows = {}


def device_rows(bc, kind, d, n_rows=N_ROWS, f32=False):
    key = (kind, d, n_rows, f32)
    if key not in _device_rows:
        z = host_rows(kind, d, n_rows)
        _device_rows[key] = bc.DeviceData(z.astype(np.float32), dtype=np.float32) if f32 else bc.DeviceData(np.array(z))
    return _device_rows[key]


class Run:
    """One native run of either kind on the recipe's problems.  Chunks of opt_itrs - 1 steps and 1 step (or `chunk`), so that the
    seam (bpsvi.psvi_many_last_step) is read before and after the last step."""

    def __init__(self, bc, kind, d, s, n_sub, itrs, diag=False, sizes=None, n_rows=N_ROWS, f32=False, starts=None, chunk=None):
        from beta_cores_amd.coreset import bpsvi
        self.__dict__.update(recipe(kind, d, s, n_sub, itrs, sizes, n_rows, starts))
        self.diag, self.f32 = bool(diag), f32
        dd = device_rows(bc, kind, d, n_rows, f32)
        self.seams, at = [], [0]

        def draw(k):
            out = self.E[at[0]:at[0] + k], self.idx[at[0]:at[0] + k]
            at[0] += k
            return out
        how = {}
        if kind == GAUSS:
            model = bc.likelihoods.GaussianLocation(self.mdl['Siginv'], self.mdl['logdet'])
            how = dict(model_id=model.model_id, sampler_kind=SAMPLER_KIND[GAUSS], model_params=model.params(),
                       sampler_params=np.concatenate((self.mdl['mu0'], self.mdl['Sig0inv'].ravel(), self.mdl['Siginv'].ravel())))
        else:
            how = dict(diag=self.diag)
        self.res = bpsvi.psvi_many_run(dd, self.pts0, self.w0, s, itrs, self.steps, draw, n_sub, n_total=n_rows,
                                       chunk_steps=chunk or max(itrs - 1, 1),
                                       on_chunk=lambda done: self.seams.append((done, bpsvi.psvi_many_last_step(dd.ctx, self.sizes, d, s))), **how)
        assert at[0] == itrs                                   # nothing was drawn past the last step
        self.last = self.seams[-1][1]

    def same_bits(self, other, mine=None, theirs=None):
        mine = range(len(self.sizes)) if mine is None else mine
        theirs = range(len(other.sizes)) if theirs is None else theirs
        return all(np.array_equal(self.res['w'][a], other.res['w'][b]) and np.array_equal(self.res['pts'][a], other.res['pts'][b])
                   and np.array_equal(self.res['modes'][a], other.res['modes'][b]) for a, b in zip(mine, theirs))

    def label(self, p):
        return '%s D %d S %d n_sub %d steps %d diag %d m %d (problem %d of %d)' % (self.kind, self.d, self.s, self.n_sub, self.itrs, self.diag,
                                                                                  self.sizes[p], p, len(self.sizes))


def check_last_step(r, problems=None):
    """Every stage of the last step of run `r`, per problem (all, or `problems`), on the device's own inputs: the snapshot is the
    previous chunk's state bit for bit (the initial state for a run of one step); mode (or mean) and draw, target, resid, g_w, g_p
    within the derived bounds; ADAM within 1 ulp of psvi_many_cases.adam_step; what _end hands out is the seam's state; no flag.
    Returns the worst error / bound per stage and the worst ADAM distance in ulp, and prints them."""
    itrs = r.itrs
    assert r.res['marked'] == [] and [done for done, _ in r.seams] == ([itrs] if itrs == 1 else [itrs - 1, itrs])
    L, ptr = r.last, r.last['row_ptr']
    before = r.seams[-2][1] if itrs > 1 else None              # its state AFTER step itrs - 2: the moments before the last step
    i = itrs - 1
    rows, scale = r.z[r.idx[i]], float(r.n_rows) / r.n_sub
    assert not L['flag'].any() and not r.res['status'].any()
    worst = {}
    for p in (range(len(r.sizes)) if problems is None else problems):
        m, label = r.sizes[p], r.label(p)
        sl = slice(ptr[p], ptr[p + 1])
        wb, pb = L['w_before'][sl], L['pts_before'][sl]
        if before is None:
            assert np.array_equal(wb, r.w0[p]) and np.array_equal(pb, r.pts0[p]), label
        else:
            assert np.array_equal(wb, before['w'][sl]) and np.array_equal(pb, before['pts'][sl]), label
        out = dict(mode=L['mode'][p], theta=L['theta'][p], target=L['target'][p], resid=L['resid'][p], gw=L['gw'][sl], gp=L['gp'][sl])
        ratios = check_stages(r.kind, label, pb, wb, r.E[i], rows, scale, r.diag, r.mdl, out)
        x0, g = state(wb, pb), state(out['gw'], out['gp'])
        m1 = np.zeros_like(x0) if before is None else state(before['mom1_w'][sl], before['mom1_p'][sl])
        m2 = np.zeros_like(x0) if before is None else state(before['mom2_w'][sl], before['mom2_p'][sl])
        x, m1, m2 = pm.adam_step(x0, g, m1, m2, r.steps[p, i], i, np.arange(m))
        for name, got, want in (('x', state(L['w'][sl], L['pts'][sl]), x), ('mom1', state(L['mom1_w'][sl], L['mom1_p'][sl]), m1),
                                ('mom2', state(L['mom2_w'][sl], L['mom2_p'][sl]), m2)):
            far = float(pm.ulps(got, want).max())
            assert far <= 1., (label, name, far)
            ratios['adam_ulp'] = max(ratios.get('adam_ulp', 0.), far)
        assert np.array_equal(r.res['w'][p], L['w'][sl]) and np.array_equal(r.res['pts'][p], L['pts'][sl]) and \
            np.array_equal(r.res['modes'][p], L['mode'][p]), label      # what _end hands out is the state the seam shows
        if r.kind == LOGISTIC:
            assert L['newton'][p, 0] >= 0 and L['newton'][p, 1] >= L['newton'][p, 0], label
        else:
            assert not L['newton'][p].any(), label
        for k, v in ratios.items():
            worst[k] = max(worst.get(k, 0.), v)
    print_worst('%s D %d S %d n_sub %d steps %d sizes %s' % (r.kind, r.d, r.s, r.n_sub, itrs, _short(r.sizes)), worst)
    return worst


def _short(sizes):
    return str(sizes) if len(sizes) <= 10 else '[%d, %d, ..., %d] (%d)' % (sizes[0], sizes[1], sizes[-1], len(sizes))


def print_worst(label, worst):
    print('EDGE %s: worst error / bound: %s' % (label, ', '.join('%s %.3e' % (k, worst[k]) for k in ('mode', 'draw', 'target', 'resid', 'gw', 'gp'))
                                                + (', ADAM %.2f ulp' % worst['adam_ulp'] if 'adam_ulp' in worst else '')))
