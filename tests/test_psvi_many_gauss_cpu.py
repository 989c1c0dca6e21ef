"""The Gaussian-location kind of the batched BatchPSVI run (include/beta_cores_psvi_many.h) without a GPU: one full step of
csrc/bc_psvi_many_dev.h and its neighbours compiled for the host (tests/psvi_many_gauss_harness.cpp) against the long-double
restatement and the derived bounds of tests/psvi_many_gauss_cases.py, the row aux against bc_project's expression bit for bit, the
marking, the whole-run restatement against the library's own host loop, and the refusals the new entry makes before a device is
touched."""
import os
import re
import subprocess

import numpy as np
import pytest

import psvi_many_gauss_cases as pg
from beta_cores_amd import _native as N
from beta_cores_amd.coreset import bpsvi
from beta_cores_amd.device import _ptr


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    return pg.build_harness(tmp_path_factory.mktemp('psvi_many_gauss'))


def check_step(label, st, r):
    assert r['status'] == 0, label
    pg.check_quadforms(label + ' rows', st, rows=st['rows'], ra_rows=r['ra_sub'], theta=r['theta'], sa=r['sa'])
    pg.check_quadforms(label + ' points', st, rows=st['pts'], ra_rows=r['ra_pts'])
    pg.check_mean_and_draw(label, st['pts'], st['w'], st['E'], st, r['mode'], r['theta'])
    pg.check_stage34(label, st['rows'], st['scale'], st['pts'], st['w'], r['theta'], st, r['target'], r['resid'], r['gw'])
    pg.check_point_grad(label, st['pts'], st['w'], r['theta'], r['resid'], st, r['gp'])
    m = st['m']
    pg.check_adam(label, np.concatenate((st['w'], st['pts'].ravel())), np.concatenate((r['gw'], r['gp'].ravel())),
                  np.concatenate((st['m1w'], st['m1p'].ravel())), np.concatenate((st['m2w'], st['m2p'].ravel())), st['step'], st['step_i'], m,
                  np.concatenate((r['w'], r['pts'].ravel())), np.concatenate((r['m1w'], r['m1p'].ravel())), np.concatenate((r['m2w'], r['m2p'].ravel())))


@pytest.mark.parametrize('d', [3, 33, 128])
@pytest.mark.parametrize('s', [7, 100])
def test_full_step_against_long_double(harness, tmp_path, d, s):
    """both forms of the posterior stage's three products: bc_pm_post_products (the one the run takes) and bc_vi_sampler's own"""
    for m in (1, 17, 40):
        for n_sub in (37, 64):
            for chains in (False, True):
                st = dict(pg.make_step(d, m, s, n_sub), chains=chains)
                check_step('D %d S %d m %d n_sub %d chains %d' % (d, s, m, n_sub, chains), st, pg.run_step(harness, st, tmp_path))


def test_row_aux_is_the_projections_expression(harness, tmp_path):
    """ra in the statements of bc_project's row quadratic form, (x * (x . Siginv)).sum(): t_a an fma chain over b, the products
    x_a t_a added in ascending a -- restated here with exact fmas (a Fraction rounds to the nearest double once), bit for bit."""
    from fractions import Fraction
    st = pg.make_step(33, 17, 7, 37)
    r = pg.run_step(harness, st, tmp_path)
    Sg = [[Fraction(v) for v in row] for row in st['Siginv']]
    for X, got in ((st['rows'], r['ra_sub']), (st['pts'], r['ra_pts'])):
        for x, g in zip(X, got):
            tot = 0.
            for a in range(33):
                t = 0.
                for b in range(33):
                    t = float(Fraction(x[b]) * Sg[b][a] + Fraction(t))
                tot += x[a] * t
            assert tot == g


def test_a_stage_that_meets_a_non_finite_number_marks_the_problem(harness, tmp_path):
    st = pg.make_step(3, 7, 5, 37)
    bad = dict(st, w=st['w'].copy())
    bad['w'][2] = np.nan
    r = pg.run_step(harness, bad, tmp_path)
    assert r['status'] == 1 and np.all(r['theta'] == 7.) and np.all(r['thp'] == 7.) and np.all(r['gw'] == 7.) and np.array_equal(r['pts'], st['pts'])
    bad = dict(st, w=-st['w'])                                 # A = Sig0inv - (sum w) Siginv is not positive definite: a pivot fails
    assert pg.run_step(harness, bad, tmp_path)['status'] == 1
    bad = dict(st, rows=st['rows'].copy())
    bad['rows'][30, 1] = np.inf
    r = pg.run_step(harness, bad, tmp_path)
    assert r['status'] == 2 and np.all(r['gp'] == 7.) and np.array_equal(r['pts'], st['pts']) and np.array_equal(r['m1w'], st['m1w'])
    bad = dict(st, m2p=st['m2p'].copy())
    bad['m2p'][1, 1] = -1e300
    assert pg.run_step(harness, bad, tmp_path)['status'] == 3


def test_whole_run_restatement_is_the_host_loop():
    """tests/psvi_many_gauss_cases.whole_run_ld against bpsvi.py:47-57 written out in NumPy doubles with LAPACK's posterior
    (oracle-free: the statements of BatchPSVICoreset._gradient and util/opt.py): the same k steps agree to rounding."""
    from beta_cores_amd.util import opt
    d, m, S, n_sub, k = 5, 4, 7, 19, 4
    mdl = pg.make_model(d)
    rng = np.random.RandomState(3)
    data = pg.make_rows(rng, 80, d)
    E, idx = rng.randn(k, S, d), rng.randint(80, size=(k, n_sub))
    pts0, w0 = data[:m].copy(), np.full(m, 80. / m)
    Si, S0, mu0, c0 = mdl['Siginv'], mdl['Sig0inv'], mdl['mu0'], pg.model_constant(mdl)
    it = [0]

    def grad(x):
        i = it[0]
        it[0] += 1
        w, p = x[:m], x[m:].reshape(m, d)
        A = S0 + w.sum() * Si
        Li = np.linalg.inv(np.linalg.cholesky(A))
        mu = Li.dot(Li.T).dot(S0.dot(mu0) + Si.dot((w[:, None] * p).sum(axis=0)))
        th = mu + E[i].dot(Li.T)

        def centred(X):
            diff = X[:, None, :] - th[None, :, :]
            ll = c0 - 0.5 * (diff * diff.dot(Si)).sum(axis=2)
            return ll - ll.mean(axis=1)[:, None]
        target = 80. / n_sub * centred(data[idx[i]]).sum(axis=0)
        cv = centred(p)
        resid = target - w.dot(cv)
        G = th.dot(Si)[None] - p.dot(Si)[:, None]
        G = G - G.mean(axis=2)[:, :, None]
        return np.concatenate((-cv.dot(resid) / S, (-(w[:, None, None] * G * resid[None, :, None]).sum(axis=1) / S).ravel()))
    sched = lambda i: 1. / (1. + i)
    want = opt.partial_nn_opt(np.concatenate((w0, pts0.ravel())), grad, np.arange(m), opt_itrs=k, step_sched=sched)
    w, p, closest = pg.whole_run_ld(data, pts0, w0, mdl, E, idx, [sched(i) for i in range(k)], 80.)
    assert closest > 1.
    assert np.abs(np.concatenate((w, p.ravel())) - want).max() <= 1e-10 * (1. + np.abs(want).max())


# ---------------------------------------------------------------- the new entries, before a device is touched
class _BeginKind:
    """The arguments of a bc_psvi_curve_begin on two problems of the Gaussian kind, D = 3, to be spoilt one at a time.  Context
    and data are stand-ins of zero bytes: every refusal tested here is made before either is looked at."""
    ORDER = ('ctx', 'data', 'model', 'kind', 'diag', 'pts', 'w0', 'row_ptr', 'P', 'start', 's', 'itrs', 'steps', 'moments', 'n_sub', 'scale',
             'mp', 'n_mp', 'sp', 'n_sp')

    def __init__(self):
        from beta_cores_amd.likelihoods import GaussianLocation
        self.ctx, self.data = N.C.create_string_buffer(4096), N.C.create_string_buffer(4096)
        self.pts, self.w = np.ones((3, 3)), np.ones(3)
        self.row_ptr = np.array([0, 1, 3], dtype=np.int64)
        self.steps, self.moments = np.ones((2, 3)), np.ones((2, 3))
        self.mp, self.sp, self.start = np.concatenate(([0.], np.eye(3).ravel())), np.concatenate((np.zeros(3), np.eye(3).ravel(), np.eye(3).ravel())), np.zeros((2, 3))
        self.kw = dict(ctx=N.C.cast(self.ctx, N.vp), data=N.C.cast(self.data, N.vp), model=int(GaussianLocation(np.eye(3), 0.).model_id), kind=1, diag=0,
                       pts=_ptr(self.pts), w0=_ptr(self.w), row_ptr=_ptr(self.row_ptr), P=2, start=None, s=2, itrs=3, steps=_ptr(self.steps),
                       moments=_ptr(self.moments), n_sub=5, scale=2., mp=_ptr(self.mp), n_mp=10, sp=_ptr(self.sp), n_sp=21)

    def refused(self, **spoil):
        kw = dict(self.kw, **spoil)
        rc = N.load().bc_psvi_curve_begin(*[kw[k] for k in self.ORDER])
        return rc == N.BC_INVALID_ARGUMENT and b'bc_psvi_curve_begin' in N.load().bc_last_error()


def test_begin_kind_refuses_before_a_device_is_touched():
    lib = N.load()
    c = _BeginKind()
    assert c.refused(diag=1) and b'diag must be 0' in lib.bc_last_error()
    assert c.refused(start=_ptr(c.start)) and b'start must be NULL' in lib.bc_last_error()
    assert c.refused(mp=None) and c.refused(sp=None)
    from beta_cores_amd.likelihoods import LinearRegression, LogisticRegression
    assert c.refused(model=int(LinearRegression(1.).model_id)) and b'linear-regression' in lib.bc_last_error()
    assert c.refused(kind=0) and c.refused(kind=2) and c.refused(kind=3)                  # the Gaussian model with another sampler
    assert c.refused(model=int(LogisticRegression().model_id)) and c.refused(model=int(LogisticRegression().model_id), kind=2)      # (parameters given)
    assert c.refused(n_sub=0) and c.refused(s=257) and c.refused(itrs=0) and c.refused(P=0)
    assert c.refused() and b'another context' in lib.bc_last_error()      # (the stand-in data handle names no context: the last refusal)
    # the old entry has no parameters to give this kind
    kw = c.kw
    rc = lib.bc_psvi_many_begin(*[kw[k] for k in c.ORDER[:16]])
    assert rc == N.BC_INVALID_ARGUMENT and b'bc_psvi_curve_begin' in lib.bc_last_error()


def test_work_space_counts():
    lib = N.load()
    R, P, D, S, n_sub, itrs = 20100, 200, 100, 200, 200, 1000      # the reference driver's shape: sizes 1 .. 200
    T = (n_sub + 15) // 16
    closed = R * (5 * D + 8 + S) + R // 2 + P * (S * D + D + T * S + 2 * S + itrs + 2) + P // 2 + 2 * itrs + 1
    logistic = lib.bc_psvi_many_work_doubles(R, P, D, S, n_sub, itrs)
    assert closed <= logistic <= closed + 24 and lib.bc_psvi_curve_work_doubles(R, P, D, S, n_sub, itrs, 2) == logistic
    gauss = lib.bc_psvi_curve_work_doubles(R, P, D, S, n_sub, itrs, 1)
    extra = P * (S * D + S) + n_sub + R
    assert logistic + extra <= gauss <= logistic + extra + 4        # (four more pieces, each rounded up to an even count)
    assert gauss < bpsvi.PSVI_MANY_MAX_WORK_DOUBLES
    for R2, P2, S2, n2 in ((5, 3, 7, 37), (65, 5, 7, 37), (66, 5, 100, 64)):      # odd counts: the rounding rule
        lg, ga = lib.bc_psvi_many_work_doubles(R2, P2, 3, S2, n2, 2), lib.bc_psvi_curve_work_doubles(R2, P2, 3, S2, n2, 2, 1)
        ex = P2 * (S2 * 3 + S2) + n2 + R2
        assert lg + ex <= ga <= lg + ex + 4
    for kind in (0, 3, -1):
        assert lib.bc_psvi_curve_work_doubles(R, P, D, S, n_sub, itrs, kind) == -1
    assert lib.bc_psvi_curve_work_doubles(R, P, 129, S, n_sub, itrs, 1) == -1 and lib.bc_psvi_curve_work_doubles(R, P, D, 257, n_sub, itrs, 1) == -1


# ---------------------------------------------------------------- the ABI of include/beta_cores_psvi_curve.h
HEADER = 'beta_cores_psvi_curve.h'
NAMES = ['bc_psvi_curve_begin', 'bc_psvi_curve_work_doubles']
_CTYPES = {'bc_ctx*': N.vp, 'const bc_data*': N.vp, 'const double*': N.vp, 'const int64_t*': N.vp, 'int64_t': N.C.c_int64, 'int32_t': N.C.c_int32,
           'int': N.C.c_int, 'double': N.C.c_double}


def test_header_ctypes_table_and_library_agree(tmp_path):
    src = open(os.path.join(pg.ROOT, 'include', HEADER)).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    protos = {}
    for ret, name, args in re.findall(r'\b(int|int64_t)\s+(bc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', code):
        protos[name] = [re.sub(r'\s*\b[A-Za-z_][A-Za-z0-9_]*$', '', ' '.join(a.split())).strip() for a in args.split(',')]
    assert sorted(protos) == N.PSVI_CURVE_EXPORTS == NAMES
    lib = N.load()
    for n, types in protos.items():
        assert N._PSVI_CURVE_SIGNATURES[n] == [_CTYPES[t] for t in types], n
        assert getattr(lib, n).argtypes == N._PSVI_CURVE_SIGNATURES[n]      # bound by load()
    assert lib.bc_psvi_curve_work_doubles.restype == N.C.c_int64
    every = [n for k in dir(N) if k.endswith('EXPORTS') and k != 'PSVI_CURVE_EXPORTS' for n in getattr(N, k)]
    assert not [o for o in every if o in src]                  # this header spells no entry point of another ...
    for hdr in os.listdir(os.path.join(pg.ROOT, 'include')):
        if hdr != HEADER:
            assert 'bc_psvi_curve' not in re.sub(r'/\*.*?\*/', '', open(os.path.join(pg.ROOT, 'include', hdr)).read(), flags=re.S), hdr      # ... and none declares its
    out = subprocess.run(['nm', '-D', '--defined-only', N.LIB_PATH], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert sorted(set(re.findall(r'\b(bc_psvi_curve_[a-z0-9_]+)\b', out.stdout))) == NAMES
    assert '_native.PSVI_CURVE_EXPORTS' in open(os.path.join(pg.ROOT, '__graft_entry__.py')).read()
    use = tmp_path / 'use_psvi_curve.c'
    use.write_text('#include "%s"\ntypedef int (*fn)(void);\nfn table[] = {%s};\n' % (HEADER, ', '.join('(fn)%s' % n for n in NAMES)))
    cc = subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic-errors', '-I', os.path.join(pg.ROOT, 'include'), '-c', str(use), '-o',
                         str(tmp_path / 'use_psvi_curve.o')], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
