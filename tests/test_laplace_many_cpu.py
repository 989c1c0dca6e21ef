"""The batched Laplace fit of many small logistic posteriors (include/beta_cores_laplace_small.h, samplers.logistic_laplace_many)
without a GPU: the header's prototypes against the ctypes table, the refusals that are made before a device is touched, the
four stages of csrc/bc_vi_laplace_dev.h compiled for the host and run over packed batches (tests/laplace_many_harness.cpp)
against the formulas in long double, where the factor bounds' constants come from, and the Python argument checks."""
import os
import re
import subprocess

import numpy as np
import pytest

import laplace_many_cases as lm
import vi_laplace_cases as lc
import vi_sampler_cases as vc
from beta_cores_amd import _native as N
from beta_cores_amd import samplers
from beta_cores_amd.device import _ptr

ROOT = lm.ROOT
HEADER = 'beta_cores_laplace_small.h'
NAMES = ['bc_laplace_small', 'bc_laplace_small_device_ms']
_CTYPES = {'bc_ctx*': N.vp, 'const bc_data*': N.vp, 'const double*': N.vp, 'double*': N.vp, 'const int64_t*': N.vp, 'int32_t*': N.vp,
           'int64_t': N.C.c_int64, 'int32_t': N.C.c_int32}


def prototypes(header):
    src = open(os.path.join(ROOT, 'include', header)).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    protos = {}
    for name, args in re.findall(r'\bint\s+(bc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', src):
        protos[name] = [re.sub(r'\s*\b[A-Za-z_][A-Za-z0-9_]*$', '', ' '.join(a.split())).strip() for a in args.split(',')]
    return protos


# ---------------------------------------------------------------- the ABI
def test_header_and_ctypes_table_agree():
    protos = prototypes(HEADER)
    assert sorted(protos) == N.LAPLACE_SMALL_EXPORTS == NAMES
    others = (N.EXPORTS, N.EXT_EXPORTS, N.F32_EXPORTS, N.NNLS_EXPORTS, N.TAKE_EXPORTS, N.BETAGRAD_EXPORTS, N.ENCODE_EXPORTS, N.VIOPT_EXPORTS,
              N.PSVI_EXPORTS, N.VILAPLACE_EXPORTS, N.HMC_EXPORTS, N.HMC_SMALL_EXPORTS, N.PREFDIAG_EXPORTS, N.SCORE_EXPORTS, N.PREDICT_EXPORTS)
    for other in others:
        assert not set(NAMES) & set(other)
        assert not [o for o in other for n in NAMES if n in o or o in n]      # no name is a part of another header's
    lib = N.load()
    for n, types in protos.items():
        assert hasattr(lib, n), 'libbeta_cores.so does not export %s' % n
        sig = N._LAPLACE_SMALL_SIGNATURES[n]
        want = [_CTYPES[t] for t in types]
        if n == 'bc_laplace_small_device_ms':
            want[1] = N.c_dp                                   # (the one number comes back through byref)
        assert sig == want, n
        assert getattr(lib, n).argtypes == sig                 # bound by load()
    mine = open(os.path.join(ROOT, 'include', HEADER)).read()
    for hdr in os.listdir(os.path.join(ROOT, 'include')):
        if hdr != HEADER:
            src = open(os.path.join(ROOT, 'include', hdr)).read()
            assert not [n for n in NAMES if n in src], hdr
    for other in others:                                       # and this header spells no entry point of another
        assert not [o for o in other if o in mine]
    makefile = open(os.path.join(ROOT, 'beta_cores_amd', 'csrc', 'Makefile')).read()
    assert ' bc_laplace_small.hip ' in makefile
    entry = open(os.path.join(ROOT, '__graft_entry__.py')).read()
    assert '_native.LAPLACE_SMALL_EXPORTS' in entry
    assert 'BC_LAPLACE_SMALL_MAX_DIM 128' in mine and 'BC_LAPLACE_SMALL_MAX_DRAWS 256' in mine
    assert (samplers.LAPLACE_SMALL_MAX_DIM, samplers.LAPLACE_SMALL_MAX_DRAWS) == (128, 256)


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / 'use_laplace_small.c'
    src.write_text('#include "%s"\n'
                   'typedef int (*fn)(void);\n'
                   'fn table[] = {%s};\n' % (HEADER, ', '.join('(fn)%s' % n for n in NAMES)))
    cmd = ['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic-errors', '-I', os.path.join(ROOT, 'include'), '-c', str(src), '-o',
           str(tmp_path / 'use_laplace_small.o')]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


class _Call:
    """The arguments of a valid call on two problems (1 and 2 rows, D = 3, S = 2), to be spoilt one at a time.  The context is a
    stand-in of zero bytes: every refusal tested here is made before the context is looked at."""

    def __init__(self):
        self.ctx = N.C.create_string_buffer(4096)
        self.rows, self.w = np.ones((3, 3)), np.ones(3)
        self.row_ptr = np.array([0, 1, 3], dtype=np.int64)
        self.E = np.ones((2, 3))
        self.mu, self.hd, self.val = np.full((2, 3), 7.), np.full((2, 3), 7.), np.full(2, 7.)
        self.cnt, self.st = np.full((2, 3), 7, dtype=np.int32), np.full(2, 7, dtype=np.int32)
        self.chol, self.inv, self.th = np.full((2, 3, 3), 7.), np.full((2, 3, 3), 7.), np.full((2, 2, 3), 7.)
        self.kw = dict(ctx=N.C.cast(self.ctx, N.vp), rows=_ptr(self.rows), w=_ptr(self.w), row_ptr=_ptr(self.row_ptr), P=2, d=3, start=None,
                       diag=0, normals=_ptr(self.E), stride=0, s=2, zt=None, yt=None, mu=_ptr(self.mu), hd=_ptr(self.hd), val=_ptr(self.val),
                       cnt=_ptr(self.cnt), st=_ptr(self.st), chol=_ptr(self.chol), inv=_ptr(self.inv), th=_ptr(self.th), cor=None, ll=None)

    def refused(self, **spoil):
        kw = dict(self.kw, **spoil)
        rc = N.load().bc_laplace_small(*[kw[k] for k in ('ctx', 'rows', 'w', 'row_ptr', 'P', 'd', 'start', 'diag', 'normals', 'stride', 's', 'zt',
                                                          'yt', 'mu', 'hd', 'val', 'cnt', 'st', 'chol', 'inv', 'th', 'cor', 'll')])
        untouched = all(np.all(a == 7) for a in (self.mu, self.hd, self.val, self.cnt, self.st, self.chol, self.inv, self.th))
        return rc == N.BC_INVALID_ARGUMENT and untouched and b'bc_laplace_small' in N.load().bc_last_error()


def test_entry_point_refuses_null_arguments():
    lib = N.load()
    assert lib.bc_laplace_small(*([None] * 4 + [0, 0, None, 0, None, 0, 0] + [None] * 12)) == N.BC_INVALID_ARGUMENT
    assert b'bc_laplace_small' in lib.bc_last_error()
    assert lib.bc_laplace_small_device_ms(None, None) == N.BC_INVALID_ARGUMENT
    assert b'bc_laplace_small_device_ms' in lib.bc_last_error()
    c = _Call()
    for name in ('ctx', 'rows', 'w', 'row_ptr', 'mu', 'hd', 'val', 'cnt', 'st'):
        assert c.refused(**{name: None}), name


def test_entry_point_refuses_what_is_outside_the_limits():
    c = _Call()
    big = np.ones((3, 129))
    assert c.refused(d=129, rows=_ptr(big))
    assert c.refused(d=0)
    assert c.refused(P=0)
    assert c.refused(s=257)
    assert c.refused(s=-1)
    assert c.refused(diag=2)
    assert c.refused(normals=None)                       # s = 2 without normals
    assert c.refused(s=0)                                # normals without draws
    assert c.refused(stride=5)                           # 0 < stride < s D
    assert c.refused(stride=-6)
    assert c.refused(row_ptr=_ptr(np.array([0, 2, 2], dtype=np.int64)))
    assert c.refused(row_ptr=_ptr(np.array([1, 2, 3], dtype=np.int64)))
    assert c.refused(chol=None)                          # out_inv without out_chol
    assert c.refused(inv=None)
    assert c.refused(diag=1)                             # factors with the diagonal form
    cor, ll = np.zeros((2, 2), dtype=np.int32), np.zeros((2, 2))
    assert c.refused(cor=_ptr(cor), ll=_ptr(ll))         # scores without held-out data
    assert c.refused(zt=N.C.cast(c.ctx, N.vp))           # zt without yt
    assert c.refused(yt=N.C.cast(c.ctx, N.vp))


# ---------------------------------------------------------------- the host build of the four stages over packed batches
@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    return lm.build_harness(tmp_path_factory.mktemp('laplace_many'))


def test_long_double_is_wider_than_double():
    assert vc.LD_OK


def test_host_newton_sets_the_factor_constants():
    """Where K_H, K_C, K_L come from: samplers.logistic_laplace(solver='newton') on host arrays -- the existing host code, not
    the code under test -- against the long-double factors around its own mode over lc.grid() + lc.extra_cases().  Each
    constant is 16 x the measured worst ratio rounded up to a power of two (lm.HOST_WORST records the ratios)."""
    worst = {'H': 0., 'C': 0., 'L': 0.}
    for c in lc.grid() + lc.extra_cases():
        keep = c['w'] > 0
        mu, LSig, LSigInv = samplers.logistic_laplace(c['w'], c['Z'], np.zeros(c['d']), solver='newton')
        Zw, ww = c['Z'][keep], c['w'][keep]
        p = 0.5 * (1. + np.tanh(0.5 * -Zw.dot(mu)))
        H = np.eye(c['d']) + (Zw * (ww * p * (1. - p))[:, np.newaxis]).T.dot(Zw)      # the host's expression (samplers.logistic_laplace)
        r = lm.factor_ratios(c, mu, H=H, C=LSigInv, L=LSig)
        worst = {k: max(worst[k], r[k]) for k in worst}
    print('worst ratios of the host fit at K = 1: H %.4g, C %.4g, L %.4g (K_H = %g, K_C = %g, K_L = %g)'
          % (worst['H'], worst['C'], worst['L'], lm.K_H, lm.K_C, lm.K_L))
    assert (lm.K_H, lm.K_C, lm.K_L) == tuple(lm.constant_of(worst[k]) for k in ('H', 'C', 'L'))
    assert (lm.K_H, lm.K_C, lm.K_L) == tuple(lm.constant_of(r) for r in lm.HOST_WORST)


def check_batch(cases, outs, diag, label):
    worst = {}
    for c, r in zip(cases, outs):
        assert r['status'] == 0
        assert 1 <= r['counts'][0] <= 200 and 0 <= r['counts'][1] <= 34 and r['counts'][1] <= r['counts'][2]
        rm, rd = lc.check_mode_and_draw(c, r['mu'], r['draws'], label)
        rf = lm.check_factors(c, r['mu'], r['hdiag'], r['chol'], r['inv'], label)
        if not diag:
            assert np.all(np.triu(r['chol'], 1) == 0.) and np.all(np.triu(r['inv'], 1) == 0.)
        for k, v in dict(rf, mode=rm, draw=rd).items():
            worst[k] = max(worst.get(k, 0.), v)
    return worst


@pytest.mark.parametrize('d', [1, 2, 3, 16, 33, 128])
def test_batches_match_the_long_double_reference(harness, tmp_path, d):
    """A packed batch per D through the split functions: every problem's mode and draw within lc.mode_bound / vc.draw_bound, its
    hdiag, C and C^-1 within the three factor bounds."""
    E = np.random.RandomState(500 + d).randn(5, d)
    cases = [lm.with_normals(c, E) for c in lm.cases_of_dim(d)]
    worst = check_batch(cases, lm.run_harness(harness, cases, E, tmp_path), False, 'host build')
    print('worst error / bound at D = %d: %s' % (d, ', '.join('%s %.3g' % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize('d', [3, 128])
def test_diagonal_batches_match_the_long_double_reference(harness, tmp_path, d):
    rng = np.random.RandomState(600 + d)
    base = lm.cases_of_dim(d)
    E = rng.randn(len(base), 5, d)                       # (its own normals per problem)
    cases = [lm.with_normals(c, E[p], diag=True) for p, c in enumerate(base)]
    outs = lm.run_harness(harness, cases, E, tmp_path, diag=True)
    check_batch(cases, outs, True, 'host build, diag')
    for c, r in zip(cases, outs):
        assert np.array_equal(r['draws'], r['mu'] + c['E'] / np.sqrt(r['hdiag']))


def test_a_problem_is_fitted_as_it_is_alone_and_a_refused_one_writes_nothing(harness, tmp_path):
    d = 16
    E = np.random.RandomState(7).randn(3, d)
    cases = [lm.with_normals(c, E) for c in lm.cases_of_dim(d)]
    batch = lm.run_harness(harness, cases, E, tmp_path)
    for p in (0, 3):
        alone = lm.run_harness(harness, cases[p:p + 1], E, tmp_path)[0]
        for k in ('mu', 'value', 'hdiag', 'chol', 'inv', 'counts', 'draws'):
            assert np.array_equal(alone[k], batch[p][k]), (p, k)
    bad = [dict(c) for c in cases]
    bad[2]['w'] = bad[2]['w'].copy()
    bad[2]['w'][5] = np.nan
    bad[4]['start'] = np.full(d, np.inf)
    outs = lm.run_harness(harness, bad, E, tmp_path)
    for p, (r, ok) in enumerate(zip(outs, batch)):
        if p in (2, 4):
            assert r['status'] == 1 and r['untouched']
        else:
            for k in ('mu', 'value', 'hdiag', 'chol', 'inv', 'counts', 'draws'):
                assert np.array_equal(r[k], ok[k]), (p, k)


def test_the_prior_comes_back_exactly(harness, tmp_path):
    """All weights 0 (and the empty coreset's one zero row), start 0: mu = 0, H = C = C^-1 = I, the draws are the normals, no
    Newton step is taken."""
    d = 5
    E = np.random.RandomState(8).randn(4, d)
    c0 = lc.make_case(d, 7, 4)
    c0['w'] = np.zeros(7)
    c1 = dict(c0, Z=np.zeros((1, d)), w=np.zeros(1), m=1)
    for r in lm.run_harness(harness, [c0, c1], E, tmp_path):
        assert r['status'] == 0 and np.all(r['mu'] == 0.) and np.all(r['hdiag'] == 1.) and r['counts'][0] == 0
        assert np.array_equal(r['chol'], np.eye(d)) and np.array_equal(r['inv'], np.eye(d)) and np.array_equal(r['draws'], E)
        assert abs(r['value'] + 0.5 * d * np.log(2. * np.pi)) <= np.spacing(0.5 * d * np.log(2. * np.pi))


# ---------------------------------------------------------------- the Python argument checks that need no device
def test_python_argument_checks():
    f = samplers.logistic_laplace_many
    Z = np.ones((4, 3))
    with pytest.raises(ValueError, match='keep_draws=False needs score'):
        f([(Z, None)], n_draws=2, keep_draws=False)
    with pytest.raises(ValueError, match="'shared' or 'independent'"):
        f([(Z, None)], draws='common')
    with pytest.raises(ValueError, match='at least one problem'):
        f([])
    with pytest.raises(ValueError, match='n x D'):
        f([(np.ones(3), None)])
    with pytest.raises(ValueError, match='columns'):
        f([(Z, None), (np.ones((2, 4)), None)])
    with pytest.raises(ValueError, match='one weight per row'):
        f([(Z, np.ones(3))])
    with pytest.raises(ValueError, match='128.*logistic_laplace has no such limit'):
        f([(np.ones((2, 129)), None)])
    with pytest.raises(ValueError, match='n_draws'):
        f([(Z, None)], n_draws=257)
    with pytest.raises(ValueError, match='n_draws'):
        f([(Z, None)], n_draws=-1)
    with pytest.raises(ValueError, match='mu0'):
        f([(Z, None), (Z, None)], mu0=np.zeros((3, 3)))
    with pytest.raises(ValueError, match='mu0'):
        f([(Z, None)], mu0=np.zeros(4))
    with pytest.raises(ValueError, match="'each' or 'batched'"):
        samplers.logistic_hmc_many([(Z, None)], laplace='all')
