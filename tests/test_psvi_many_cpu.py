"""The batched BatchPSVI run (include/beta_cores_psvi_many.h, BatchPSVICoreset.build_many) without a GPU: one full step of
csrc/bc_psvi_many_dev.h and its neighbours compiled for the host (tests/psvi_many_harness.cpp) against the long-double
restatement of tests/psvi_many_cases.py on cases of tests/vi_laplace_cases.py and tests/psvi_cases.py, the ADAM stage against
util/opt.py bit for bit, the header against the ctypes table and the library, the refusals made before a device is touched, and
route='each' with a black-box projector."""
import os
import re
import subprocess

import numpy as np
import pytest

import psvi_cases as pc
import psvi_many_cases as pm
import vi_laplace_cases as lc
from beta_cores_amd import _native as N
from beta_cores_amd.coreset import BlackBoxProjector, bpsvi
from beta_cores_amd.device import _ptr
from beta_cores_amd.util import opt

ROOT = pm.ROOT
HEADER = 'beta_cores_psvi_many.h'
NAMES = ['bc_psvi_many_auto_chunk', 'bc_psvi_many_begin', 'bc_psvi_many_chunk_begin', 'bc_psvi_many_chunk_end', 'bc_psvi_many_device_ms',
         'bc_psvi_many_end', 'bc_psvi_many_last_step', 'bc_psvi_many_work_doubles']
_CTYPES = {'bc_ctx*': N.vp, 'const bc_data*': N.vp, 'const double*': N.vp, 'double*': N.vp, 'const int64_t*': N.vp, 'int32_t*': N.vp,
           'int64_t': N.C.c_int64, 'int32_t': N.C.c_int32, 'int': N.C.c_int, 'double': N.C.c_double}


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    return pm.build_harness(tmp_path_factory.mktemp('psvi_many'))


def check_step(label, st, r):
    """stages 2-4 of a harness result against long double, stage 5 against util/opt.py's statements bit for bit"""
    assert r['status'] == 0, label
    pm.check_mode_and_draw(label, st['pts'], st['w'], st['E'], st['diag'], r['mode'], r['theta'], key=st.get('key'))
    pm.check_stage34(label, st['rows'], st['scale'], st['pts'], st['w'], r['theta'], r['target'], r['resid'], r['gw'])
    pm.check_point_grad(label, st['pts'], st['w'], r['theta'], r['resid'], r['gp'])
    m = st['m']
    x0 = np.concatenate((st['w'], st['pts'].ravel()))
    g = np.concatenate((r['gw'], r['gp'].ravel()))
    i = st['step_i']
    x, m1, m2 = pm.adam_step(x0, g, np.concatenate((st['m1w'], st['m1p'].ravel())), np.concatenate((st['m2w'], st['m2p'].ravel())), st['step'], i,
                             np.arange(m))
    for name, got, want in (('x', np.concatenate((r['w'], r['pts'].ravel())), x), ('mom1', np.concatenate((r['m1w'], r['m1p'].ravel())), m1),
                            ('mom2', np.concatenate((r['m2w'], r['m2p'].ravel())), m2)):
        assert np.array_equal(got, want), (label, name)


# ---------------------------------------------------------------- one full step against long double
@pytest.mark.parametrize('d', [1, 3, 16, 33, 128])
@pytest.mark.parametrize('shape', [0, 1, 2])
def test_full_step_on_the_laplace_cases(harness, tmp_path, d, shape):
    m, s = lc.SHAPES[shape]
    for n_sub, diag in ((37, False), (64, True)):
        st = pm.make_step(d, m, s, n_sub, diag=diag, variant=shape + d)      # (the variants of vi_laplace_cases.grid())
        check_step('D %d m %d S %d n_sub %d diag %d' % (d, m, s, n_sub, diag), st, pm.run_step(harness, st, tmp_path))


def test_full_step_at_the_widest_sample_count(harness, tmp_path):
    st = pm.make_step(33, 300, 256, 200, variant=3 + 33)
    check_step('S 256', st, pm.run_step(harness, st, tmp_path))


@pytest.mark.parametrize('d', [3, 33, 128])
@pytest.mark.parametrize('shape', [(7, 5), (130, 100)])
def test_full_step_on_the_point_gradient_cases(harness, tmp_path, d, shape):
    """points of tests/psvi_cases.py (row 0 scaled towards the branch at -z.th >= 100, an exactly zero weight)"""
    c = pc.make_case(pc.LOGISTIC, shape[0], shape[1], d)
    st = pm.psvi_step_case(c)
    r = pm.run_step(harness, st, tmp_path)
    check_step('psvi case D %d' % d, st, r)
    zero = np.where(st['w'] == 0.)[0]
    assert zero.size and np.all(r['gp'][zero] == 0.)           # a zero weight keeps an exactly zero g_p row


# ---------------------------------------------------------------- the ADAM stage is util/opt.py's
def test_adam_restatement_is_partial_nn_opt():
    """tests/psvi_many_cases.adam_step, iterated, gives partial_nn_opt's bits: the statement the harness is held to is the
    library's own loop."""
    rng = np.random.RandomState(5)
    x0, Q = rng.randn(30), rng.randn(30, 30)
    grd = lambda x: Q.dot(np.sin(x))
    sched = lambda i: 0.7 / (1. + i)
    want = opt.partial_nn_opt(x0, grd, np.arange(6), opt_itrs=9, step_sched=sched)
    x, m1, m2 = x0.copy(), np.zeros(30), np.zeros(30)
    for i in range(9):
        x, m1, m2 = pm.adam_step(x, grd(x), m1, m2, sched(i), i, np.arange(6))
    assert np.array_equal(x, want)
    arr = opt.adam_step_arrays(9, sched)
    assert np.array_equal(arr[1], [1. - pm.B1 ** (i + 1) for i in range(9)]) and np.array_equal(arr[2], [1. - pm.B2 ** (i + 1) for i in range(9)])


def test_first_step_equals_one_iteration_of_partial_nn_opt(harness, tmp_path):
    st = pm.make_step(16, 7, 5, 37, step_i=0)
    for k in ('m1w', 'm1p', 'm2w', 'm2p'):
        st[k] = np.zeros_like(st[k])
    r = pm.run_step(harness, st, tmp_path)
    g = np.concatenate((r['gw'], r['gp'].ravel()))
    want = opt.partial_nn_opt(np.concatenate((st['w'], st['pts'].ravel())), lambda x: g, np.arange(7), opt_itrs=1, step_sched=lambda i: 1. / (1. + i))
    assert np.array_equal(np.concatenate((r['w'], r['pts'].ravel())), want)
    assert np.all(r['w'] >= 0.) and np.any(r['pts'] < 0.)      # the projection applies to the weights only


# ---------------------------------------------------------------- marking
def test_a_stage_that_meets_a_non_finite_number_marks_the_problem(harness, tmp_path):
    st = pm.make_step(3, 7, 5, 37)
    bad = dict(st, w=st['w'].copy())
    bad['w'][2] = np.nan
    r = pm.run_step(harness, bad, tmp_path)
    assert r['status'] == 1 and np.all(r['theta'] == 7.) and np.all(r['gw'] == 7.) and np.array_equal(r['pts'], st['pts'])
    bad = dict(st, rows=st['rows'].copy())
    bad['rows'][30, 1] = np.inf
    r = pm.run_step(harness, bad, tmp_path)
    assert r['status'] == 2 and np.all(r['gp'] == 7.) and np.array_equal(r['pts'], st['pts']) and np.array_equal(r['m1w'], st['m1w'])
    bad = dict(st, m2p=st['m2p'].copy())
    bad['m2p'][1, 1] = -1e300                                  # sqrt of a negative moment: the coordinate is NaN after the step
    assert pm.run_step(harness, bad, tmp_path)['status'] == 3


# ---------------------------------------------------------------- the ABI
def prototypes(header):
    src = open(os.path.join(ROOT, 'include', header)).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    protos = {}
    for ret, name, args in re.findall(r'\b(int|int64_t)\s+(bc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', src):
        protos[name] = [re.sub(r'\s*\b[A-Za-z_][A-Za-z0-9_]*$', '', ' '.join(a.split())).strip() for a in args.split(',')]
    return protos


def test_header_and_ctypes_table_agree():
    protos = prototypes(HEADER)
    assert sorted(protos) == N.PSVI_MANY_EXPORTS == NAMES
    others = (N.EXPORTS, N.EXT_EXPORTS, N.F32_EXPORTS, N.NNLS_EXPORTS, N.TAKE_EXPORTS, N.BETAGRAD_EXPORTS, N.ENCODE_EXPORTS, N.VIOPT_EXPORTS,
              N.PSVI_EXPORTS, N.VILAPLACE_EXPORTS, N.HMC_EXPORTS, N.HMC_SMALL_EXPORTS, N.PREFDIAG_EXPORTS, N.SCORE_EXPORTS, N.PREDICT_EXPORTS,
              N.LAPLACE_SMALL_EXPORTS)
    for other in others:
        assert not set(NAMES) & set(other)
    lib = N.load()
    for n, types in protos.items():
        assert hasattr(lib, n), 'libbeta_cores.so does not export %s' % n
        sig = N._PSVI_MANY_SIGNATURES[n]
        want = [_CTYPES[t] for t in types]
        if n == 'bc_psvi_many_device_ms':
            want[1] = N.c_dp                                   # (the one number comes back through byref)
        assert sig == want, n
        assert getattr(lib, n).argtypes == sig                 # bound by load()
    assert lib.bc_psvi_many_work_doubles.restype == N.C.c_int64
    mine = open(os.path.join(ROOT, 'include', HEADER)).read()
    for hdr in os.listdir(os.path.join(ROOT, 'include')):
        if hdr != HEADER:
            assert 'bc_psvi_many' not in open(os.path.join(ROOT, 'include', hdr)).read(), hdr
    for other in others:                                       # and this header spells no entry point of another
        assert not [o for o in other if o in mine]
    assert ' bc_psvi_many.hip ' in open(os.path.join(ROOT, 'beta_cores_amd', 'csrc', 'Makefile')).read()
    assert '_native.PSVI_MANY_EXPORTS' in open(os.path.join(ROOT, '__graft_entry__.py')).read()
    for name, value in (('MAX_SAMPLES', bpsvi.PSVI_MANY_MAX_SAMPLES), ('MAX_SUB', bpsvi.PSVI_MANY_MAX_SUB), ('MAX_PROBLEMS', bpsvi.PSVI_MANY_MAX_PROBLEMS),
                        ('MAX_POINTS', bpsvi.PSVI_MANY_MAX_POINTS)):
        assert re.search(r'#define BC_PSVI_MANY_%s %d\b' % (name, value), mine), name
    assert '#define BC_PSVI_MANY_MAX_WORK_DOUBLES (1ll << 27)' in mine and bpsvi.PSVI_MANY_MAX_WORK_DOUBLES == 1 << 27


def test_library_exports_exactly_the_headers_symbols():
    out = subprocess.run(['nm', '-D', '--defined-only', N.LIB_PATH], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    exported = sorted(set(re.findall(r'\b(bc_psvi_many_[a-z0-9_]+)\b', out.stdout)))
    assert exported == NAMES


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / 'use_psvi_many.c'
    src.write_text('#include "%s"\n'
                   'typedef int (*fn)(void);\n'
                   'fn table[] = {%s};\n' % (HEADER, ', '.join('(fn)%s' % n for n in NAMES)))
    cmd = ['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic-errors', '-I', os.path.join(ROOT, 'include'), '-c', str(src), '-o',
           str(tmp_path / 'use_psvi_many.o')]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


class _Begin:
    """The arguments of a valid bc_psvi_many_begin on two problems (1 and 2 points, S = 2, 3 steps), to be spoilt one at a time.
    Context and data are stand-ins of zero bytes: every refusal tested here is made before either is looked at."""
    ORDER = ('ctx', 'data', 'model', 'kind', 'diag', 'pts', 'w0', 'row_ptr', 'P', 'start', 's', 'itrs', 'steps', 'moments', 'n_sub', 'scale')

    def __init__(self):
        self.ctx, self.data = N.C.create_string_buffer(4096), N.C.create_string_buffer(4096)
        self.pts, self.w = np.ones((3, 3)), np.ones(3)
        self.row_ptr = np.array([0, 1, 3], dtype=np.int64)
        self.steps, self.moments = np.ones((2, 3)), np.ones((2, 3))
        from beta_cores_amd.likelihoods import LogisticRegression
        self.kw = dict(ctx=N.C.cast(self.ctx, N.vp), data=N.C.cast(self.data, N.vp), model=int(LogisticRegression().model_id), kind=2, diag=0,
                       pts=_ptr(self.pts), w0=_ptr(self.w), row_ptr=_ptr(self.row_ptr), P=2, start=None, s=2, itrs=3, steps=_ptr(self.steps),
                       moments=_ptr(self.moments), n_sub=5, scale=2.)

    def refused(self, **spoil):
        kw = dict(self.kw, **spoil)
        rc = N.load().bc_psvi_many_begin(*[kw[k] for k in self.ORDER])
        return rc == N.BC_INVALID_ARGUMENT and b'bc_psvi_many_begin' in N.load().bc_last_error()


def test_entry_points_refuse_null_arguments_and_limits():
    lib = N.load()
    c = _Begin()
    for name in ('ctx', 'data', 'pts', 'w0', 'row_ptr', 'steps', 'moments'):
        assert c.refused(**{name: None}), name
    from beta_cores_amd.likelihoods import LinearRegression
    assert c.refused(model=int(LinearRegression(1.).model_id)) and b'linear-regression' in lib.bc_last_error()
    assert c.refused(kind=0) and c.refused(kind=1) and c.refused(kind=3)
    assert c.refused(diag=2) and c.refused(diag=-1)
    assert c.refused(n_sub=0) and b'all rows every step' in lib.bc_last_error()
    assert c.refused(n_sub=-1) and c.refused(n_sub=bpsvi.PSVI_MANY_MAX_SUB + 1)
    assert c.refused(s=0) and c.refused(s=bpsvi.PSVI_MANY_MAX_SAMPLES + 1)
    assert c.refused(itrs=0) and c.refused(P=0) and c.refused(P=bpsvi.PSVI_MANY_MAX_PROBLEMS + 1)
    assert c.refused(row_ptr=_ptr(np.array([1, 2, 3], dtype=np.int64)))
    assert c.refused(row_ptr=_ptr(np.array([0, 1, 1], dtype=np.int64)))
    assert c.refused(row_ptr=_ptr(np.array([0, 1, 2 + bpsvi.PSVI_MANY_MAX_POINTS], dtype=np.int64)))
    assert c.refused(scale=np.nan) and c.refused(scale=np.inf)
    assert c.refused() and b'another context' in lib.bc_last_error()      # (the stand-in data handle names no context: the last refusal)
    for fn, args in (('bc_psvi_many_chunk_begin', (None, None, None, 1)), ('bc_psvi_many_chunk_end', (None, None)),
                     ('bc_psvi_many_end', (None, None, None, None, None)), ('bc_psvi_many_device_ms', (None, None)),
                     ('bc_psvi_many_last_step', (None, 1, 1, 1, 1) + (None,) * 16)):
        assert getattr(lib, fn)(*args) == N.BC_INVALID_ARGUMENT and fn.encode() in lib.bc_last_error(), fn
    # the work space: the documented closed form, and -1 outside the limits
    R, P, D, S, n_sub, itrs = 5050, 100, 128, 100, 200, 500
    T = (n_sub + 15) // 16
    closed = R * (5 * D + 8 + S) + R // 2 + P * (S * D + D + T * S + 2 * S + itrs + 2) + P // 2 + 2 * itrs + 1
    got = lib.bc_psvi_many_work_doubles(R, P, D, S, n_sub, itrs)
    assert closed <= got <= closed + 24                             # (each of the 23 pieces is rounded up to an even count)
    assert got < bpsvi.PSVI_MANY_MAX_WORK_DOUBLES
    for args in ((0, P, D, S, n_sub, itrs), (R, 0, D, S, n_sub, itrs), (R, P, 129, S, n_sub, itrs), (R, P, D, 257, n_sub, itrs),
                 (R, P, D, S, 0, itrs), (R, P, D, S, n_sub, 0), (R, bpsvi.PSVI_MANY_MAX_PROBLEMS + 1, D, S, n_sub, itrs),
                 (2 * bpsvi.PSVI_MANY_MAX_POINTS + 1, 2, D, S, n_sub, itrs)):
        assert lib.bc_psvi_many_work_doubles(*args) == -1, args
    assert lib.bc_psvi_many_auto_chunk(100, 128, 200) == (32 << 20) // (8 * (100 * 128 + 200))
    assert lib.bc_psvi_many_auto_chunk(0, 1, 1) == 1


# ---------------------------------------------------------------- route='each' with a black-box projector
class _FakeSampler:
    """A sampler as the reference drivers write them: Theta = a function of the weights plus S x D normals of its stream (the
    global one, or an injected RandomState in `_rng`, which is where build_many looks for the sampler's stream)."""

    def __init__(self, D, rng=None):
        self.D, self._rng = D, rng

    def __call__(self, n, wts, pts):
        e = np.random.randn(n, self.D) if self._rng is None else self._rng.randn(n, self.D)
        return e * 0.3 + (0.01 * np.tanh(np.asarray(wts).sum()) if np.asarray(wts).size else 0.)


def _loglik(z, th):
    return -np.logaddexp(0., -np.atleast_2d(z).dot(th.T))


def _grad_loglik(z, th):
    return (1. / (1. + np.exp(np.atleast_2d(z).dot(th.T))))[:, :, None] * th[None]


class _HostPSVI(bpsvi.BatchPSVICoreset):
    """BatchPSVICoreset with a black-box projector on the host; the base class would reduce the N x S projection on the device."""

    def _data_term(self, rows=None, scale=None):
        if rows is None:
            rows, scale = self._rows()
        return scale * self.ll_projector.project(rows).sum(axis=0)


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and tuple(a[2:]) == tuple(b[2:])


def _each_setup(seed, rng=None):
    data = np.random.RandomState(3).randn(80, 4)
    prj = BlackBoxProjector(_FakeSampler(4, rng=rng), 6, _loglik, _grad_loglik)
    alg = _HostPSVI(data, prj, opt_itrs=4, n_subsample_opt=20, pin_data=False)
    np.random.seed(seed)
    return data, alg


@pytest.mark.parametrize('own_rng', [False, True])
def test_route_each_is_the_single_build_from_the_same_state(own_rng):
    sizes = [1, 2, 5, 17]
    rng = np.random.RandomState(11) if own_rng else None
    data, alg = _each_setup(21, rng)
    alg.wts, alg.pts, alg.idcs = np.array([2.]), data[:1].copy(), np.array([0])
    s_np, s_rng = np.random.get_state(), rng.get_state() if own_rng else None
    curve = alg.build_many(sizes, route='each')
    assert curve.route == 'each' and curve.marked == [] and curve.device_ms == 0. and len(curve) == len(sizes)
    assert np.array_equal(alg.wts, [2.]) and np.array_equal(alg.idcs, [0]) and np.array_equal(alg.pts, data[:1])      # left as they were
    end_np = np.random.get_state()
    end_rng = rng.get_state() if own_rng else None
    inits = []
    for m, entry in zip(sizes, curve):
        np.random.set_state(s_np)
        if own_rng:
            rng.set_state(s_rng)
        one = _HostPSVI(data, alg.ll_projector, opt_itrs=4, n_subsample_opt=20, pin_data=False)
        one.build(1, m)
        for got, want in zip(entry, one.get()):
            assert np.array_equal(got, want), m
        inits.append(one.idcs.copy())
        # both streams end where ONE build ends, whatever its size
        assert _same_state(np.random.get_state(), end_np)
        if own_rng:
            assert _same_state(rng.get_state(), end_rng)
    for a, b in zip(inits, inits[1:]):
        assert np.array_equal(a, b[:a.size])                   # the inits are nested


def test_build_many_argument_checks_and_routes():
    data, alg = _each_setup(1)
    with pytest.raises(ValueError):
        alg.build_many([1, 2], route='fast')
    with pytest.raises(ValueError):
        alg.build_many([0, 2])
    with pytest.raises(ValueError):
        alg.build_many([81])
    with pytest.raises(NotImplementedError, match='not a DeviceProjector'):
        alg.build_many([1, 2], route='batched')
    assert alg.build_many([], route='each') == [] and alg.build_many([1, 3]).route == 'each'      # 'auto' takes the loop when not covered
