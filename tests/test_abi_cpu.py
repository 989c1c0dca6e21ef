"""CPU-side checks of the boundary: the shared library loads without a GPU and exports every
symbol include/beta_cores.h declares; the product path fails loudly (no CPU fallback) when no
gfx950 device is present; host-only logic (ADAM optimiser, solver host loop, error protocol)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def header_functions():
    src = open(os.path.join(ROOT, 'include', 'beta_cores.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(bc_[a-z0-9_]+)\s*\(', src)))


def have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_library_exports_every_declared_symbol():
    from beta_cores_amd import _native
    lib = _native.load()
    names = header_functions()
    assert len(names) >= 45
    for n in names:
        assert hasattr(lib, n), 'libbeta_cores.so does not export %s' % n
    assert set(names) == set(_native.EXPORTS), set(names) ^ set(_native.EXPORTS)   # the ctypes table binds exactly the header
    assert lib.bc_version() >= 100
    assert isinstance(_native.last_error(), str)


def test_no_oracle_import_in_product():
    """The oracle is test infrastructure: nothing under beta_cores_amd/ may reference it."""
    for dirpath, _, files in os.walk(os.path.join(ROOT, 'beta_cores_amd')):
        for f in files:
            if f.endswith('.py'):
                txt = open(os.path.join(dirpath, f)).read()
                assert not re.search(r'^\s*(from|import)\s+oracle\b', txt, flags=re.M), os.path.join(dirpath, f)
                assert 'fake_engine' not in txt


def test_prefdiag_test_aids_live_in_their_own_unit():
    """The solver's kernels and host side know nothing of the diagnostic seam; bc_snnls_diag.hip defines exactly its entries."""
    csrc = os.path.join(ROOT, 'beta_cores_amd', 'csrc')
    for f in ('bc_snnls.hip', 'bc_snnls_dev.h'):
        assert 'prefdiag' not in open(os.path.join(csrc, f)).read(), f
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'beta_cores_prefdiag.h')).read(), flags=re.S)
    declared = sorted(re.findall(r'\b(bc_snnls_prefdiag_[a-z0-9_]+)\s*\(', hdr))
    assert len(declared) == 3 and len(set(declared)) == 3, declared
    diag = open(os.path.join(csrc, 'bc_snnls_diag.hip')).read()
    defined = sorted(re.findall(r'^extern "C" int (bc_snnls_prefdiag_[a-z0-9_]+)\s*\(', diag, flags=re.M))
    assert defined == declared, (defined, declared)
    assert diag.count('extern "C"') == 3          # ... and no other entry point
    srcs = re.search(r'^SRCS\s*=\s*(.*)$', open(os.path.join(csrc, 'Makefile')).read(), flags=re.M).group(1).split()
    assert 'bc_snnls_diag.hip' in srcs and 'bc_snnls.hip' in srcs, srcs


@pytest.mark.skipif(have_gpu(), reason='checks the no-GPU failure mode')
def test_product_path_fails_loudly_without_gpu():
    import beta_cores_amd as bc
    phi = np.random.RandomState(0).randn(50, 4)
    with pytest.raises((RuntimeError, ValueError)):
        bc.Context(0)
    with pytest.raises((RuntimeError, ValueError)):
        bc.snnls.GIGA(phi.T, phi.sum(axis=0))
    with pytest.raises((RuntimeError, ValueError)):
        bc.DeviceProjector(lambda n, w, p: np.zeros((4, 3)), 4, bc.likelihoods.LinearRegression(1.0))
    prj = bc.BlackBoxProjector(lambda n, w, p: np.zeros((4, 3)), 4, lambda z, t: np.zeros((z.shape[0], 4)) + np.arange(4.))
    with pytest.raises((RuntimeError, ValueError)):
        bc.HilbertCoreset(np.zeros((10, 4)), prj)


def test_status_translation():
    from beta_cores_amd import _native
    import beta_cores_amd as bc
    _native.check(0)
    with pytest.raises(bc.NumericalPrecisionError):
        _native.check(1)
    with pytest.raises(ValueError):
        _native.check(2)
    with pytest.raises(RuntimeError):
        _native.check(-1003)
    # argument validation happens before any HIP call: NULL handles are rejected, not dereferenced
    lib = _native.load()
    assert lib.bc_ctx_sync(None) == 2
    assert lib.bc_phi_colsum(None, None) == 2
    assert lib.bc_snnls_build(None, 3, None) == 2
    # native exchange: validated before RCCL or the device is touched
    import ctypes as C
    buf = (C.c_ubyte * 128)()
    assert lib.bc_comm_unique_id(None, 128) == 2 and lib.bc_comm_unique_id(C.cast(buf, C.c_void_p), 64) == 2
    h = C.c_void_p()
    assert lib.bc_comm_create(None, C.cast(buf, C.c_void_p), 0, 1, C.byref(h)) == 2
    assert lib.bc_comm_selftest(None) == 2 and lib.bc_comm_all_gather(None, None, None, 4) == 2
    assert lib.bc_snnls_bind_comm(None, None) == 2 and lib.bc_comm_destroy(None) == 0


def test_nn_opt_matches_reference_bits():
    import beta_cores_amd as bc
    g = load_golden('f7_nn_opt')
    Q, c, x0 = g['Q'], g['c'], g['x0']
    grd = lambda x: Q.dot(x) - c
    assert np.array_equal(bc.util.nn_opt(x0, grd, opt_itrs=50, step_sched=lambda i: 0.5 / (1. + i)), g['nn'])
    assert np.array_equal(bc.util.opt.partial_nn_opt(x0, grd, np.arange(0, 12, 2), opt_itrs=50,
                                                     step_sched=lambda i: 0.5 / (1. + i)), g['pnn'])
    assert np.array_equal(x0, g['x0'])                                 # input untouched


def test_util_surface():
    import beta_cores_amd as bc
    assert bc.util.TOL == 1e-12
    bc.util.set_tolerance(1e-9)
    assert bc.util.TOL == 1e-9
    bc.util.set_tolerance(1e-12)
    bc.util.set_verbosity('error')
    for name in ('HilbertCoreset', 'SparseVICoreset', 'BetaCoreset', 'BlackBoxProjector', 'Projector',
                 'BetaBlackBoxProjector'):
        assert hasattr(bc, name)                                       # bayesiancoresets/__init__.py:1 (in-scope names)
    for name in ('FrankWolfe', 'ImportanceSampling', 'UniformSampling', 'GIGA', 'OrthoPursuit'):
        assert hasattr(bc.snnls, name)                                 # snnls/__init__.py:1-4


# ------------------------------------------------------------------ solver host loop on a NumPy engine (no GPU)
F1 = load_golden('f1_snnls')


@pytest.mark.parametrize('case', [c for c in F1['cases'] if c.startswith('gauss_N')])
@pytest.mark.parametrize('alg', ['giga', 'fw'])
@pytest.mark.parametrize('fused', [True, False])
def test_host_loop_with_numpy_engine_reproduces_goldens(case, alg, fused):
    """snnls.py:31-79 restated in SparseNNLS.build_stepwise (guard, revert, retry-once) and the
    engine contract, exercised without a GPU through the injected NumPy engine."""
    import beta_cores_amd as bc
    from fake_engine import NumpyShardEngine
    X = F1[case + '_X']
    Wg, eg, lg = F1['%s_%s_W' % (case, alg)], F1['%s_%s_err' % (case, alg)], F1['%s_%s_lim' % (case, alg)]
    cls = bc.snnls.GIGA if alg == 'giga' else bc.snnls.FrankWolfe
    s = cls(X.T, X.sum(axis=0), engine=NumpyShardEngine(X, X.sum(axis=0), alg, 0, None))
    scale = np.sqrt((X.sum(axis=0) ** 2).sum())
    for m in range(Wg.shape[0]):
        if fused:
            s.build(1)
        elif not s.reached_numeric_limit:
            s.build_stepwise(1)
        if eg[m] < 1e-9 * scale or lg[m]:
            break
        np.testing.assert_allclose(s.weights(), Wg[m], rtol=1e-9, atol=1e-14)
        np.testing.assert_allclose(s.error(), eg[m], rtol=1e-7, atol=1e-12)


def test_host_loop_retry_protocol():
    """A step that fails twice in a row inside one build() call sets reached_numeric_limit
    (snnls.py:63-72); with itrs=1 per call it never does (the flag is per call, snnls.py:40)."""
    import beta_cores_amd as bc
    from fake_engine import NumpyShardEngine

    class AlwaysFails(bc.snnls.GIGA):
        def _reweight(self, f):
            raise bc.NumericalPrecisionError('forced')
    X = np.random.RandomState(0).randn(30, 4)
    mk = lambda: AlwaysFails(X.T, X.sum(axis=0), engine=NumpyShardEngine(X, X.sum(axis=0), 'giga', 0, None))
    s = mk()
    assert not s._use_fused()                                          # overridden hook -> host loop
    for _ in range(5):
        s.build(1)
    assert not s.reached_numeric_limit and s.size() == 0
    s = mk()
    s.build(5)
    assert s.reached_numeric_limit
    s.build(5)                                                         # returns immediately (snnls.py:32-34)
    s.reset()
    assert not s.reached_numeric_limit


def _build_c_consumer(tmp_path):
    import subprocess
    exe = str(tmp_path / 'c_abi_smoke')
    libdir = os.path.join(ROOT, 'beta_cores_amd')
    cmd = ['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'c_abi_smoke.c'),
           '-L', libdir, '-lbeta_cores', '-Wl,-rpath,' + libdir, '-Wl,-rpath,/opt/rocm/lib', '-lm', '-o', exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def test_header_is_plain_c_and_links(tmp_path):
    """include/beta_cores.h compiles as C99 and a pure-C program links against every entry point."""
    import subprocess
    exe = _build_c_consumer(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'entry points' in out.stdout
    n = int(out.stdout.split(',')[1].split()[0])
    assert n == len(header_functions())


def test_every_entry_point_refuses_null_arguments():
    """tests/abi_null_sweep.py against the shipped library (the same sweep runs on a host-sanitized build in
    tests/test_sanitized_cpu.py and, with a live context, in the -m gpu suite)."""
    import subprocess
    import sys
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'abi_null_sweep.py')], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and 'swept 8' in res.stdout, res.stdout + res.stderr[-2000:]
