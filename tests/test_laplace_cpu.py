"""The full-data logistic Laplace fit without a GPU: the Newton driver shared by the device route walks the host routine's
path (run here with a NumPy pass in _lr_mode_newton's expression order), and the device route checks its arguments and has
no CPU fallback."""
import numpy as np
import pytest

import beta_cores_amd as bc
from beta_cores_amd import samplers as S


def numpy_pass(Zw, ww):
    """A stand-in for bc.logistic_newton_pass on the rows Zw with weights ww, in _lr_mode_newton's expressions."""
    def lik(th, hessian):
        m = -Zw.dot(th)
        value = -(ww * (np.maximum(m, 0.) + np.log1p(np.exp(-np.fabs(m))))).sum()
        p = 0.5 * (1. + np.tanh(0.5 * m))
        grad = Zw.T.dot(ww * p)
        H = (Zw * (ww * p * (1. - p))[:, np.newaxis]).T.dot(Zw) if hessian else None
        return value, grad, H
    return lik


def problem(n, d, seed, scale=1.0):
    rng = np.random.RandomState(seed)
    X = rng.randn(n, d)
    y = np.where(rng.rand(n) < 1. / (1. + np.exp(-X.dot(rng.randn(d)))), 1., -1.)
    return y[:, None] * X, rng.rand(n) * scale


@pytest.mark.parametrize('n,d,seed,scale', [(200, 3, 0, 1.), (500, 6, 1, 40.), (80, 11, 2, 1e3), (1000, 16, 3, 5.)])
def test_newton_driver_matches_host_routine(n, d, seed, scale):
    Z, w = problem(n, d, seed, scale)
    w[::7] = 0.                                          # zero weights: filtered on the host, weight 0 in the pass
    mu0 = np.zeros(d)
    host = S._lr_mode_newton(Z[w > 0], w[w > 0], mu0)
    drv = S._newton_mode(numpy_pass(Z[w > 0], w[w > 0]), mu0)
    np.testing.assert_array_equal(drv, host)
    start = np.random.RandomState(seed + 9).randn(d)
    np.testing.assert_array_equal(S._newton_mode(numpy_pass(Z[w > 0], w[w > 0]), start),
                                  S._lr_mode_newton(Z[w > 0], w[w > 0], start))


def test_newton_driver_all_zero_weights_gives_prior_mode():
    Z, _ = problem(50, 5, 4)
    w = np.zeros(50)
    start = np.linspace(-1., 2., 5)
    host = S._lr_mode_newton(Z[w > 0], w[w > 0], start)
    drv = S._newton_mode(numpy_pass(Z[w > 0], w[w > 0]), start)
    np.testing.assert_array_equal(drv, host)
    np.testing.assert_array_equal(drv, np.zeros(5))


def fake_device_rows(n, d):
    """A DeviceData shell that never reached a GPU: enough for the argument checks, which run before any native call."""
    dd = bc.DeviceData.__new__(bc.DeviceData)
    dd.shape, dd.ctx, dd.row_offset = (n, d), None, 0
    return dd


def test_device_route_argument_checks():
    dd = fake_device_rows(10, 3)
    with pytest.raises(ValueError, match='one weight per row'):
        S.logistic_laplace(np.ones(9), dd, np.zeros(3))
    with pytest.raises(ValueError, match='mu0'):
        S.logistic_laplace(np.ones(10), dd, np.zeros(4))
    with pytest.raises(ValueError, match='solver'):
        S.logistic_laplace(None, dd, np.zeros(3), solver='lbfgs')
    with pytest.raises(ValueError, match='mu0'):
        S.LaplaceFullDataSampler(dd, np.zeros(2))


def test_pass_argument_checks():
    dd = fake_device_rows(10, 3)
    with pytest.raises(ValueError, match='theta'):
        bc.logistic_newton_pass(dd, np.zeros(4))
    with pytest.raises(ValueError, match='one weight per row'):
        bc.logistic_newton_pass(dd, np.zeros(3), w=np.ones(11))


def test_no_cpu_fallback():
    """Host rows handed to the device pass are uploaded first: without a GPU that fails loudly instead of computing on the CPU."""
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip('a GPU is present: the device route runs (tests/test_gpu_laplace.py)')
    except ImportError:
        pass
    Z, w = problem(20, 3, 5)
    with pytest.raises(RuntimeError):
        bc.logistic_newton_pass(Z, np.zeros(3), w=w)


def test_host_route_unchanged():
    """ndarray rows keep the host routine (the coreset-sized LogisticLaplaceSampler path)."""
    Z, w = problem(60, 4, 6)
    mu, LSig, LSigInv = S.logistic_laplace(w, Z, np.zeros(4), solver='newton')
    np.testing.assert_array_equal(mu, S._lr_mode_newton(Z[w > 0], w[w > 0], np.zeros(4)))
    np.testing.assert_allclose(LSig.dot(LSigInv), np.eye(4), atol=1e-12)


def ext_header_functions():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'beta_cores_laplace.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(bc_[a-z0-9_]+)\s*\(', src)))


def test_extension_header_and_ctypes_table_agree():
    from beta_cores_amd import _native as N
    names = ext_header_functions()
    assert names == N.EXT_EXPORTS == ['bc_logistic_newton_pass']
    assert not set(names) & set(N.EXPORTS)                 # the core table of include/beta_cores.h is left as it is
    lib = N.load()
    for n in names:
        assert hasattr(lib, n), 'libbeta_cores.so does not export %s' % n


def test_extension_entry_points_refuse_null_arguments():
    import ctypes as C
    from beta_cores_amd import _native as N
    lib = N.load()
    for name, argtypes in N._EXT_SIGNATURES.items():
        rc = getattr(lib, name)(*[None for _ in argtypes])
        assert rc == N.BC_INVALID_ARGUMENT, (name, rc)
        assert lib.bc_last_error(), name
        assert all(t is C.c_void_p for t in argtypes)


def test_extension_header_is_plain_c_and_links(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / 'c_abi_laplace')
    libdir = os.path.join(root, 'beta_cores_amd')
    cmd = ['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(root, 'include'), os.path.join(root, 'tests', 'c_abi_laplace.c'),
           '-L', libdir, '-lbeta_cores', '-Wl,-rpath,' + libdir, '-Wl,-rpath,/opt/rocm/lib', '-lm', '-o', exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert int(out.stdout.split(',')[1].split()[0]) == len(ext_header_functions())
