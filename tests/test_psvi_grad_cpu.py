"""BatchPSVICoreset's fused point-gradient without a GPU: csrc/bc_psvi_dev.h compiled for the host (tests/psvi_grad_harness.cpp)
against the reference's own expression evaluated in np.longdouble, and the ABI of include/beta_cores_psvi.h.

The bound, 8 (S + D) 2^-53 A[i, c], and its derivation are in tests/psvi_cases.py; the worst observed ratio error / bound per D is
recorded in profiles/psvi_notes.md."""
import os
import re
import subprocess

import numpy as np
import pytest

import psvi_cases as pc
from beta_cores_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(['bc_psvi_gradient', 'bc_psvi_gradient_begin', 'bc_psvi_gradient_end'])


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    return pc.build_harness(tmp_path_factory.mktemp('psvi_grad'))


def test_long_double_carries_more_bits_than_double():
    assert pc.LD_OK


@pytest.mark.parametrize('d', pc.DIMS)
def test_point_gradient_matches_the_long_double_reference(harness, tmp_path, d):
    worst = worst_np = 0.
    beyond = False
    for m, s in pc.SHAPES:
        for kind, sigsq in pc.MODELS:
            c = pc.make_case(kind, m, s, d, sigsq)
            assert m == 1 or (c['w'] == 0.).any()
            ref, bound = pc.reference(c)
            got = pc.run_harness(harness, c, tmp_path)
            err = np.abs(got - ref)
            ratio = float((err / np.where(bound > 0, bound, 1.)).max())
            # bpsvi.py:80 in NumPy doubles on the oracle's tensor lies within the same bound: the bound is no looser than the
            # reference's own rounding needs it to be
            err_np = np.abs(pc.numpy_expression(c) - ref)
            ratio_np = float((err_np / np.where(bound > 0, bound, 1.)).max())
            worst, worst_np = max(worst, ratio), max(worst_np, ratio_np)
            print('kind %d sigsq %.1f M %3d S %3d D %3d: host build %.3e (ratio %.3f), NumPy expression %.3e (ratio %.3f)'
                  % (kind, sigsq, m, s, d, float(err.max()), ratio, float(err_np.max()), ratio_np))
            assert np.all(err <= bound), (kind, sigsq, m, s, d, ratio)
            assert np.all(err_np <= bound), (kind, sigsq, m, s, d, ratio_np)
            if m > 1:
                assert np.all(got[m // 2] == 0.)                 # a zero weight: an exactly zero row
            if kind == pc.LOGISTIC:
                beyond = beyond or bool((-(c['pts'].dot(c['theta'].T)) >= 100.).any())
                if d == 1:
                    assert np.all(got == 0.)                     # centring over ONE coordinate leaves nothing
    assert beyond or d < 33      # (the scaled row takes some -z.th past the branch at 100 once the products can get there)
    print('worst ratio at D = %d: host build %.3f, NumPy expression %.3f' % (d, worst, worst_np))


def test_commuted_form_is_the_references_expression():
    """What the header relies on -- centring over the coordinates commutes with the sum over the samples -- in long double."""
    c = pc.make_case(pc.LINREG, 7, 5, 33, 2.5)
    ld = np.longdouble
    Gu, _ = pc.tensors_ld(c)
    V = (Gu * np.asarray(c['resid'], dtype=ld)[np.newaxis, :, np.newaxis]).sum(axis=1)
    g = -(np.asarray(c['w'], dtype=ld) / c['s'])[:, np.newaxis] * (V - V.mean(axis=1)[:, np.newaxis])
    ref, bound = pc.reference(c)
    assert np.all(np.abs(g - ref) <= bound * 2. ** -8)


# ---------------------------------------------------------------- the ABI of include/beta_cores_psvi.h
_CTYPES = {'bc_ctx*': N.vp, 'const bc_data*': N.vp, 'const double*': N.vp, 'double*': N.vp,
           'int64_t': N.C.c_int64, 'int32_t': N.C.c_int32, 'int': N.C.c_int, 'double': N.C.c_double}


def psvi_prototypes():
    src = open(os.path.join(ROOT, 'include', 'beta_cores_psvi.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    protos = {}
    for name, args in re.findall(r'\bint\s+(bc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', src):
        protos[name] = [re.sub(r'\s*\b[A-Za-z_][A-Za-z0-9_]*$', '', ' '.join(a.split())).strip() for a in args.split(',')]
    return protos


def test_psvi_header_and_ctypes_table_agree():
    protos = psvi_prototypes()
    assert sorted(protos) == N.PSVI_EXPORTS == NAMES
    for other in (N.EXPORTS, N.EXT_EXPORTS, N.F32_EXPORTS, N.NNLS_EXPORTS, N.TAKE_EXPORTS, N.BETAGRAD_EXPORTS, N.ENCODE_EXPORTS,
                  N.VIOPT_EXPORTS):
        assert not set(NAMES) & set(other)                    # the existing tables are left as they are
    lib = N.load()
    for n, types in protos.items():
        assert hasattr(lib, n), 'libbeta_cores.so does not export %s' % n
        want = [_CTYPES[t] for t in types]
        sig = N._PSVI_SIGNATURES[n]
        assert len(sig) == len(want), n
        for k, (a, b) in enumerate(zip(sig, want)):
            assert a is b, (n, k, types[k], a)
        assert getattr(lib, n).argtypes == sig                 # bound by load()
    for hdr in os.listdir(os.path.join(ROOT, 'include')):
        if hdr != 'beta_cores_psvi.h':
            src = open(os.path.join(ROOT, 'include', hdr)).read()
            assert not [n for n in NAMES if n in src], hdr


def test_psvi_header_compiles_as_c99(tmp_path):
    src = tmp_path / 'use_psvi.c'
    src.write_text('#include "beta_cores_psvi.h"\n'
                   'typedef int (*fn)(void);\n'
                   'fn table[] = {%s};\n' % ', '.join('(fn)%s' % n for n in NAMES))
    cmd = ['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic-errors', '-I', os.path.join(ROOT, 'include'), '-c', str(src), '-o', str(tmp_path / 'use_psvi.o')]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_psvi_refuses_null_arguments():
    lib = N.load()
    assert lib.bc_psvi_gradient(None, None, None, 0, 0, None, 0, None, 0, None, 1., None, None, None) == N.BC_INVALID_ARGUMENT
    assert b'bc_psvi_gradient' in lib.bc_last_error()
    assert lib.bc_psvi_gradient_begin(None, None, None, 0, 0, None, 0, None, 0, None, 1.) == N.BC_INVALID_ARGUMENT
    assert b'bc_psvi_gradient' in lib.bc_last_error()
    assert lib.bc_psvi_gradient_end(None, None, None, None) == N.BC_INVALID_ARGUMENT
    assert b'bc_psvi_gradient_end' in lib.bc_last_error()


def test_python_surface_without_a_gpu():
    """The flag and its counter exist and default to off; the row limit Python declines at is the header's."""
    import inspect
    from beta_cores_amd.coreset import projector
    from beta_cores_amd.coreset.bpsvi import BatchPSVICoreset
    assert inspect.signature(BatchPSVICoreset.__init__).parameters['fused_gradient'].default is False
    assert hasattr(projector.DeviceProjector, 'psvi_gradient') and not hasattr(projector.BlackBoxProjector, 'psvi_gradient')
    hdr = open(os.path.join(ROOT, 'beta_cores_amd', 'csrc', 'bc_psvi_dev.h')).read()
    assert int(re.search(r'#define\s+BC_PSVI_MAX_DZ\s+(\d+)', hdr).group(1)) == projector.PSVI_MAX_ROW_DOUBLES
    assert (2 * projector.PSVI_MAX_ROW_DOUBLES + projector.VI_MAX_SAMPLES + 17) * 8 <= 64 * 1024      # the kernel's LDS work space
