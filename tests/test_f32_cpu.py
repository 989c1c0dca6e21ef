"""float32 data rows without a GPU: the extension header include/beta_cores_f32.h is plain C, every function it declares is
exported and bound by a ctypes table of its own (the two existing tables are left as they are), the new entry points refuse
NULL arguments before touching a device, and DeviceData refuses to round the caller's data before any context exists."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import beta_cores_amd as bc
from beta_cores_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def f32_header_functions():
    src = open(os.path.join(ROOT, 'include', 'beta_cores_f32.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(bc_[a-z0-9_]+)\s*\(', src)))


def test_f32_header_and_ctypes_table_agree():
    names = f32_header_functions()
    assert names == N.F32_EXPORTS
    assert {'bc_data_from_host_f32', 'bc_data_from_device_f32', 'bc_project_from_host_f32', 'bc_data_elem_bytes'} <= set(names)
    assert not set(names) & set(N.EXPORTS)                 # the core table of include/beta_cores.h is left as it is
    assert not set(names) & set(N.EXT_EXPORTS)             # and so is the Laplace extension's
    lib = N.load()
    for n in names:
        assert hasattr(lib, n), 'libbeta_cores.so does not export %s' % n
        assert getattr(lib, n).argtypes == N._F32_SIGNATURES[n]      # bound by load()


def test_existing_headers_do_not_declare_the_f32_entry_points():
    for hdr in ('beta_cores.h', 'beta_cores_laplace.h'):
        src = open(os.path.join(ROOT, 'include', hdr)).read()
        for n in N.F32_EXPORTS:
            assert n not in src, (hdr, n)


def test_f32_entry_points_refuse_null_arguments():
    lib = N.load()
    for name, argtypes in N._F32_SIGNATURES.items():
        rc = getattr(lib, name)(*[0 if t in (C.c_int64, C.c_int32, C.c_int) else None for t in argtypes])
        assert rc == N.BC_INVALID_ARGUMENT, (name, rc)
        assert name.encode() in lib.bc_last_error(), name


def test_f32_header_is_plain_c_and_links(tmp_path):
    exe = str(tmp_path / 'c_abi_f32')
    libdir = os.path.join(ROOT, 'beta_cores_amd')
    cmd = ['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'c_abi_f32.c'),
           '-L', libdir, '-lbeta_cores', '-Wl,-rpath,' + libdir, '-Wl,-rpath,/opt/rocm/lib', '-lm', '-o', exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert int(out.stdout.split(',')[1].split()[0]) == len(f32_header_functions())


class _NoContext:
    """Stands in for a Context: reaching for its handle means the dtype check came too late."""

    @property
    def h(self):
        raise AssertionError('the dtype check must run before any native call')


@pytest.mark.parametrize('make', [lambda: np.zeros((5, 3)), lambda: np.zeros((5, 3), dtype=np.float16),
                                  lambda: np.zeros((5, 3), dtype=np.int32), lambda: [[1., 2.], [3., 4.]]])
def test_float32_storage_never_rounds_the_callers_data(make, monkeypatch):
    from beta_cores_amd import device
    monkeypatch.setattr(device, 'default_context', lambda: (_ for _ in ()).throw(AssertionError('no context may be created')))
    with pytest.raises(ValueError, match='float32'):
        bc.DeviceData(make(), dtype=np.float32)
    with pytest.raises(ValueError, match='float32'):
        bc.DeviceData(make(), ctx=_NoContext(), dtype=np.float32)


@pytest.mark.parametrize('dtype', [np.float16, np.int32, np.int64, 'complex128'])
def test_unsupported_storage_dtypes_are_refused(dtype, monkeypatch):
    from beta_cores_amd import device
    monkeypatch.setattr(device, 'default_context', lambda: (_ for _ in ()).throw(AssertionError('no context may be created')))
    with pytest.raises(ValueError, match='float64 or float32'):
        bc.DeviceData(np.zeros((5, 3), dtype=np.float32), dtype=dtype)
    with pytest.raises(ValueError, match='float64 or float32'):
        bc.DeviceData(device_ptr=4096, shape=(5, 3), dtype=dtype)


def test_storage_dtype_rules():
    from beta_cores_amd.device import _as_rows, _storage_dtype
    z32 = np.arange(12, dtype=np.float32).reshape(4, 3)
    assert _storage_dtype(z32, None) == np.float64          # the default keeps today's behaviour: widened, stored as float64
    assert _storage_dtype(z32, np.float64) == np.float64
    assert _storage_dtype(z32, np.float32) == np.float32
    assert _storage_dtype(z32, 'float32') == np.float32
    rows = _as_rows(z32, np.dtype(np.float32), 'data')
    assert rows is z32                                      # uploaded as it is: no copy, and certainly no float64 one
    assert _as_rows(z32[:, ::2], np.dtype(np.float32), 'data').dtype == np.float32
    assert _as_rows(z32, np.dtype(np.float64), 'data').dtype == np.float64


def test_projector_keeps_large_float32_arrays_float32():
    from beta_cores_amd.coreset import projector as P
    big = np.zeros((P._SMALL_ROWS, 2), dtype=np.float32)
    assert P._resident_dtype(big) is np.float32
    assert P._resident_dtype(big[:-1]) is None              # small and transient inputs keep the float64 slots
    assert P._resident_dtype(big.astype(np.float64)) is None
    assert P._resident_dtype(bc.DeviceData.__new__(bc.DeviceData)) is None
