"""The boundary of include/beta_cores_hmc_small.h without a GPU: every prototype is bound by _native (_HMC_SMALL_SIGNATURES) with
the argument types the header declares and nothing else is bound for it, the header compiles as C99, every entry point refuses
NULL arguments, and include/beta_cores.h and the tables of the other headers are untouched."""
import os
import re
import subprocess

from beta_cores_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['bc_hmc_small_begin', 'bc_hmc_small_chunk_begin', 'bc_hmc_small_chunk_end', 'bc_hmc_small_device_ms', 'bc_hmc_small_end',
         'bc_hmc_small_fits', 'bc_hmc_small_logjoint']
_CTYPES = {'bc_ctx*': N.vp, 'const double*': N.vp, 'double*': N.vp, 'const int64_t*': N.vp, 'int32_t*': N.vp, 'int32_t': N.C.c_int32,
           'int64_t': N.C.c_int64}


def prototypes(header):
    src = open(os.path.join(ROOT, 'include', header)).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    protos = {}
    for name, args in re.findall(r'\bint\s+(bc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', src):
        protos[name] = [re.sub(r'\s*\b[A-Za-z_][A-Za-z0-9_]*$', '', ' '.join(a.split())).strip() for a in args.split(',')]
    return protos


def test_header_and_ctypes_table_agree():
    protos = prototypes('beta_cores_hmc_small.h')
    assert sorted(protos) == N.HMC_SMALL_EXPORTS == NAMES
    others = (N.EXPORTS, N.EXT_EXPORTS, N.F32_EXPORTS, N.NNLS_EXPORTS, N.TAKE_EXPORTS, N.BETAGRAD_EXPORTS, N.ENCODE_EXPORTS, N.VIOPT_EXPORTS,
              N.PSVI_EXPORTS, N.VILAPLACE_EXPORTS, N.HMC_EXPORTS)
    for other in others:
        assert not set(NAMES) & set(other)                    # the existing tables are left as they are
    lib = N.load()
    for n, types in protos.items():
        assert hasattr(lib, n), 'libbeta_cores.so does not export %s' % n
        want = [_CTYPES[t] for t in types]
        sig = N._HMC_SMALL_SIGNATURES[n]
        assert len(sig) == len(want), n
        for k, (a, b) in enumerate(zip(sig, want)):
            assert a is b or (b is N.vp and a is N.c_dp), (n, k, types[k], a)      # (a typed double* is a void* to ctypes)
        assert getattr(lib, n).argtypes == sig                 # bound by load()
    for hdr in os.listdir(os.path.join(ROOT, 'include')):
        if hdr != 'beta_cores_hmc_small.h':
            src = open(os.path.join(ROOT, 'include', hdr)).read()
            assert 'bc_hmc_small' not in src, hdr
    # nothing else in _native is bound for this header
    bound = [n for n in dir(lib) if n.startswith('bc_hmc_small')]
    assert sorted(bound) == NAMES


def test_the_other_headers_keep_their_counts():
    assert len(N.EXPORTS) == 83 and len(N.HMC_EXPORTS) == 8 and len(prototypes('beta_cores_hmc.h')) == 8
    core = open(os.path.join(ROOT, 'include', 'beta_cores.h')).read()
    assert 'hmc' not in core.lower()


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / 'use_hmc_small.c'
    src.write_text('#include "beta_cores_hmc_small.h"\n'
                   'typedef int (*fn)(void);\n'
                   'fn table[] = {%s};\n' % ', '.join('(fn)%s' % n for n in NAMES))
    cmd = ['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic-errors', '-I', os.path.join(ROOT, 'include'), '-c', str(src), '-o',
           str(tmp_path / 'use_hmc_small.o')]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_entry_points_refuse_null_arguments():
    lib = N.load()
    assert lib.bc_hmc_small_fits(None, 10, 4) == 0
    assert lib.bc_hmc_small_logjoint(None, None, None, None, 0, 0, None, 0, None, None) == N.BC_INVALID_ARGUMENT
    assert b'bc_hmc_small_logjoint' in lib.bc_last_error()
    assert lib.bc_hmc_small_begin(None, None, None, None, 0, 0, None, 0, None, 0, 0) == N.BC_INVALID_ARGUMENT
    assert b'bc_hmc_small_begin' in lib.bc_last_error()
    assert lib.bc_hmc_small_chunk_begin(None, None, None, 0, 0, None) == N.BC_INVALID_ARGUMENT
    assert lib.bc_hmc_small_chunk_end(None, None, None, None, None) == N.BC_INVALID_ARGUMENT
    assert lib.bc_hmc_small_end(None) == N.BC_INVALID_ARGUMENT
    assert lib.bc_hmc_small_device_ms(None, None) == N.BC_INVALID_ARGUMENT
    assert b'bc_hmc_small_device_ms' in lib.bc_last_error()
