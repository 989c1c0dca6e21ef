"""The boundary of include/beta_cores_score.h without a GPU: every prototype is exported by the library and bound by _native
(_SCORE_SIGNATURES) with the argument types the header declares, the header compiles as C99, every entry point refuses NULL
arguments before it touches a device, and the tables of the other headers are left as they are."""
import os
import re
import subprocess

from beta_cores_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['bc_lr_score', 'bc_score_chunk', 'bc_score_chunk_end']
_CTYPES = {'bc_ctx*': N.vp, 'const bc_data*': N.vp, 'const double*': N.vp, 'double*': N.vp, 'int32_t*': N.vp, 'int64_t': N.C.c_int64}


def prototypes(header):
    src = open(os.path.join(ROOT, 'include', header)).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    protos = {}
    for name, args in re.findall(r'\bint\s+(bc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', src):
        protos[name] = [re.sub(r'\s*\b[A-Za-z_][A-Za-z0-9_]*$', '', ' '.join(a.split())).strip() for a in args.split(',')]
    return protos


def test_header_and_ctypes_table_agree():
    protos = prototypes('beta_cores_score.h')
    assert sorted(protos) == N.SCORE_EXPORTS == NAMES
    for other in (N.EXPORTS, N.EXT_EXPORTS, N.F32_EXPORTS, N.NNLS_EXPORTS, N.TAKE_EXPORTS, N.BETAGRAD_EXPORTS, N.ENCODE_EXPORTS, N.VIOPT_EXPORTS,
                  N.PSVI_EXPORTS, N.VILAPLACE_EXPORTS, N.HMC_EXPORTS, N.HMC_SMALL_EXPORTS, N.PREFDIAG_EXPORTS):
        assert not set(NAMES) & set(other)
    lib = N.load()
    for n, types in protos.items():
        assert hasattr(lib, n), 'libbeta_cores.so does not export %s' % n
        sig = N._SCORE_SIGNATURES[n]
        assert sig == [_CTYPES[t] for t in types], n
        assert getattr(lib, n).argtypes == sig                 # bound by load()
    for hdr in os.listdir(os.path.join(ROOT, 'include')):
        if hdr != 'beta_cores_score.h':
            src = open(os.path.join(ROOT, 'include', hdr)).read()
            assert not [n for n in NAMES if n in src], hdr
    makefile = open(os.path.join(ROOT, 'beta_cores_amd', 'csrc', 'Makefile')).read()
    # the source is built, and the header is a prerequisite of every object: by name, or as one of all public headers
    assert ' bc_score.hip ' in makefile
    assert 'include/beta_cores_score.h' in makefile or 'HDRS = $(wildcard *.h) $(wildcard ../../include/*.h)\n%.o: %.hip $(HDRS)' in makefile


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / 'use_score.c'
    src.write_text('#include "beta_cores_score.h"\n'
                   'typedef int (*fn)(void);\n'
                   'fn table[] = {%s};\n' % ', '.join('(fn)%s' % n for n in NAMES))
    cmd = ['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic-errors', '-I', os.path.join(ROOT, 'include'), '-c', str(src), '-o',
           str(tmp_path / 'use_score.o')]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_entry_points_refuse_null_arguments():
    lib = N.load()
    assert lib.bc_lr_score(None, None, None, None, 0, None, None) == N.BC_INVALID_ARGUMENT
    assert b'bc_lr_score' in lib.bc_last_error()
    assert lib.bc_score_chunk(None, None, None) == N.BC_INVALID_ARGUMENT
    assert b'bc_score_chunk' in lib.bc_last_error()
    assert lib.bc_score_chunk_end(None, None, None, None, None, None, None) == N.BC_INVALID_ARGUMENT
    assert b'bc_score_chunk_end' in lib.bc_last_error()
