"""The boundary of include/beta_cores_predict.h without a GPU: the prototype is exported by the library and bound by _native
(_PREDICT_SIGNATURES) with the argument types the header declares, the header compiles as C99, the entry point refuses NULL
arguments before it touches a device, and the tables of the other headers are left as they are."""
import os
import re
import subprocess

from beta_cores_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['bc_linreg_predict']
_CTYPES = {'bc_ctx*': N.vp, 'const bc_data*': N.vp, 'const double*': N.vp, 'double*': N.vp, 'int64_t': N.C.c_int64}


def prototypes(header):
    src = open(os.path.join(ROOT, 'include', header)).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    protos = {}
    for name, args in re.findall(r'\bint\s+(bc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', src):
        protos[name] = [re.sub(r'\s*\b[A-Za-z_][A-Za-z0-9_]*$', '', ' '.join(a.split())).strip() for a in args.split(',')]
    return protos


def test_header_and_ctypes_table_agree():
    protos = prototypes('beta_cores_predict.h')
    assert sorted(protos) == N.PREDICT_EXPORTS == NAMES
    others = (N.EXPORTS, N.EXT_EXPORTS, N.F32_EXPORTS, N.NNLS_EXPORTS, N.TAKE_EXPORTS, N.BETAGRAD_EXPORTS, N.ENCODE_EXPORTS, N.VIOPT_EXPORTS,
              N.PSVI_EXPORTS, N.VILAPLACE_EXPORTS, N.HMC_EXPORTS, N.HMC_SMALL_EXPORTS, N.PREFDIAG_EXPORTS, N.SCORE_EXPORTS)
    for other in others:
        assert not set(NAMES) & set(other)
        assert not [o for o in other for n in NAMES if n in o or o in n]      # no name is a part of another
    lib = N.load()
    for n, types in protos.items():
        assert hasattr(lib, n), 'libbeta_cores.so does not export %s' % n
        sig = N._PREDICT_SIGNATURES[n]
        assert sig == [_CTYPES[t] for t in types], n
        assert getattr(lib, n).argtypes == sig                 # bound by load()
    mine = open(os.path.join(ROOT, 'include', 'beta_cores_predict.h')).read()
    for hdr in os.listdir(os.path.join(ROOT, 'include')):
        if hdr != 'beta_cores_predict.h':
            src = open(os.path.join(ROOT, 'include', hdr)).read()
            assert not [n for n in NAMES if n in src], hdr
    for other in others:                                       # and this header spells no entry point of another
        assert not [o for o in other if o in mine]
    makefile = open(os.path.join(ROOT, 'beta_cores_amd', 'csrc', 'Makefile')).read()
    assert ' bc_score.hip bc_predict.hip ' in makefile
    assert 'include/beta_cores_predict.h' in makefile or 'HDRS = $(wildcard *.h) $(wildcard ../../include/*.h)\n%.o: %.hip $(HDRS)' in makefile
    entry = open(os.path.join(ROOT, '__graft_entry__.py')).read()
    assert '_native.PREDICT_EXPORTS' in entry


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / 'use_predict.c'
    src.write_text('#include "beta_cores_predict.h"\n'
                   'typedef int (*fn)(void);\n'
                   'fn table[] = {%s};\n' % ', '.join('(fn)%s' % n for n in NAMES))
    cmd = ['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic-errors', '-I', os.path.join(ROOT, 'include'), '-c', str(src), '-o',
           str(tmp_path / 'use_predict.o')]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_entry_point_refuses_null_arguments():
    lib = N.load()
    assert lib.bc_linreg_predict(None, None, None, None, None, None, 0, None, None, None, None) == N.BC_INVALID_ARGUMENT
    err = lib.bc_last_error()
    assert b'bc_linreg_predict' in err and b'ctx is NULL' in err
