"""The boundary of include/beta_cores_prefdiag.h without a GPU: every prototype is bound by _native (_PREFDIAG_SIGNATURES) with
the argument types the header declares and nothing else is bound for it, the header compiles as C99, the info indices are
those the library fills, every entry point refuses NULL arguments with a message, and include/beta_cores.h is untouched."""
import os
import re
import subprocess

from beta_cores_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['bc_snnls_prefdiag_copy', 'bc_snnls_prefdiag_info', 'bc_snnls_prefdiag_sweep']
_CTYPES = {'bc_snnls*': N.vp, 'const bc_snnls*': N.vp, 'const char*': N.C.c_char_p, 'void*': N.vp, 'const double*': N.vp, 'float*': N.vp,
           'int64_t*': N.c_i64p, 'int32_t*': N.c_i32p, 'int32_t': N.C.c_int32, 'int64_t': N.C.c_int64, 'double': N.C.c_double}


def prototypes():
    src = open(os.path.join(ROOT, 'include', 'beta_cores_prefdiag.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    protos = {}
    for name, args in re.findall(r'\bint\s+(bc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', src):
        protos[name] = [re.sub(r'\s*\b[A-Za-z_][A-Za-z0-9_]*$', '', ' '.join(a.split())).strip() for a in args.split(',')]
    return protos


def test_header_and_ctypes_table_agree():
    protos = prototypes()
    assert sorted(protos) == N.PREFDIAG_EXPORTS == NAMES
    lib = N.load()
    for n, types in protos.items():
        assert hasattr(lib, n), 'libbeta_cores.so does not export %s' % n
        assert N._PREFDIAG_SIGNATURES[n] == [_CTYPES[t] for t in types], n
        assert getattr(lib, n).argtypes == N._PREFDIAG_SIGNATURES[n]
    assert not set(NAMES) & set(N.EXPORTS)
    assert 'prefdiag' not in open(os.path.join(ROOT, 'include', 'beta_cores.h')).read()


def test_header_compiles_as_c99_and_the_indices_are_dense(tmp_path):
    src = tmp_path / 'use_prefdiag.c'
    src.write_text('#include "beta_cores_prefdiag.h"\n'
                   'typedef int (*fn)(void);\n'
                   'fn table[] = {%s};\n'
                   'int64_t info[BC_PREFDIAG_INFO_N];\n' % ', '.join('(fn)%s' % n for n in NAMES))
    cmd = ['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic-errors', '-I', os.path.join(ROOT, 'include'), '-c', str(src), '-o',
           str(tmp_path / 'use_prefdiag.o')]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    hdr = open(os.path.join(ROOT, 'include', 'beta_cores_prefdiag.h')).read()
    idx = dict((k, int(v)) for k, v in re.findall(r'#define (BC_PREFDIAG_[A-Z0-9_]+) (\d+)', hdr))
    n = idx.pop('BC_PREFDIAG_INFO_N')
    assert sorted(idx.values()) == list(range(n))


def test_every_named_buffer_is_documented():
    """The names bc_snnls_prefdiag_copy accepts (the table of bc_pref_diag_buffer and the solver's own in bc_snnls_diag.hip) are
    those the header lists, "ctrl_swept" -- the control block as a diagnostic two-level sweep left it -- among them."""
    csrc = os.path.join(ROOT, 'beta_cores_amd', 'csrc')
    tab = re.findall(r'\{"([a-z0-9_]+)", p->[a-z0-9_]+, ', open(os.path.join(csrc, 'bc_prefilter.hip')).read())
    own = re.findall(r'strcmp\(which, "([a-z0-9_]+)"\)', open(os.path.join(csrc, 'bc_snnls_diag.hip')).read())
    assert 'ctrl' in tab and 'ctrl_swept' in tab and 'spill' in tab and 'v' in own
    hdr = open(os.path.join(ROOT, 'include', 'beta_cores_prefdiag.h')).read()
    doc = hdr[hdr.index('Copies ONE named device buffer'):hdr.index('int bc_snnls_prefdiag_copy')]
    assert sorted(set(re.findall(r'"([a-z0-9_]+)"', doc))) == sorted(set(tab + own))


def test_entry_points_refuse_null_arguments():
    lib = N.load()
    assert lib.bc_snnls_prefdiag_info(None, None) == N.BC_INVALID_ARGUMENT and b'bc_snnls_prefdiag_info' in lib.bc_last_error()
    assert lib.bc_snnls_prefdiag_copy(None, None, None, 0, None) == N.BC_INVALID_ARGUMENT and b'bc_snnls_prefdiag_copy' in lib.bc_last_error()
    assert lib.bc_snnls_prefdiag_sweep(None, 0, None, 1.0, 0, None, None, None, 0, 0, None) == N.BC_INVALID_ARGUMENT
    assert b'bc_snnls_prefdiag_sweep' in lib.bc_last_error()
