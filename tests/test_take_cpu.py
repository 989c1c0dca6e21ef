"""The on-device row sub-sample without a GPU: the extension header include/beta_cores_take.h is plain C, the name it declares
is exported and bound by a ctypes table of its own (the four existing tables are left as they are), NULL arguments are refused
before any device is touched, and the access width the launch code picks (csrc/bc_take_width.h, compiled for the host) is the
widest that alignment allows for every base alignment, dz in 1..40 and 127..130, and both element sizes."""
import os
import re
import subprocess

from beta_cores_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['bc_data_take_rows']


def take_header_functions():
    src = open(os.path.join(ROOT, 'include', 'beta_cores_take.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(bc_[a-z0-9_]+)\s*\(', src)))


def test_take_header_compiles_as_c99(tmp_path):
    src = tmp_path / 'use_take.c'
    src.write_text('#include "beta_cores_take.h"\n'
                   'typedef int (*fn)(void);\n'
                   'fn table[] = {%s};\n' % ', '.join('(fn)%s' % n for n in NAMES))
    cmd = ['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic-errors', '-I', os.path.join(ROOT, 'include'), '-c', str(src), '-o', str(tmp_path / 'use_take.o')]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_take_header_and_ctypes_table_agree():
    names = take_header_functions()
    assert names == N.TAKE_EXPORTS == NAMES
    for other in (N.EXPORTS, N.EXT_EXPORTS, N.F32_EXPORTS, N.NNLS_EXPORTS):      # the four existing tables are left as they are
        assert not set(names) & set(other)
    lib = N.load()
    for n in names:
        assert hasattr(lib, n), 'libbeta_cores.so does not export %s' % n
        assert getattr(lib, n).argtypes == N._TAKE_SIGNATURES[n]      # bound by load()
    for hdr in ('beta_cores.h', 'beta_cores_laplace.h', 'beta_cores_f32.h', 'beta_cores_nnls.h'):
        src = open(os.path.join(ROOT, 'include', hdr)).read()
        assert not [n for n in names if n in src], hdr


def test_take_refuses_null_arguments():
    lib = N.load()
    assert lib.bc_data_take_rows(None, None, 0, None) == N.BC_INVALID_ARGUMENT
    assert b'bc_data_take_rows' in lib.bc_last_error()


def test_take_header_is_plain_c_and_links(tmp_path):
    exe = str(tmp_path / 'c_abi_take')
    libdir = os.path.join(ROOT, 'beta_cores_amd')
    cmd = ['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'c_abi_take.c'),
           '-L', libdir, '-lbeta_cores', '-Wl,-rpath,' + libdir, '-Wl,-rpath,/opt/rocm/lib', '-lm', '-o', exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert int(out.stdout.split(',')[1].split()[0]) == len(take_header_functions())


def test_access_width_is_the_widest_that_alignment_allows(tmp_path):
    """csrc/bc_take_width.h against a brute-force walk over the words of the rows (tests/take_width_harness.c): 2 element
    sizes x 44 column counts x every element-aligned pair of base offsets below 64."""
    exe = str(tmp_path / 'take_width')
    cmd = ['gcc', '-std=c99', '-O1', '-Wall', '-Werror', '-pedantic-errors', '-I', os.path.join(ROOT, 'beta_cores_amd', 'csrc'),
           os.path.join(ROOT, 'tests', 'take_width_harness.c'), '-o', exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert int(out.stdout.split()[0]) == 44 * (16 * 16 + 8 * 8)
