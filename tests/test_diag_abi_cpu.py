"""The boundary of include/beta_cores_diag.h without a GPU: every prototype is exported by the library and bound by _native
(_DIAG_SIGNATURES) with the argument types the header declares, the header compiles as C99, every NULL and every limit is
refused before a device is touched (context stand-ins of zero bytes), bc_diag_work_doubles is its documented closed form, and the
tables of the other headers are left as they are."""
import os
import re
import subprocess

import numpy as np

import diag_cases as DC
from beta_cores_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = 'beta_cores_diag.h'
NAMES = ['bc_chain_summary', 'bc_diag_attach', 'bc_diag_chunk', 'bc_diag_end', 'bc_diag_work_doubles']
_CTYPES = {'bc_ctx*': N.vp, 'const double*': N.vp, 'double*': N.vp, 'int32_t*': N.vp, 'int64_t': N.C.c_int64, 'int32_t': N.C.c_int32}


def prototypes():
    src = open(os.path.join(ROOT, 'include', HEADER)).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    protos = {}
    for name, args in re.findall(r'\b(?:int|int64_t)\s+(bc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', src):
        protos[name] = [re.sub(r'\s*\b[A-Za-z_][A-Za-z0-9_]*$', '', ' '.join(a.split())).strip() for a in args.split(',')]
    return protos


def test_header_and_ctypes_table_agree():
    protos = prototypes()
    assert sorted(protos) == N.DIAG_EXPORTS == NAMES
    every = (N.EXPORTS, N.EXT_EXPORTS, N.F32_EXPORTS, N.NNLS_EXPORTS, N.TAKE_EXPORTS, N.BETAGRAD_EXPORTS, N.ENCODE_EXPORTS, N.VIOPT_EXPORTS,
             N.PSVI_EXPORTS, N.VILAPLACE_EXPORTS, N.HMC_EXPORTS, N.HMC_SMALL_EXPORTS, N.PREFDIAG_EXPORTS, N.SCORE_EXPORTS, N.PREDICT_EXPORTS,
             N.LAPLACE_SMALL_EXPORTS, N.PSVI_MANY_EXPORTS, N.PSVI_CURVE_EXPORTS)
    mine = open(os.path.join(ROOT, 'include', HEADER)).read()
    for other in every:
        assert not set(NAMES) & set(other)
        assert not [o for o in other if o in mine and o != 'bc_last_error']      # this header spells no entry point of another ...
    lib = N.load()
    for n, types in protos.items():
        assert hasattr(lib, n), 'libbeta_cores.so does not export %s' % n
        sig = N._DIAG_SIGNATURES[n]
        assert sig == [_CTYPES[t] for t in types], n
        assert getattr(lib, n).argtypes == sig                 # bound by load()
    assert lib.bc_diag_work_doubles.restype == N.C.c_int64
    for hdr in os.listdir(os.path.join(ROOT, 'include')):      # ... and no other header spells one of its own
        if hdr != HEADER:
            src = open(os.path.join(ROOT, 'include', hdr)).read()
            assert not [n for n in NAMES if n in src], hdr
    makefile = open(os.path.join(ROOT, 'beta_cores_amd', 'csrc', 'Makefile')).read()
    assert ' bc_diag.hip ' in makefile
    assert 'HDRS = $(wildcard *.h) $(wildcard ../../include/*.h)\n%.o: %.hip $(HDRS)' in makefile
    import __graft_entry__ as g
    assert 'DIAG_EXPORTS' in open(g.__file__).read()           # build() looks for the new symbols


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / 'use_diag.c'
    src.write_text('#include "%s"\n'
                   'typedef int (*fn)(void);\n'
                   'fn table[] = {%s};\n'
                   'int64_t cap = BC_DIAG_MAX_WORK_DOUBLES;\nint chunk = BC_DIAG_COV_CHUNK;\n' % (HEADER, ', '.join('(fn)%s' % n for n in NAMES)))
    cmd = ['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic-errors', '-I', os.path.join(ROOT, 'include'), '-c', str(src), '-o',
           str(tmp_path / 'use_diag.o')]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_work_doubles_is_the_documented_closed_form():
    lib = N.load()
    for P, n, c, d, lag in [(1, 4, 1, 1, 1), (3, 4, 1, 1, 7), (2, 5, 2, 17, 1), (5, 64, 16, 9, 31), (2, 200, 16, 128, 10 ** 9), (1, 37, 3, 129, 4),
                            (1, 12, 64, 256, 5), (101, 1000, 16, 128, 499), (2000, 64, 16, 9, 31), (101, 200, 16, 16, 99), (7, 2049, 1, 16, 3)]:
        want = DC.work_doubles(P, n, c, d, lag)
        assert want > 0 and lib.bc_diag_work_doubles(P, n, c, d, lag) == want, (P, n, c, d, lag)
    assert DC.work_doubles(101, 1000, 16, 128, 499) == 2 * 101 * 1000 * 16 * 128 + 256 * 101 * 8 * 36 + 3 * 101 * 128 + 101 * 128 * 128 \
        + 2 * 101 * 128 + 101 * 128 * 500 + 6464 + 52
    for P, n, c, d, lag in [(0, 8, 2, 3, 1), (1, 3, 2, 3, 1), (1, 8, 0, 3, 1), (1, 8, 65, 3, 1), (1, 8, 2, 0, 1), (1, 8, 2, 257, 1), (1, 8, 2, 3, 0),
                            (1, 8, 2, 3, -1), (-1, 8, 2, 3, 1), (1, 1 << 31, 1, 1, 1), (1 << 20, 64, 16, 9, 31), (101, 2000, 16, 128, 3),
                            (1 << 40, 1 << 40, 64, 256, 1)]:
        assert DC.work_doubles(P, n, c, d, lag) == -1 and lib.bc_diag_work_doubles(P, n, c, d, lag) == -1, (P, n, c, d, lag)


class _Call:
    """The arguments of a valid bc_chain_summary on 2 x 8 x 2 x 3 draws, to be spoilt one at a time.  The context is a stand-in of
    zero bytes: every refusal tested here is made before it is looked at."""
    ORDER = ('ctx', 'samples', 'p', 'n', 'c', 'd', 'max_lag', 'mean', 'cov', 'rhat', 'ess', 'trunc', 'status', 'rho', 'moments')

    def __init__(self):
        self.ctx = N.C.create_string_buffer(4096)
        self.keep = [np.ones((2, 8, 2, 3)), np.zeros((2, 3)), np.zeros((2, 3, 3)), np.zeros((2, 3)), np.zeros((2, 3)),
                     np.zeros((2, 3), dtype=np.int32), np.zeros(2, dtype=np.int32)]
        ptr = [a.ctypes.data_as(N.vp) for a in self.keep]
        self.args = dict(ctx=N.C.cast(self.ctx, N.vp), samples=ptr[0], p=2, n=8, c=2, d=3, max_lag=3, mean=ptr[1], cov=ptr[2], rhat=ptr[3],
                         ess=ptr[4], trunc=ptr[5], status=ptr[6], rho=None, moments=None)

    def refused(self, **spoilt):
        a = dict(self.args, **spoilt)
        lib = N.load()
        return lib.bc_chain_summary(*[a[k] for k in self.ORDER]) == N.BC_INVALID_ARGUMENT and b'bc_chain_summary' in lib.bc_last_error()


def test_every_null_and_every_limit_is_refused_before_a_device_is_touched():
    lib = N.load()
    c = _Call()
    for k in ('ctx', 'samples', 'mean', 'cov', 'rhat', 'ess', 'trunc', 'status'):
        assert c.refused(**{k: None}), k
    assert c.refused(p=0) and c.refused(p=-2) and c.refused(n=3) and c.refused(n=0) and c.refused(c=0) and c.refused(c=65)
    assert c.refused(d=0) and c.refused(d=257) and c.refused(max_lag=0) and c.refused(max_lag=-1)
    assert c.refused(p=1 << 28)                                # the cap on the work space
    assert c.refused(n=1 << 31, c=1, d=1, p=1)                 # n C >= 2^31
    zero = N.C.cast(N.C.create_string_buffer(4096), N.vp)
    out = [a.ctypes.data_as(N.vp) for a in c.keep[1:]] + [None, None]
    for fn, args in (('bc_diag_attach', (None, 8, 3)), ('bc_diag_attach', (zero, 8, 3)), ('bc_diag_chunk', (None,)), ('bc_diag_chunk', (zero,)),
                     ('bc_diag_end', (None,) + (None,) * 8), ('bc_diag_end', (zero,) + tuple(out))):
        assert getattr(lib, fn)(*args) == N.BC_INVALID_ARGUMENT and fn.encode() in lib.bc_last_error(), fn
