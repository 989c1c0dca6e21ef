"""The device feature encoder without a GPU: the extension header include/beta_cores_encode.h is plain C, the names it
declares are exported and bound by a ctypes table of its own (the existing tables are left as they are), every entry point
refuses NULL arguments before any device is touched, MLPEncoder.from_torch / host() restate a torch network (a live one and
golden F23, the reference's feature extractor) within a derived bound, and the kernel's shape arithmetic
(csrc/bc_encode_tile.h) holds for every width 1..512 and depth 1..4 (tests/encode_tile_harness.c, a stand-alone program built
with -fsanitize=address,undefined).

The bound: host(bound=True) carries e through the layers with u the unit roundoff and gamma_k = k u / (1 - k u):
    a = |W||h| + |b|;   e_pre = |W| e_in + 2 gamma_{K+2} a;   e_post = |s| e_pre + 4 u (|pre * s| + |t|);   e_in = 0.
torch's float32 forward is checked against the float64 restatement with u = 2^-24.  (torch folds an eval-mode batch norm into
scale and shift in float32, the restatement in float64; the recurrence has no term of its own for that folding -- the slack of
gamma_{K+2} a, two evaluations' worth where only torch's is float32, covers it by a wide margin on these networks.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from beta_cores_amd import _native as N
from beta_cores_amd import encoders as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['bc_data_encode', 'bc_encoder_create', 'bc_encoder_destroy', 'bc_encoder_set_layer']
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'f23_neural_encoder.npz')


def header_functions():
    src = open(os.path.join(ROOT, 'include', 'beta_cores_encode.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(bc_[a-z0-9_]+)\s*\(', src)))


def test_encode_header_compiles_as_c99(tmp_path):
    src = tmp_path / 'use_encode.c'
    src.write_text('#include "beta_cores_encode.h"\n'
                   'typedef int (*fn)(void);\n'
                   'fn table[] = {%s};\n' % ', '.join('(fn)%s' % n for n in NAMES))
    cmd = ['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic-errors', '-I', os.path.join(ROOT, 'include'), '-c', str(src), '-o', str(tmp_path / 'use_encode.o')]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_encode_header_and_ctypes_table_agree():
    names = header_functions()
    assert names == N.ENCODE_EXPORTS == NAMES
    for other in (N.EXPORTS, N.EXT_EXPORTS, N.F32_EXPORTS, N.NNLS_EXPORTS, N.TAKE_EXPORTS, N.BETAGRAD_EXPORTS):
        assert not set(names) & set(other)
    lib = N.load()
    for n in names:
        assert hasattr(lib, n), 'libbeta_cores.so does not export %s' % n
        assert getattr(lib, n).argtypes == N._ENCODE_SIGNATURES[n]      # bound by load()
    for hdr in ('beta_cores.h', 'beta_cores_laplace.h', 'beta_cores_f32.h', 'beta_cores_nnls.h', 'beta_cores_take.h', 'beta_cores_betagrad.h'):
        src = open(os.path.join(ROOT, 'include', hdr)).read()
        assert not [n for n in names if n in src], hdr


def test_every_encode_entry_point_refuses_null_arguments():
    """A sweep over _ENCODE_SIGNATURES: all pointers NULL, all integers 0 -- refused with a message that names the entry
    point, before any device is touched."""
    lib = N.load()
    swept = 0
    for name, argtypes in sorted(N._ENCODE_SIGNATURES.items()):
        args = [None if t in (N.vp, N.vpp) else 0 for t in argtypes]
        assert getattr(lib, name)(*args) == N.BC_INVALID_ARGUMENT, name
        assert name.encode() in lib.bc_last_error(), name
        swept += 1
    assert swept == len(NAMES) == 4
    # each pointer on its own: a non-NULL neighbour does not get a NULL one through (the other pointers are never dereferenced
    # before the NULL check, so a dummy address is safe)
    dummy = C.c_void_p()
    w = (C.c_int32 * 2)(4, 4)
    assert lib.bc_encoder_create(None, 1, w, C.byref(dummy)) == N.BC_INVALID_ARGUMENT
    assert lib.bc_data_encode(None, None, 0, 8, C.byref(dummy)) == N.BC_INVALID_ARGUMENT
    assert lib.bc_encoder_set_layer(None, 0, w, None, None, None, 0) == N.BC_INVALID_ARGUMENT


def _sequential(seed=0, widths=(13, 20, 20)):
    import torch
    import torch.nn as nn
    torch.manual_seed(seed)
    mods = []
    for i in range(len(widths) - 1):
        mods += [nn.Linear(widths[i], widths[i + 1]), nn.BatchNorm1d(widths[i + 1]), nn.ReLU()]
    m = nn.Sequential(*mods)
    m.train()
    for _ in range(3):
        m(torch.randn(64, widths[0]) * 2 + 0.5)       # the running statistics move
    with torch.no_grad():
        for mod in m:
            if isinstance(mod, nn.BatchNorm1d):
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.normal_(0, 0.3)
    m.eval()
    return m


def _check_against_torch(layers, x, want):
    h, e64 = E.host_forward(layers, x, dtype=np.float64, bound=True)
    _, e32 = E.host_forward(layers, x, dtype=np.float64, bound=True, u=2.0 ** -24)
    err = np.abs(want.astype(np.float64) - h)
    print('torch float32 forward vs host: max err %.3e, max bound %.3e (float64 bound %.3e)' % (err.max(), e32.max(), e64.max()))
    assert np.all(err <= e32), np.max(err - e32)
    assert np.all(e64 < e32) and np.all(e64 >= 0)
    return h


def test_from_torch_on_a_live_module():
    import torch
    m = _sequential()
    layers = E.layers_from_torch(m)
    assert [l[0].shape for l in layers] == [(20, 13), (20, 20)] and all(l[4] for l in layers)
    assert all(l[0].dtype == np.float64 and l[2].dtype == np.float64 for l in layers)
    x = np.random.RandomState(1).randn(129, 13).astype(np.float32)
    with torch.no_grad():
        want = m(torch.from_numpy(x)).numpy()
    h = _check_against_torch(layers, x, want)
    # the same module in float64: the restatement's own bound
    m64 = _sequential().double()
    with torch.no_grad():
        want64 = m64(torch.from_numpy(x.astype(np.float64))).numpy()
    h64, e = E.host_forward(E.layers_from_torch(m64), x, dtype=np.float64, bound=True)
    assert np.all(np.abs(want64 - h64) <= e)
    # host(dtype=) rounds once; a Linear without bias, a last layer without ReLU or batch norm
    assert np.array_equal(E.host_forward(layers, x, dtype=np.float32), h.astype(np.float32).astype(np.float64))
    import torch.nn as nn
    m2 = nn.Sequential(nn.Linear(5, 7, bias=False), nn.ReLU(), nn.Linear(7, 3)).eval()
    l2 = E.layers_from_torch(m2)
    assert l2[0][1] is None and l2[0][2] is None and l2[0][4] and not l2[1][4]
    x2 = np.random.RandomState(2).randn(10, 5).astype(np.float32)
    with torch.no_grad():
        _check_against_torch(l2, x2, m2(torch.from_numpy(x2)).numpy())


def test_from_torch_on_golden_f23():
    import torch
    import torch.nn as nn
    g = np.load(GOLDEN)
    m = nn.Sequential(nn.Linear(13, 20), nn.BatchNorm1d(20), nn.ReLU(), nn.Linear(20, 20), nn.BatchNorm1d(20), nn.ReLU())
    m.load_state_dict({k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith('sd_')})
    for i in (1, 4):
        m[i].eps = float(g['eps'])
    m.eval()
    x = g['x']
    assert x.shape == (257, 13) and x.dtype == np.float32 and g['features'].dtype == np.float32
    assert (x[3] == 0).all() and (np.abs(x) == 1e4).sum() == 4
    h = _check_against_torch(E.layers_from_torch(m), x, g['features'])
    neg = g['all_negative_rows']
    assert (h[neg] == h[neg[0]]).all()                # all first-layer pre-activations negative: one and the same feature row
    assert os.path.getsize(GOLDEN) < 100 * 1024


def test_from_torch_refusals():
    import torch.nn as nn
    m = _sequential()
    m.train()
    with pytest.raises(ValueError, match='training'):
        E.layers_from_torch(m)
    m.eval()
    m[1].train()                                       # one batch norm left in training mode
    with pytest.raises(ValueError, match='training'):
        E.layers_from_torch(m)
    for bad, what in ((nn.Sequential(nn.Linear(3, 3), nn.Tanh()), 'Tanh'),
                      (nn.Sequential(nn.Linear(3, 3), nn.Dropout()), 'Dropout'),
                      (nn.Sequential(nn.BatchNorm1d(3), nn.Linear(3, 3)), 'follow a Linear'),
                      (nn.Sequential(nn.Linear(3, 3), nn.ReLU(), nn.BatchNorm1d(3)), 'follow a Linear'),
                      (nn.Sequential(nn.Linear(3, 3), nn.BatchNorm1d(3), nn.BatchNorm1d(3)), 'follow a Linear'),
                      (nn.Sequential(nn.ReLU(), nn.Linear(3, 3)), 'ReLU must follow'),
                      (nn.Sequential(), 'no Linear')):
        with pytest.raises(ValueError, match=what):
            E.layers_from_torch(bad.eval())
    with pytest.raises(ValueError, match='Sequential'):
        E.layers_from_torch(nn.Linear(3, 3).eval())
    with pytest.raises(ValueError, match='takes 4 inputs'):
        E.host_forward([(np.zeros((3, 2)), None, None, None, True), (np.zeros((2, 4)), None, None, None, True)], np.zeros((1, 2)))
    with pytest.raises(ValueError, match='1..512'):
        E.host_forward([(np.zeros((513, 2)), None, None, None, True)], np.zeros((1, 2)))


def test_host_relu_passes_nan_and_bound_is_zero_without_rounding():
    W = np.eye(3)
    x = np.array([[1., -2., 0.], [np.nan, 1., 1.]])       # (0 * nan is nan: the second row is nan throughout)
    out = E.host_forward([(W, None, None, None, True)], x, dtype=np.float64)
    assert np.array_equal(out[0], [1., 0., 0.]) and np.isnan(out[1]).all()
    h, e = E.host_forward([(W, None, None, None, False)], np.array([[1., 2., 3.]]), dtype=np.float64, bound=True)
    assert np.array_equal(h, [[1., 2., 3.]]) and np.all(e > 0) and np.all(e < 1e-14)


def test_tile_arithmetic_under_sanitizers(tmp_path):
    """tests/encode_tile_harness.c: the chooser for 4 x 512 x 512 width classes (rows per tile >= 16, a multiple of 16, LDS
    within budget) and the kernel's panel / padding indices replayed in an exactly-sized heap block."""
    exe = str(tmp_path / 'encode_tile')
    cmd = ['gcc', '-std=c99', '-O1', '-g', '-Wall', '-Werror', '-pedantic-errors', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
           '-I', os.path.join(ROOT, 'beta_cores_amd', 'csrc'), os.path.join(ROOT, 'tests', 'encode_tile_harness.c'), '-o', exe, '-lm']
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert int(out.stdout.split()[0]) == 512 + 3 * 512 * 512 and int(out.stdout.split()[3]) >= 16
