"""The logistic Laplace sampler of the device weight optimisation without a GPU: csrc/bc_vi_laplace_dev.h compiled for the host
(tests/vi_laplace_harness.cpp) against the formulas in long double (tests/vi_laplace_cases.py), and the ABI of
include/beta_cores_vilaplace.h.  (The same harness under the sanitizers: tests/test_vi_laplace_sanitized_cpu.py.)

Bounds per case (vi_laplace_cases.check_mode_and_draw):
  mode:  max|mu - mu*| <= C_MODE 2^-53 (1 + max|mu*| + max_j sum_n w_n |z_nj|), C_MODE = 2^21 from the host's own Newton search
  draw:  Theta - mu against E . C(mu)^-T around the RETURNED mu under vi_sampler_cases.draw_bound, no constant changed."""
import os
import re
import subprocess

import numpy as np
import pytest

import vi_laplace_cases as lc
import vi_sampler_cases as vc
from beta_cores_amd import _native as N
from beta_cores_amd import samplers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['bc_vi_laplace_last_mode']


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    return lc.build_harness(tmp_path_factory.mktemp('vi_laplace'))


def test_long_double_carries_more_bits_than_double():
    assert np.finfo(np.longdouble).nmant >= 63 and vc.LD_OK


def test_host_newton_sets_the_constant():
    """Where C_MODE comes from: samplers._lr_mode_newton, cold from mu0 = 0, against the long-double mode over the whole grid.
    The measured worst ratio (8.91e4, recorded as lc.HOST_WORST_RATIO) times 16, rounded up to a power of two, is C_MODE; the
    host's search is held to the bound the two builds of the device text are held to."""
    assert lc.C_MODE == 2. ** np.ceil(np.log2(16. * lc.HOST_WORST_RATIO))
    worst = 0.
    for c in lc.grid() + lc.extra_cases():
        mu_ref = lc.reference_mode(c).astype(np.float64)
        keep = c['w'] > 0
        mu = samplers._lr_mode_newton(c['Z'][keep], c['w'][keep], np.zeros(c['d']))
        ratio = np.abs(mu - mu_ref).max() / (2. ** -53 * lc.mode_scale(c, mu_ref))
        worst = max(worst, ratio)
        assert ratio <= lc.C_MODE, (c['key'], ratio)
    print('worst ratio of the host Newton search: %.4g (C_MODE = %g)' % (worst, lc.C_MODE))


@pytest.mark.parametrize('d', lc.DIMS)
def test_mode_and_draw_match_the_long_double_reference(harness, tmp_path, d):
    worst = [0., 0.]
    for i, (m, s) in enumerate(lc.SHAPES):
        c = lc.make_case(d, m, s, variant=i + d)
        assert (c['w'] == 0.).any() or m == 1
        r = lc.run_laplace(harness, c, tmp_path)
        assert r['status'] == 0 and np.all(r['pad'] == 7.0)      # the padding of the zero-padded Theta is never written
        assert 1 <= r['counts'][0] <= 200 and r['counts'][2] == r['counts'][0] and 0 <= r['counts'][1] <= 34
        rm, rd = lc.check_mode_and_draw(c, r['mode'], r['theta'], 'host build')
        worst = [max(worst[0], rm), max(worst[1], rd)]
    print('worst error / bound at D = %d: mode %.3g, draw %.3g' % (d, worst[0], worst[1]))


@pytest.mark.parametrize('d,m,s', [(1, 7, 5), (3, 7, 5), (33, 130, 100), (128, 130, 100)])
def test_diagonal_form(harness, tmp_path, d, m, s):
    c = lc.make_case(d, m, s, variant=d, diag=True)
    r = lc.run_laplace(harness, c, tmp_path)
    assert r['status'] == 0 and np.all(r['pad'] == 7.0)
    lc.check_mode_and_draw(c, r['mode'], r['theta'], 'host build, diag')
    full = lc.run_laplace(harness, dict(c, diag=False), tmp_path)
    assert np.array_equal(full['mode'], r['mode'])                # the flag only changes the draw
    assert d == 1 or not np.array_equal(full['theta'], r['theta'])


def test_far_start_halves_and_reaches_the_mode(harness, tmp_path):
    c = lc.far_start_case()
    r = lc.run_laplace(harness, c, tmp_path)
    assert r['status'] == 0 and np.all(r['pad'] == 7.0)
    assert r['counts'][3] >= 1, r['counts']                       # the line search had to halve at least once
    lc.check_mode_and_draw(c, r['mode'], r['theta'], 'host build, far start')


def test_large_margins(harness, tmp_path):
    c = lc.large_margin_case()
    r = lc.run_laplace(harness, c, tmp_path)
    assert r['status'] == 0 and np.all(r['pad'] == 7.0)
    lc.check_mode_and_draw(c, r['mode'], r['theta'], 'host build, -z.start >= 100')


@pytest.mark.parametrize('d,m,s', [(1, 1, 1), (16, 7, 5), (128, 130, 100)])
def test_all_weights_zero_is_the_prior(harness, tmp_path, d, m, s):
    c = lc.make_case(d, m, s)
    c['w'] = np.zeros(m)
    r = lc.run_laplace(harness, c, tmp_path)
    assert r['status'] == 0 and np.all(r['pad'] == 7.0)
    assert np.array_equal(r['theta'], c['E']) and np.all(r['mode'] == 0.)
    assert r['counts'][0] == 0 and r['dec'] == 0.                 # no Newton step: the gradient is exactly 0
    c['start'] = 50. * np.ones(d)
    r = lc.run_laplace(harness, c, tmp_path)
    assert r['status'] == 0 and np.all(r['mode'] == 0.) and r['counts'][0] == 1      # cand = mu - mu in one full step
    assert np.array_equal(r['theta'], c['E'])


def test_a_weight_of_zero_contributes_exactly_nothing(harness, tmp_path):
    """The reference's Z[wts > 0]: dropping the rows of weight 0 changes no bit -- not even when such a row is infinite."""
    c = lc.make_case(16, 130, 5, variant=1)
    keep = c['w'] > 0
    r = lc.run_laplace(harness, c, tmp_path)
    sub = dict(c, Z=c['Z'][keep], w=c['w'][keep], m=int(keep.sum()))
    r2 = lc.run_laplace(harness, sub, tmp_path)
    assert np.array_equal(r['mode'], r2['mode']) and np.array_equal(r['theta'], r2['theta'])
    Z = c['Z'].copy()
    Z[np.where(~keep)[0][0], 3] = np.inf
    r3 = lc.run_laplace(harness, dict(c, Z=Z), tmp_path)
    assert r3['status'] == 0 and np.array_equal(r3['mode'], r['mode']) and np.array_equal(r3['theta'], r['theta'])


@pytest.mark.parametrize('what', ['nan weight', 'inf weight', 'inf row', 'nan start'])
def test_failures_return_the_status_and_write_nothing(harness, tmp_path, what):
    c = lc.make_case(16, 7, 5)
    c['Z'], c['w'], c['start'] = c['Z'].copy(), c['w'].copy(), c['start'].copy()
    n = int(np.where(c['w'] > 0)[0][0])
    if what == 'nan weight':
        c['w'][3] = np.nan
    elif what == 'inf weight':
        c['w'][n] = np.inf
    elif what == 'inf row':
        c['Z'][n, 2] = np.inf
    else:
        c['start'][5] = np.nan
    r = lc.run_laplace(harness, c, tmp_path)
    assert r['status'] == 1 and r['untouched']


# ---------------------------------------------------------------- the ABI of include/beta_cores_vilaplace.h
_CTYPES = {'bc_ctx*': N.vp, 'double*': N.vp, 'int32_t*': N.vp, 'int32_t': N.C.c_int32}


def test_vilaplace_header_and_ctypes_table_agree():
    src = open(os.path.join(ROOT, 'include', 'beta_cores_vilaplace.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    protos = {}
    for name, args in re.findall(r'\bint\s+(bc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', src):
        protos[name] = [re.sub(r'\s*\b[A-Za-z_][A-Za-z0-9_]*$', '', ' '.join(a.split())).strip() for a in args.split(',')]
    assert sorted(protos) == N.VILAPLACE_EXPORTS == NAMES
    for other in (N.EXPORTS, N.EXT_EXPORTS, N.F32_EXPORTS, N.NNLS_EXPORTS, N.TAKE_EXPORTS, N.BETAGRAD_EXPORTS, N.ENCODE_EXPORTS,
                  N.VIOPT_EXPORTS, N.PSVI_EXPORTS):
        assert not set(NAMES) & set(other)
    lib = N.load()
    for n, types in protos.items():
        assert hasattr(lib, n), 'libbeta_cores.so does not export %s' % n
        assert N._VILAPLACE_SIGNATURES[n] == [_CTYPES[t] for t in types]
        assert getattr(lib, n).argtypes == N._VILAPLACE_SIGNATURES[n]      # bound by load()
    viopt = open(os.path.join(ROOT, 'include', 'beta_cores_viopt.h')).read()
    assert re.search(r'#define\s+BC_VI_SAMPLER_LOGISTIC\s+2\b', viopt)
    assert 'a Newton solve on the device' not in viopt            # the line is struck from the header's "out of scope" list


def test_vilaplace_header_compiles_as_c99(tmp_path):
    src = tmp_path / 'use_vilaplace.c'
    src.write_text('#include "beta_cores_vilaplace.h"\n'
                   'typedef int (*fn)(void);\n'
                   'fn table[] = {%s};\n'
                   'int kind = BC_VI_SAMPLER_LOGISTIC;\n' % ', '.join('(fn)%s' % n for n in NAMES))
    cmd = ['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic-errors', '-I', os.path.join(ROOT, 'include'), '-c', str(src),
           '-o', str(tmp_path / 'use_vilaplace.o')]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_vilaplace_refuses_null_arguments():
    lib = N.load()
    assert lib.bc_vi_laplace_last_mode(None, 0, None, None) == N.BC_INVALID_ARGUMENT
    assert b'bc_vi_laplace_last_mode' in lib.bc_last_error()


def test_device_spec_of_the_logistic_sampler():
    mu0 = np.arange(3.)
    assert samplers.LogisticLaplaceSampler(mu0).device_spec() is None                       # the reference's BFGS stays on the host
    kind, sp = samplers.LogisticLaplaceSampler(mu0, solver='newton').device_spec()
    assert kind == 2 and np.array_equal(sp, [0., 1., 2., 0.])
    smp = samplers.LogisticLaplaceSampler(mu0, diag=True, solver='newton')
    smp._mode = np.array([5., 6., 7.])
    assert np.array_equal(smp.device_spec()[1], [5., 6., 7., 1.])
