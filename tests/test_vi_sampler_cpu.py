"""The posterior draw and the ADAM body of the device weight optimisation without a GPU: csrc/bc_vi_sampler_dev.h compiled for
the host (tests/vi_sampler_harness.cpp) against the oracle's weighted posteriors and util.opt.nn_opt, and the ABI of
include/beta_cores_viopt.h.

Bound of the draw per case: 16 D 2^-53 kappa_2(A) (1 + max|Theta_ref|) -- the forward-error form of a Cholesky solve with a
margin of 16.  The worst observed ratio error / bound is recorded in profiles/vi_optimize_notes.md."""
import os
import re
import subprocess

import numpy as np
import pytest

import vi_sampler_cases as vc
from beta_cores_amd import _native as N
from beta_cores_amd.util.opt import adam_step_arrays, nn_opt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(['bc_vi_optimize', 'bc_vi_optimize_auto_chunk', 'bc_vi_optimize_begin', 'bc_vi_optimize_chunk_begin',
                'bc_vi_optimize_chunk_end', 'bc_vi_optimize_device_ms', 'bc_vi_optimize_end', 'bc_vi_optimize_last_draw'])


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    return vc.build_harness(tmp_path_factory.mktemp('vi_sampler'))


@pytest.mark.parametrize('kind', [vc.LINREG, vc.GAUSS])
@pytest.mark.parametrize('d', vc.DIMS)
def test_draw_matches_the_oracle(harness, tmp_path, kind, d):
    worst = 0.
    for m in vc.ROWS:
        for s in vc.SAMPLES:
            c = vc.make_case(kind, d, m, s)
            assert (c['w'] == 0.).any() or m == 1
            ref, kappa = vc.reference(c)
            status, theta, pad, saux, raw = vc.run_sampler(harness, c, tmp_path)
            assert status == 0
            assert np.all(pad == 7.0)                      # the padding of the zero-padded Theta is never written
            got = theta if kind == vc.LINREG else raw
            bound = 16. * d * 2. ** -53 * kappa * (1. + np.abs(ref).max())
            err = np.abs(got - ref).max()
            worst = max(worst, err / bound)
            print('kind %d D %3d m %3d S %3d: max error %.3e, bound %.3e, ratio %.3f, kappa %.3e' % (kind, d, m, s, err, bound, err / bound, kappa))
            assert err <= bound, (kind, d, m, s, err, bound)
            if kind == vc.GAUSS:
                # what K1 reads of a Gaussian draw: Theta' = (Siginv . Theta^T)^T and theta^T Siginv theta of the draw itself
                Si = c['Siginv']
                scale = np.abs(Si).sum(axis=1).max() * np.abs(raw).max()
                assert np.abs(theta - raw.dot(Si.T)).max() <= 4. * d * 2. ** -53 * scale
                assert np.abs(saux - (raw * raw.dot(Si)).sum(axis=1)).max() <= 4. * d * 2. ** -53 * scale * d * np.abs(raw).max()
    print('worst ratio of kind %d, D = %d: %.3f' % (kind, d, worst))


def test_long_double_carries_more_bits_than_double():
    """reference_ld is only a HIGH-precision reference where long double is x87 extended or wider; elsewhere the tests below
    fall back to the oracle and print that they did."""
    assert np.finfo(np.longdouble).nmant >= 63 and vc.LD_OK


@pytest.mark.parametrize('kind', [vc.LINREG, vc.GAUSS])
@pytest.mark.parametrize('d', vc.MORE_DIMS)
def test_general_prior_draw_matches_the_long_double_reference(harness, tmp_path, kind, d):
    """Dense Sig0inv, th0 != 0, sigsq != 1, scaled weights, nearly collinear columns (vc.make_general_case): the host build --
    bc_vi_prior_rhs included, the harness is handed th0 -- against the formulas in long double, and that reference against the
    oracle (LAPACK / BLAS in double).  Both under the bound of test_draw_matches_the_oracle, no constant changed."""
    worst = [0., 0.]
    for i, (m, s) in enumerate(vc.SHAPES):
        c = vc.make_general_case(kind, d, m, s, variant=i + d)
        ref, kappa = vc.high_precision_reference(c)
        status, theta, pad, saux, raw = vc.run_sampler(harness, c, tmp_path)
        assert status == 0 and np.all(pad == 7.0)
        got = theta if kind == vc.LINREG else raw
        bound = vc.draw_bound(d, kappa, ref)
        err, err_oracle = np.abs(got - ref).max(), np.abs(vc.reference(c)[0] - ref).max()
        worst = [max(worst[0], err / bound), max(worst[1], err_oracle / bound)]
        print('kind %d D %3d m %3d S %3d variant %d: host build %.3e, oracle %.3e, bound %.3e, kappa %.3e'
              % (kind, d, m, s, c['variant'], err, err_oracle, bound, kappa))
        assert err <= bound, (kind, d, m, s, err, bound)
        assert err_oracle <= bound, (kind, d, m, s, err_oracle, bound)
        if kind == vc.GAUSS:
            Si = c['Siginv']
            scale = np.abs(Si).sum(axis=1).max() * np.abs(raw).max()
            assert np.abs(theta - raw.dot(Si.T)).max() <= 4. * d * 2. ** -53 * scale
            assert np.abs(saux - (raw * raw.dot(Si)).sum(axis=1)).max() <= 4. * d * 2. ** -53 * scale * d * np.abs(raw).max()
    print('worst ratio of kind %d, D = %d, general priors: host build %.3f, oracle %.3f' % (kind, d, worst[0], worst[1]))


def test_prior_term_of_the_right_hand_side_takes_the_full_matrix(harness, tmp_path):
    """A strict upper triangle of Sig0inv that differs from the lower one: the factorisation reads the lower triangle (as LAPACK
    does), Sig0inv . th0 the whole matrix (as np.dot does)."""
    c = vc.make_general_case(vc.LINREG, 16, 7, 5, variant=1)
    c['Sig0inv'] = c['Sig0inv'] + np.triu(np.random.RandomState(3).randn(16, 16) * 0.05, 1)
    ref, kappa = vc.high_precision_reference(c)
    status, theta, _, _, _ = vc.run_sampler(harness, c, tmp_path)
    assert status == 0
    bound = vc.draw_bound(16, kappa, ref)
    assert np.abs(theta - ref).max() <= bound and np.abs(vc.reference(c)[0] - ref).max() <= bound
    sym = dict(c, Sig0inv=np.tril(c['Sig0inv']) + np.tril(c['Sig0inv'], -1).T)
    assert np.abs(vc.high_precision_reference(sym)[0] - ref).max() > 1e3 * bound      # (the case can tell the two apart)


@pytest.mark.parametrize('kind', [vc.LINREG, vc.GAUSS])
@pytest.mark.parametrize('d', [1, 3, 33, 128])
def test_precision_matrix_that_is_not_positive_definite_returns_the_flag(harness, tmp_path, kind, d):
    c = vc.make_case(kind, d, 7, 5, sig0_sign=-1.)
    if kind == vc.LINREG:
        c['w'] = c['w'] * 0.     # A = -I exactly
    else:
        c['w'] = c['w'] * 1e-3   # A = -I + (small) Siginv
    assert vc.run_sampler(harness, c, tmp_path)[0] == 1


def test_nan_in_the_weights_returns_the_flag(harness, tmp_path):
    c = vc.make_case(vc.LINREG, 16, 7, 5)
    c['w'][3] = np.nan
    assert vc.run_sampler(harness, c, tmp_path)[0] == 1


@pytest.mark.parametrize('sched', ['harmonic', 'large'])
def test_adam_body_is_nn_opt_bit_for_bit(harness, tmp_path, sched):
    rng = np.random.RandomState(5)
    m, itrs = 37, 60
    q, c, x0 = rng.rand(m) * 3. + .1, rng.randn(m), rng.rand(m)
    step_sched = (lambda i: 1. / (1. + i)) if sched == 'harmonic' else (lambda i: 2.5 / (1. + i) ** .5)
    trace = []

    def grd(x):
        trace.append(x.copy())
        return q * x - c
    ref = nn_opt(x0, grd, opt_itrs=itrs, step_sched=step_sched)
    got = vc.run_adam(harness, q, c, x0, adam_step_arrays(itrs, step_sched), tmp_path)
    assert np.array_equal(got[-1], ref)
    assert np.array_equal(got[:-1], np.array(trace[1:]))      # every intermediate iterate too
    assert (ref == 0.).any() and (ref > 0.).any()            # the clamp was exercised


def test_adam_body_propagates_nan(harness, tmp_path):
    q, c, x0 = np.ones(3), np.array([0., np.nan, 1.]), np.ones(3)
    ref = nn_opt(x0, lambda x: q * x - c, opt_itrs=3)
    got = vc.run_adam(harness, q, c, x0, adam_step_arrays(3, lambda i: 1. / (i + 1)), tmp_path)[-1]
    assert np.isnan(ref[1]) and np.array_equal(got, ref, equal_nan=True)


# ---------------------------------------------------------------- the ABI of include/beta_cores_viopt.h
_CTYPES = {'bc_ctx*': N.vp, 'const bc_data*': N.vp, 'const double*': N.vp, 'double*': N.vp, 'const int64_t*': N.vp,
           'int64_t': N.C.c_int64, 'int32_t': N.C.c_int32, 'int': N.C.c_int, 'double': N.C.c_double}


def viopt_prototypes():
    src = open(os.path.join(ROOT, 'include', 'beta_cores_viopt.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    protos = {}
    for name, args in re.findall(r'\bint\s+(bc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', src):
        types = []
        for a in args.split(','):
            a = ' '.join(a.split())
            types.append(re.sub(r'\s*\b[A-Za-z_][A-Za-z0-9_]*$', '', a).strip())      # drop the parameter's name
        protos[name] = types
    return protos


def test_viopt_header_and_ctypes_table_agree():
    protos = viopt_prototypes()
    assert sorted(protos) == N.VIOPT_EXPORTS == NAMES
    for other in (N.EXPORTS, N.EXT_EXPORTS, N.F32_EXPORTS, N.NNLS_EXPORTS, N.TAKE_EXPORTS, N.BETAGRAD_EXPORTS, N.ENCODE_EXPORTS):
        assert not set(NAMES) & set(other)                    # the existing tables are left as they are
    lib = N.load()
    for n, types in protos.items():
        assert hasattr(lib, n), 'libbeta_cores.so does not export %s' % n
        want = [_CTYPES[t] for t in types]
        sig = N._VIOPT_SIGNATURES[n]
        assert len(sig) == len(want), n
        for k, (a, b) in enumerate(zip(sig, want)):
            assert a is b or (b is N.vp and a is N.c_dp), (n, k, types[k], a)      # (a typed double* is a void* to ctypes)
        assert getattr(lib, n).argtypes == sig                 # bound by load()
    for hdr in os.listdir(os.path.join(ROOT, 'include')):
        if hdr != 'beta_cores_viopt.h':
            src = open(os.path.join(ROOT, 'include', hdr)).read()
            assert not [n for n in NAMES if n in src], hdr


def test_viopt_header_compiles_as_c99(tmp_path):
    src = tmp_path / 'use_viopt.c'
    src.write_text('#include "beta_cores_viopt.h"\n'
                   'typedef int (*fn)(void);\n'
                   'fn table[] = {%s};\n' % ', '.join('(fn)%s' % n for n in NAMES))
    cmd = ['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic-errors', '-I', os.path.join(ROOT, 'include'), '-c', str(src), '-o', str(tmp_path / 'use_viopt.o')]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_viopt_refuses_null_arguments():
    lib = N.load()
    z = [None] * 20
    assert lib.bc_vi_optimize(None, None, None, 0, 0, None, 0, 0, None, 0, None, 0, None, None, None, 0, 0., 0, None, None) == N.BC_INVALID_ARGUMENT
    assert b'bc_vi_optimize' in lib.bc_last_error()
    assert lib.bc_vi_optimize_begin(None, None, None, 0, 0, None, 0, 0, None, 0, None, 0, None, 0, 0., 0) == N.BC_INVALID_ARGUMENT
    assert lib.bc_vi_optimize_chunk_begin(None, None, None, 0) == N.BC_INVALID_ARGUMENT
    assert lib.bc_vi_optimize_chunk_end(None) == N.BC_INVALID_ARGUMENT
    assert lib.bc_vi_optimize_end(None, None, None) == N.BC_INVALID_ARGUMENT
    assert lib.bc_vi_optimize_device_ms(None, None) == N.BC_INVALID_ARGUMENT
    assert lib.bc_vi_optimize_last_draw(None, 0, 0, None, None, None, None) == N.BC_INVALID_ARGUMENT
    assert b'bc_vi_optimize_last_draw' in lib.bc_last_error()
    del z


def test_automatic_chunk_keeps_the_draws_under_the_budget():
    lib = N.load()
    budget = 32 << 20
    src = open(os.path.join(ROOT, 'include', 'beta_cores_viopt.h')).read()
    assert re.search(r'#define\s+BC_VI_STAGE_BYTES\s+\(32u << 20\)', src)
    for s, d, n_sub in ((100, 64, 0), (100, 64, 1000), (256, 128, 100000), (5, 1, 0), (256, 128, 10 ** 8)):
        k = lib.bc_vi_optimize_auto_chunk(s, d, n_sub)
        per = 8 * (s * d + n_sub)
        assert k >= 1 and (k * per <= budget or k == 1) and (k + 1) * per > budget or k == 1048576
