"""Shared by tests/test_vi_sampler_cpu.py and tests/test_vi_sampler_sanitized_cpu.py (no test collects from this file): the
seeded inputs of the posterior draw, the oracle's answer, and a runner for tests/vi_sampler_harness.cpp."""
import os
import subprocess

import numpy as np

from oracle import models_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINREG, GAUSS = 0, 1
DIMS, ROWS, SAMPLES = (1, 2, 3, 16, 33, 64, 128), (1, 7, 130), (1, 5, 100)


def build_harness(outdir, extra=()):
    exe = os.path.join(str(outdir), 'vi_sampler_harness')
    cmd = ['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-Wall', '-Werror'] + list(extra) \
        + [os.path.join(ROOT, 'tests', 'vi_sampler_harness.cpp'), '-o', exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def make_case(kind, d, m, s, sig0_sign=1.):
    """Sig0inv = I (times sig0_sign), weights in [0, 2] with some exactly 0 (never all of them)."""
    rng = np.random.RandomState(1000 * d + 10 * m + s + kind)
    x = rng.randn(m, d)
    w = rng.rand(m) * 2.
    w[rng.rand(m) < 0.3] = 0.
    if m > 1:
        w[0], w[m // 2] = 1.25, 0.
    th0 = rng.randn(d)
    E = rng.randn(s, d)
    c = {'kind': kind, 'd': d, 'm': m, 's': s, 'w': w, 'th0': th0, 'Sig0inv': sig0_sign * np.eye(d), 'E': E}
    if kind == LINREG:
        y = x.dot(rng.randn(d)) + rng.randn(m)
        c['rows'] = np.hstack((x, y[:, None]))
        c['sigsq'] = 1.5
    else:
        q = rng.randn(d, d)
        Sig = q.dot(q.T) / d + np.eye(d)
        c['rows'] = x
        c['Siginv'] = np.linalg.inv(Sig)
        c['Siginv'] = (c['Siginv'] + c['Siginv'].T) / 2.
    return c


def reference(c):
    """(Theta_ref = mu + E . L^T, kappa_2(A)) from the oracle's weighted posterior."""
    if c['kind'] == LINREG:
        mu, Ci, C = models_ref.linreg_weighted_post(c['th0'], c['Sig0inv'], c['sigsq'], c['rows'], c['w'])
    else:
        mu, Ci, C = models_ref.gauss_weighted_post(c['th0'], c['Sig0inv'], c['Siginv'], c['rows'], c['w'])
    return mu + c['E'].dot(Ci.T), np.linalg.cond(C.dot(C.T), 2)


def run_sampler(exe, c, tmp):
    """(status, theta [s][d], pad [s][3], saux [s], raw [s][d]) of the host build of bc_vi_sampler on case c."""
    d, m, s = c['d'], c['m'], c['s']
    parts = [np.array([c['kind'], d, m, s], dtype=np.float64), c['rows'].ravel(), c['w'], c['Sig0inv'].ravel(),
             np.dot(c['Sig0inv'], c['th0'])]
    parts.append(np.array([c['sigsq']]) if c['kind'] == LINREG else c['Siginv'].ravel())
    parts.append(c['E'].ravel())
    fin, fout = os.path.join(str(tmp), 'in.bin'), os.path.join(str(tmp), 'out.bin')
    np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in parts]).tofile(fin)
    out = subprocess.run([exe, 'sampler', fin, fout], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stderr == '', (out.returncode, out.stderr[-2000:])
    res = np.fromfile(fout)
    if int(res[0]) != 0:
        assert res.size == 1
        return int(res[0]), None, None, None, None
    dk = d + 3
    theta = res[1:1 + s * dk].reshape(s, dk)
    saux = res[1 + s * dk:1 + s * dk + s]
    raw = res[1 + s * dk + s:].reshape(s, d)
    return 0, theta[:, :d], theta[:, d:], saux, raw


def run_adam(exe, q, c, x0, step, tmp):
    itrs = step.shape[1]
    fin, fout = os.path.join(str(tmp), 'adam_in.bin'), os.path.join(str(tmp), 'adam_out.bin')
    np.concatenate([np.array([q.shape[0], itrs], dtype=np.float64), q, c, x0, step.ravel()]).tofile(fin)
    out = subprocess.run([exe, 'adam', fin, fout], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stderr == '', (out.returncode, out.stderr[-2000:])
    return np.fromfile(fout).reshape(itrs, q.shape[0])
