"""Shared inputs of the NNLS refit tests (test_gpu_nnls.py on the device, test_nnls_cpu.py on the host model of the same
code): the seeded family of small least-squares problems, and a runner for tests/nnls_host_model.cpp."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S_VALUES = (1, 3, 7, 33, 64, 65, 100, 200, 257)
N_VALUES = (1, 2, 63, 64, 65, 127, 128)


def refit_cases(seed=5):
    """(S, n, cols[n, S], b[S], start weights[n]) for every S and every n <= S: rows Gaussian, every third case all-positive;
    b alternately a random vector and A.|x| + 0.1 noise; about half of the non-negative start weights are zero."""
    rng = np.random.RandomState(seed)
    k = 0
    for S in S_VALUES:
        for n in N_VALUES:
            if n > S:
                continue
            cols = rng.randn(n, S)
            if k % 3 == 2:
                cols = np.abs(cols)
            if k % 2 == 0:
                b = rng.randn(S)
            else:
                b = np.abs(rng.randn(n)).dot(cols) + 0.1 * rng.randn(S)
            val = np.abs(rng.randn(n)) * (rng.rand(n) < 0.5)
            k += 1
            yield S, n, cols, b, val


def build_host_model(outdir):
    exe = os.path.join(str(outdir), 'nnls_host_model')
    cmd = ['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-Wall', '-Werror', os.path.join(ROOT, 'tests', 'nnls_host_model.cpp'), '-o', exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def run_host_model(exe, cols, b, val, enter, whole_list, path):
    n, s = cols.shape
    with open(path, 'wb') as f:
        np.array([n, s, enter, whole_list], dtype=np.float64).tofile(f)
        np.ascontiguousarray(cols, dtype=np.float64).tofile(f)
        np.ascontiguousarray(b, dtype=np.float64).tofile(f)
        np.ascontiguousarray(val, dtype=np.float64).tofile(f)
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.split('\n')
    head = [int(v) for v in lines[0].split()]
    x = np.array([float(v) for v in lines[1:1 + n]])
    return head[0], head[1:], x
