#!/usr/bin/env python3
"""What scoring held-out rows of the linear-regression models on the device costs (k_linreg_predict, samplers.linreg_predictive),
measured.

    python tools/predict_bench.py [--parts abc] [--reps 5] [--no-host] [--json profiles/predict_bench.json] [--table profiles/predict_table.md]

(a) Nt = 1M, D = 128, T = 101 (an evaluation curve's posteriors against a held-out set of the flagship's scale), float64 rows.
(b) Nt = 200 000, D = 512, T = 21, float64 rows: the widest rows the kernel serves, F walked in k-panels.
(c) The shape of examples/neural_linear.py: Nt = 200 000 raw float32 rows of 13 features through the encoder to 20 features, T = 1,
    with the re-encode (the network was retrained: encoder.version moved) and without it.

Per workload, after a warm call of the same shape: `gpu_ms`, HIP events around the call's kernels (the context's timer class 6:
the pack of F, k_linreg_predict, the combine) of `reps` synchronised calls, every repeat recorded; `wall_s`, the whole call with
the upload of the posteriors.  Kernel times by name come from a separate `rocprofv3 --kernel-trace --stats` run of this script.
The bounds: 2 T Nt D (D + 1) flops over the fp64 matrix peak (78.6 TFLOP/s, the spec figure the other notes use) and the rows'
bytes -- every posterior reads them once -- over the HBM peak (8 TB/s); `binds` names the larger, `share_of_bound` is it over the
best GPU time.  The parent commit has no device path, so the comparison (`numpy_*`) is the NumPy fp64 restatement on this host
with its threads -- Phi @ F, square, row-sum, the density -- timed in the same call on `--host-posteriors` posteriors and scaled
to T; for (c) it includes the encoder's NumPy restatement, which the host route needs first."""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))
import numpy as np

PEAK_FP64_MATRIX = 78.6e12
PEAK_HBM = 8.0e12


def numpy_predictive(Phi, y, mu, F, noise, scale):
    m = Phi.dot(mu)
    V = Phi.dot(F)
    var = noise + scale * (V * V).sum(axis=1)
    r = y - m
    return (-0.5 * (r * r / var + np.log(var) + np.log(2. * np.pi))).sum(), (r * r).sum()


def timed_calls(bc, ctx, reps, call, before=None):
    gpu, wall = [], []
    for _ in range(reps):
        if before:
            before()
        ctx.enable_timing(True)
        ctx.kernel_time_reset()
        t0 = time.perf_counter()
        res = call()
        wall.append(time.perf_counter() - t0)
        gpu.append(ctx.kernel_time(6)[0])
        ctx.enable_timing(False)
    return gpu, wall, res


def bounds(t, nt, d, row_bytes):
    flop_s = 2. * t * nt * d * (d + 1) / PEAK_FP64_MATRIX
    byte_s = float(t) * nt * row_bytes / PEAK_HBM
    return {'flop_bound_ms': flop_s * 1e3, 'byte_bound_ms': byte_s * 1e3, 'binds': 'fp64 matrix peak' if flop_s >= byte_s else 'HBM peak',
            'bound_ms': max(flop_s, byte_s) * 1e3}


def dense(a, bc, ctx, part, nt, d, t):
    rng = np.random.RandomState(3)
    Z = rng.randn(nt, d + 1)
    mu = rng.randn(t, d) / np.sqrt(d)
    F = np.tril(rng.randn(t, d, d)) * (0.3 / np.sqrt(d))
    noise, scale = 0.5 + rng.rand(t), np.ones(t)
    held = bc.RegressionHeldOut(Z)
    bc.linreg_predictive(held, mu[:1], F[:1], noise[:1], scale[:1])
    bc.linreg_predictive(held, mu, F, noise, scale)                      # the warm call of the measured shape
    gpu, wall, res = timed_calls(bc, ctx, a.reps, lambda: bc.linreg_predictive(held, mu, F, noise, scale))
    r = {'part': part, 'Nt': nt, 'D': d, 'T': t, 'rows': 'float64', 'gpu_ms': gpu, 'wall_s': wall}
    r.update(bounds(t, nt, d, (d + 1) * 8))
    r['share_of_bound'] = r['bound_ms'] / min(gpu)
    if not a.no_host:
        host, k = [], min(t, a.host_posteriors)
        for i in range(k):
            t0 = time.perf_counter()
            ll, sse = numpy_predictive(Z[:, :d], Z[:, d], mu[i], F[i], noise[i], scale[i])
            host.append(time.perf_counter() - t0)
        r.update({'numpy_s_per_posterior': host, 'numpy_s_scaled_to_T': min(host) * t, 'host_threads': os.environ.get('OMP_NUM_THREADS'),
                  'll_rel_diff': abs(res.ll[k - 1] - ll) / abs(ll), 'sse_rel_diff': abs(res.sse[k - 1] - sse) / abs(sse)})
    print(json.dumps(r), flush=True)
    return r


def example_shape(a, bc, ctx):
    rng = np.random.RandomState(4)
    nt, d0, d1 = 200000, 13, 20
    X = rng.randn(nt, d0)
    y = np.tanh(X[:, 0]) + 0.5 * X[:, 1] * X[:, 2] + 0.1 * rng.randn(nt)
    raw = np.hstack((X, y[:, None])).astype(np.float32)

    def layers():
        return [(rng.randn(d1, d0) * 0.3, rng.randn(d1) * 0.1, 1. + 0.1 * rng.rand(d1), rng.randn(d1) * 0.1, True),
                (rng.randn(d1, d1) * 0.3, rng.randn(d1) * 0.1, 1. + 0.1 * rng.rand(d1), rng.randn(d1) * 0.1, True)]
    enc = bc.encoders.MLPEncoder(layers())
    held = bc.RegressionHeldOut(raw, encoder=enc, dtype=np.float32)
    mu, F = rng.randn(d1) / np.sqrt(d1), np.tril(rng.randn(d1, d1)) * 0.1
    bc.linreg_predictive(held, mu, F, 1.0)
    out = []
    for name, before in (('c_with_re_encode', lambda: enc.update(enc.layers)), ('c_without_re_encode', None)):
        t0 = time.perf_counter()
        wall_all = []
        for _ in range(a.reps):
            if before:
                before()
            t0 = time.perf_counter()
            res = bc.linreg_predictive(held, mu, F, 1.0)
            wall_all.append(time.perf_counter() - t0)
        gpu, wall, res = timed_calls(bc, ctx, a.reps, lambda: bc.linreg_predictive(held, mu, F, 1.0), before=before)
        r = {'part': name, 'Nt': nt, 'D': d1, 'T': 1, 'rows': 'float32, encoded from %d raw features' % d0, 'gpu_ms_scoring_kernels': gpu,
             'wall_s_timed': wall, 'wall_s': wall_all}
        r.update(bounds(1, nt, d1, (d1 + 1) * 4))
        if not a.no_host:
            host = []
            for _ in range(2):
                t0 = time.perf_counter()
                if before:
                    feats = enc.host(raw[:, :d0], dtype=np.float32).astype(np.float64)
                ll, sse = numpy_predictive(feats, raw[:, d0].astype(np.float64), mu, F, 1.0, 1.0)
                host.append(time.perf_counter() - t0)
            r.update({'numpy_s': host, 'host_threads': os.environ.get('OMP_NUM_THREADS'), 'll_rel_diff': abs(res.ll[0] - ll) / abs(ll)})
        out.append(r)
        print(json.dumps(r), flush=True)
    return out


def table(rows):
    lines = ['| workload | Nt | D | T | GPU ms (each repeat) | best wall s | bound ms (which) | share of bound | NumPy on the host, s |', '|---|---|---|---|---|---|---|---|---|']
    for r in rows:
        gpu = r.get('gpu_ms', r.get('gpu_ms_scoring_kernels'))
        host = r.get('numpy_s_scaled_to_T', min(r['numpy_s']) if 'numpy_s' in r else None)
        lines.append('| %s | %d | %d | %d | %s | %.4f | %.3f (%s) | %.3f | %s |' % (
            r['part'], r['Nt'], r['D'], r['T'], ', '.join('%.3f' % g for g in gpu), min(r['wall_s']), r['bound_ms'], r['binds'],
            r['bound_ms'] / min(gpu), 'not measured' if host is None else '%.3g' % host))
    return '\n'.join(lines) + '\n'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parts', default='abc')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host-posteriors', type=int, default=2)
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--json', default=None)
    ap.add_argument('--table', default=None)
    a = ap.parse_args()
    import beta_cores_amd as bc
    ctx = bc.default_context()
    ctx.timing_classes(0x47)
    out = []
    if 'a' in a.parts:
        out.append(dense(a, bc, ctx, 'a', 1000000, 128, 101))
    if 'b' in a.parts:
        out.append(dense(a, bc, ctx, 'b', 200000, 512, 21))
    if 'c' in a.parts:
        out += example_shape(a, bc, ctx)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(out, f, indent=1)
    if a.table:
        with open(a.table, 'w') as f:
            f.write(table(out))


if __name__ == '__main__':
    main()
