#!/usr/bin/env python3
"""The Laplace fits of the logistic drivers' evaluation curve -- the weighted coresets of sizes 0 .. 100 -- by one batched call
(samplers.logistic_laplace_many, k_laplace_many) beside the loop of samplers.logistic_laplace it replaces.

    python tools/laplace_many_bench.py [--dims 16,128] [--sizes 100] [--reps 5] [--baseline-tree DIR] [--json out.json]

Every leg runs in a process of its own (a fresh context), one warm pass of the same shapes first, then `reps` timed repeats; a
figure is a host clock around calls that return with their results on the host.  Reported: median (min - max).
  a_loop / a_many      the loop of logistic_laplace(w, DeviceData(Z), 0, solver='newton') over the P problems (upload included,
                       as logistic_hmc_many's default path does it) / one logistic_laplace_many call, with its GPU milliseconds
                       (bc_laplace_small_device_ms) beside the wall clock
  b_each / b_batched   logistic_hmc_many(start=None, inv_mass='laplace'), 16 chains, 200 iterations, with the fits inside the
                       window: laplace='each' (the default; in the baseline tree the call without the keyword) / 'batched'
  c_loop / c_many      the Laplace curve scored on 2 000 held-out rows with 1 000 draws per coreset: the loop of fits, NumPy's
                       draws and logistic_score / logistic_laplace_many(score=held, keep_draws=False) in 4 calls of 250 draws
                       (a call serves at most 256)
  tmc                  P = 2 000 problems of 1 .. 50 rows, D = 9 (tmc_shapley's shape): fits per second of one call
With --baseline-tree the loop legs import the package from DIR -- the parent commit's tree, built -- so the baseline is never this
tree's code; without it they use this tree (and say so)."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ.get('BC_BENCH_TREE') or os.path.join(HERE, '..'))
import numpy as np

BASELINE_LEGS = ('a_loop', 'b_each', 'c_loop')


def make_problems(sizes, d, seed=7):
    """The empty coreset and prefixes of 1 .. sizes rows of one data set (rows z = y x, the intercept the last column), weights
    N / m with N = 20 000: the README's curve."""
    rng = np.random.RandomState(seed)
    x = rng.randn(sizes, d)
    x[:, -1] = 1.
    y = np.where(rng.rand(sizes) < 1. / (1. + np.exp(-x.dot(rng.randn(d) / np.sqrt(d)))), 1., -1.)
    Z = y[:, None] * x
    return [(np.zeros((0, d)), np.zeros(0))] + [(Z[:m].copy(), np.full(m, 20000. / m)) for m in range(1, sizes + 1)]


def shapley_problems(P=2000, d=9, seed=9):
    rng = np.random.RandomState(seed)
    x = rng.randn(50, d)
    Z = np.where(rng.rand(50) < 0.5, 1., -1.)[:, None] * x
    return [(Z[rng.permutation(50)[:1 + p % 50]].copy(), None) for p in range(P)]


def held_out(samplers, d, n=2000, seed=13):
    rng = np.random.RandomState(seed)
    X = rng.randn(n, d)
    X[:, -1] = 1.
    return samplers.HeldOut(X, np.where(rng.rand(n) < 0.5, 1., -1.))


def leg_role(a):
    import beta_cores_amd as bc
    from beta_cores_amd import samplers
    bc.default_context()
    leg, d = a.leg, a.d
    probs = shapley_problems() if leg == 'tmc' else make_problems(a.sizes, d)
    own = not os.environ.get('BC_BENCH_TREE')
    held = held_out(samplers, d) if leg.startswith('c_') else None
    hmc = dict(start=None, inv_mass='laplace', n_samples=200, n_chains=16, step_size=0.004, n_leapfrog=8)
    gpu = []

    def fit_loop():
        out = []
        for Z, w in probs:
            if Z.shape[0] == 0:
                Z, w = np.zeros((1, d)), np.zeros(1)
            out.append(samplers.logistic_laplace(w, bc.DeviceData(Z), np.zeros(d), solver='newton'))
        return out

    def run():
        if leg == 'a_loop':
            fit_loop()
        elif leg in ('a_many', 'tmc'):
            gpu.append(samplers.logistic_laplace_many(probs).device_ms)
        elif leg == 'b_each':
            samplers.logistic_hmc_many(probs, rng=np.random.RandomState(3), **(dict(hmc, laplace='each') if own else hmc))
        elif leg == 'b_batched':
            samplers.logistic_hmc_many(probs, rng=np.random.RandomState(3), laplace='batched', **hmc)
        elif leg == 'c_loop':
            rng = np.random.RandomState(3)
            for mu, LSig, _ in fit_loop():
                samplers.logistic_score(held, mu + rng.randn(1000, d).dot(LSig.T))
        elif leg == 'c_many':
            rng = np.random.RandomState(3)
            gpu.append(sum(samplers.logistic_laplace_many(probs, n_draws=250, rng=rng, score=held, keep_draws=False).device_ms for _ in range(4)))
    run()
    del gpu[:]
    walls = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        run()
        walls.append(time.perf_counter() - t0)
    print(json.dumps({'leg': leg, 'D': d, 'P': len(probs), 'wall_s': walls, 'gpu_ms': gpu, 'tree': 'own' if own else 'baseline tree'}), flush=True)


def spread(v, scale=1.):
    v = sorted(x * scale for x in v)
    return '%.4g (%.4g - %.4g)' % (v[len(v) // 2], v[0], v[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dims', default='16,128')
    ap.add_argument('--sizes', type=int, default=100)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--legs', default='a_loop,a_many,b_each,b_batched,c_loop,c_many,tmc')
    ap.add_argument('--baseline-tree', default=None)
    ap.add_argument('--json', default=None)
    ap.add_argument('--leg', default=None)
    ap.add_argument('--d', type=int, default=16)
    a = ap.parse_args()
    if a.leg:
        return leg_role(a)
    out = []
    jobs = [(leg, int(d)) for d in a.dims.split(',') for leg in a.legs.split(',') if leg != 'tmc'] + ([('tmc', 9)] if 'tmc' in a.legs.split(',') else [])
    for leg, d in jobs:
        env = dict(os.environ)
        if a.baseline_tree and leg in BASELINE_LEGS:
            env['BC_BENCH_TREE'] = os.path.abspath(a.baseline_tree)
        cmd = [sys.executable, os.path.abspath(__file__), '--leg', leg, '--d', str(d), '--sizes', str(a.sizes), '--reps', str(a.reps)]
        child = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        if child.returncode != 0:
            raise RuntimeError('leg %s at D = %d failed (status %d): %s' % (leg, d, child.returncode, child.stderr[-2000:]))
        r = [json.loads(l) for l in child.stdout.splitlines() if l.startswith('{')][-1]
        out.append(r)
        line = '%-10s D %3d P %4d (%s): wall %s s' % (leg, d, r['P'], r['tree'], spread(r['wall_s']))
        if r['gpu_ms']:
            line += ', GPU %s ms' % spread(r['gpu_ms'])
        if leg in ('a_many', 'tmc'):
            line += ', %.0f fits / s' % (r['P'] / sorted(r['wall_s'])[len(r['wall_s']) // 2])
        print(line, flush=True)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
