#!/usr/bin/env python3
"""The evaluation curve of the logistic drivers -- the posteriors of the weighted coresets of sizes 0 .. 100 -- sampled by one
batched call (samplers.logistic_hmc_many, k_hmc_small) beside a loop of samplers.logistic_hmc over the same problems.

    python tools/hmc_many_bench.py [--dims 16,128] [--sizes 100] [--chains 16] [--leapfrog 8] [--iters 200] [--reps 3]
                                   [--baseline-tree DIR] [--json out.json]

Problems: P = sizes + 1 weighted coresets, the empty one and n = 1 .. sizes rows of a seeded logistic data set, weights of
coreset size.  Every figure is a host clock around a call that ends in a device synchronise (the results are on the host when it
returns), after one warm call of the same shapes; `reps` repeats of the loop first, then of the batched call, every repeat
recorded; the ratios use the fastest repeat of each.
  many_shared / many_independent   logistic_hmc_many with draws='shared' / 'independent': wall seconds, the GPU milliseconds of
                                   the launch (bc_hmc_small_device_ms: HIP events around it) and GPU time per leapfrog step and
                                   problem; host_draw_s: the time NumPy takes for the draws of that mode alone
  loop                             logistic_hmc per problem with equally seeded streams, run in a child process.  With
                                   --baseline-tree the child imports the package from DIR -- the parent commit's tree, built --
                                   so the baseline is never this tree's code; without it the child uses this tree (and says so)
  agreement                        the largest relative deviation of the batched run's samples from the loop's (shared draws)"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ.get('BC_BENCH_TREE') or os.path.join(HERE, '..'))
import numpy as np


def make_problems(sizes, d, seed=7):
    """The empty coreset and prefixes of 1 .. sizes rows of one data set (rows z = y x, the intercept the last column), with
    weights that sum to about 20 000: a coreset of a data set of that size."""
    rng = np.random.RandomState(seed)
    x = rng.randn(sizes, d)
    x[:, -1] = 1.
    ths = rng.randn(d) / np.sqrt(d)
    y = np.where(rng.rand(sizes) < 1. / (1. + np.exp(-x.dot(ths))), 1., -1.)
    Z = y[:, None] * x
    probs = [(np.zeros((0, d)), np.zeros(0))]
    for m in range(1, sizes + 1):
        w = rng.rand(m) * 2. * (20000. / m)
        probs.append((Z[:m].copy(), w))
    return probs


def run_args(a, d):
    rng = np.random.RandomState(11)
    return dict(n_samples=a.iters, n_chains=a.chains, step_size=a.step, n_leapfrog=a.leapfrog, inv_mass=np.ones(d),
                start=rng.randn(a.chains, d) * 0.05)


def loop_role(a):
    """The child: a loop of logistic_hmc over the problems, `reps` times after a warm pass; prints one JSON line per dimension."""
    from beta_cores_amd import samplers
    for d in a.dims:
        probs = make_problems(a.sizes, d)
        kw = run_args(a, d)

        def loop(n_samples):
            out = []
            for Z, w in probs:
                if Z.shape[0] == 0:
                    Z, w = np.zeros((1, d)), np.zeros(1)
                out.append(samplers.logistic_hmc(Z, w, rng=np.random.RandomState(3), **dict(kw, n_samples=n_samples)).samples)
            return out
        loop(3)
        walls = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            res = loop(a.iters)
            walls.append(time.perf_counter() - t0)
        np.save(os.path.join(a.loop_out, 'loop_d%d.npy' % d), np.array(res))
        print(json.dumps({'D': d, 'loop_wall_s': walls, 'tree': 'baseline tree' if os.environ.get('BC_BENCH_TREE') else 'own'}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dims', default='16,128')
    ap.add_argument('--sizes', type=int, default=100)
    ap.add_argument('--chains', type=int, default=16)
    ap.add_argument('--leapfrog', type=int, default=8)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--step', type=float, default=0.004)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--baseline-tree', default=None)
    ap.add_argument('--json', default=None)
    ap.add_argument('--role', default='many', choices=['many', 'loop'])
    ap.add_argument('--loop-out', default=None)
    a = ap.parse_args()
    a.dims = [int(v) for v in a.dims.split(',')]
    if a.role == 'loop':
        return loop_role(a)
    import beta_cores_amd as bc
    from beta_cores_amd import samplers
    bc.default_context()
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        # the baseline first, in a fresh child process (its own context; this process has not launched anything yet)
        env = dict(os.environ)
        if a.baseline_tree:
            env['BC_BENCH_TREE'] = os.path.abspath(a.baseline_tree)
        cmd = [sys.executable, os.path.abspath(__file__), '--role', 'loop', '--loop-out', tmp, '--dims', ','.join(str(d) for d in a.dims),
               '--sizes', str(a.sizes), '--chains', str(a.chains), '--leapfrog', str(a.leapfrog), '--iters', str(a.iters), '--step', str(a.step),
               '--reps', str(a.reps)]
        child = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1500)
        if child.returncode != 0:
            raise RuntimeError('the baseline loop failed: ' + child.stderr[-2000:])
        loops = {r['D']: r for r in (json.loads(l) for l in child.stdout.splitlines() if l.startswith('{'))}
        for d in a.dims:
            probs = make_problems(a.sizes, d)
            kw = run_args(a, d)
            P = len(probs)
            r = {'D': d, 'P': P, 'C': a.chains, 'L': a.leapfrog, 'iterations': a.iters, 'step': a.step,
                 'loop_wall_s': loops[d]['loop_wall_s'], 'loop_tree': loops[d]['tree']}
            for mode in ('shared', 'independent'):
                samplers.logistic_hmc_many(probs, rng=np.random.RandomState(3), draws=mode, **dict(kw, n_samples=3))      # the warm launch
                walls, gpu = [], []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    res = samplers.logistic_hmc_many(probs, rng=np.random.RandomState(3), draws=mode, **kw)
                    walls.append(time.perf_counter() - t0)
                    gpu.append(res.device_ms)
                rng = np.random.RandomState(3)
                t0 = time.perf_counter()
                for _ in range(1 if mode == 'shared' else P):
                    rng.randn(a.iters, a.chains, d), np.log(rng.rand(a.iters, a.chains))
                r['many_%s' % mode] = {'wall_s': walls, 'gpu_ms': gpu, 'host_draw_s': time.perf_counter() - t0,
                                       'gpu_us_per_leapfrog_step_and_problem': min(gpu) * 1e3 / (a.iters * a.leapfrog * P),
                                       'accept_rate': float(np.mean([x.accept_rate.mean() for x in res])), 'fallback': res.fallback}
                if mode == 'shared':
                    ref = np.load(os.path.join(tmp, 'loop_d%d.npy' % d))
                    got = np.array([x.samples for x in res])
                    r['agreement_max_rel_dev'] = float(np.abs(got - ref).max() / np.abs(ref).max())
            best = min(r['loop_wall_s'])
            r['speedup_shared'] = best / min(r['many_shared']['wall_s'])
            r['speedup_independent'] = best / min(r['many_independent']['wall_s'])
            r['loop_ms_per_iteration_and_problem'] = best * 1e3 / (a.iters * P)
            out.append(r)
            print(json.dumps(r), flush=True)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
