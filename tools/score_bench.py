#!/usr/bin/env python3
"""What scoring posterior samples on the device buys (k_lr_score, samplers.logistic_score, logistic_hmc_many(score=...),
valuation.tmc_shapley), measured.

    python tools/score_bench.py --part a [--thetas 323200] [--test-rows 10000] [--dims 128,16] [--reps 3] [--json out.json]
    python tools/score_bench.py --part bc [--test-rows 2000] [--dims 128,16] [--reps 2] [--baseline-tree DIR] [--json out.json]

(a) logistic_score of T thetas against Nt held-out rows.  gpu_ms: HIP events around the kernel (the context's timer class 6),
    after a warm call of the same shape; wall_s: the whole call, upload of the thetas included.  share_of_matrix_peak:
    2 T Nt D flops over the GPU time against the fp64 matrix peak of 78.6 TFLOP/s (the spec figure the other notes use);
    ns_per_term: GPU time per (theta, row) pair, the unit of the exp / log1p work.  numpy: the example's scoring
    (examples/logistic_mcmc_eval.py: compute_accuracy and the summed log_likelihood, three log_likelihood passes) on the host,
    timed on `--host-coresets` coresets' worth of thetas (T / 101 each) and scaled to T: the matrices of all T thetas at once
    would not fit the host's memory, and the example scores coreset by coreset too.
(b) The evaluation curve of the README -- 101 coresets of 0 .. 100 rows, 16 chains, 200 iterations of 8 leapfrog steps -- wall
    seconds of: `host`, logistic_hmc_many + the example's NumPy scoring, run in a child process that imports the package from
    --baseline-tree (the parent commit's tree, built) when given; `device`, logistic_hmc_many(score=held, keep_samples=False).
    The two alternate, `reps` times each, every repeat recorded.  sample_s / score_s split the host path.
(c) tmc_shapley: 50 groups of at most 50 rows, D = 9, max_groups = 20, T = 200 permutations: problems per second."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ.get('BC_BENCH_TREE') or os.path.join(HERE, '..'))
import numpy as np

PEAK_FP64_MATRIX = 78.6e12


def log_likelihood(z, th):
    """examples/logistic_mcmc_eval.py (model_lr.py:72-79)"""
    m = -np.atleast_2d(z).dot(np.atleast_2d(th).T)
    small = m < 100
    m[small] = -np.log1p(np.exp(m[small]))
    m[np.logical_not(small)] = -m[np.logical_not(small)]
    return m


def compute_accuracy(Xt, Yt, thetas):
    """examples/logistic_mcmc_eval.py (model_lr.py:32-42)"""
    loglikep, logliken = log_likelihood(Xt, thetas), log_likelihood(-Xt, thetas)
    predictions = np.ones(loglikep.shape)
    predictions[logliken > loglikep] = -1
    return np.mean(Yt[:, np.newaxis] == predictions)


def numpy_score(Xt, Yt, Zt, th):
    return compute_accuracy(Xt, Yt, th), log_likelihood(Zt, th).sum(axis=0).mean()


def make_test(nt, d, seed=5):
    rng = np.random.RandomState(seed)
    Xt = rng.randn(nt, d)
    Xt[:, -1] = 1.
    Yt = np.where(rng.rand(nt) < 0.5, 1., -1.)
    return Xt, Yt, Yt[:, None] * Xt


def make_problems(sizes, d, seed=7):
    """tools/hmc_many_bench.py's curve: the empty coreset and prefixes of 1 .. sizes rows, weights of coreset size."""
    rng = np.random.RandomState(seed)
    x = rng.randn(sizes, d)
    x[:, -1] = 1.
    ths = rng.randn(d) / np.sqrt(d)
    y = np.where(rng.rand(sizes) < 1. / (1. + np.exp(-x.dot(ths))), 1., -1.)
    Z = y[:, None] * x
    probs = [(np.zeros((0, d)), np.zeros(0))]
    for m in range(1, sizes + 1):
        probs.append((Z[:m].copy(), rng.rand(m) * 2. * (20000. / m)))
    return probs


def curve_args(a, d):
    rng = np.random.RandomState(11)
    return dict(n_samples=a.iters, n_chains=a.chains, step_size=0.004, n_leapfrog=a.leapfrog, inv_mass=np.ones(d), start=rng.randn(a.chains, d) * 0.05)


def part_a(a):
    import beta_cores_amd as bc
    ctx = bc.default_context()
    ctx.timing_classes(0x47)
    out = []
    for d in a.dims:
        Xt, Yt, Zt = make_test(a.test_rows, d)
        held = bc.samplers.HeldOut(Xt, Yt)
        th = np.random.RandomState(3).randn(a.thetas, d) / np.sqrt(d)
        bc.samplers.logistic_score(held, th[:4096])
        bc.samplers.logistic_score(held, th)                      # the warm call of the measured shape
        gpu, wall = [], []
        for _ in range(a.reps):
            ctx.enable_timing(True)
            ctx.kernel_time_reset()
            t0 = time.perf_counter()
            cor, ll = bc.samplers.logistic_score(held, th)
            wall.append(time.perf_counter() - t0)
            gpu.append(ctx.kernel_time(6)[0])
            ctx.enable_timing(False)
        per = max(1, a.thetas // 101)
        host = []
        for i in range(a.host_coresets):
            t0 = time.perf_counter()
            acc, tll = numpy_score(Xt, Yt, Zt, th[i * per:(i + 1) * per])
            host.append(time.perf_counter() - t0)
        i = a.host_coresets - 1
        dev_acc = held.accuracy(cor[i * per:(i + 1) * per])
        flops = 2. * a.thetas * a.test_rows * d
        r = {'part': 'a', 'D': d, 'T': a.thetas, 'Nt': a.test_rows, 'gpu_ms': gpu, 'wall_s': wall,
             'share_of_matrix_peak': flops / (min(gpu) * 1e-3) / PEAK_FP64_MATRIX, 'ns_per_term': min(gpu) * 1e6 / (a.thetas * a.test_rows),
             'numpy_s_per_coreset': host, 'numpy_thetas_per_coreset': per, 'numpy_s_scaled_to_T': min(host) * a.thetas / per,
             'host_threads': os.environ.get('OMP_NUM_THREADS'), 'accuracy_device': dev_acc, 'accuracy_numpy': float(acc),
             'test_ll_device': float(ll[i * per:(i + 1) * per].mean()), 'test_ll_numpy': float(tll)}
        out.append(r)
        print(json.dumps(r), flush=True)
    return out


def host_role(a):
    """The child of part (b): logistic_hmc_many + NumPy scoring, one JSON line per repeat as they finish."""
    from beta_cores_amd import samplers
    import beta_cores_amd
    d = a.dims[0]
    probs, kw = make_problems(a.sizes, d), curve_args(a, d)
    Xt, Yt, Zt = make_test(a.test_rows, d)
    samplers.logistic_hmc_many(probs, rng=np.random.RandomState(3), **dict(kw, n_samples=3))
    print(json.dumps({'ready': True, 'tree': os.path.dirname(os.path.dirname(os.path.abspath(beta_cores_amd.__file__)))}), flush=True)
    for line in sys.stdin:
        if line.strip() != 'go':
            break
        t0 = time.perf_counter()
        res = samplers.logistic_hmc_many(probs, rng=np.random.RandomState(3), **kw)
        t1 = time.perf_counter()
        sc = [numpy_score(Xt, Yt, Zt, r.pooled()) for r in res]
        t2 = time.perf_counter()
        print(json.dumps({'wall_s': t2 - t0, 'sample_s': t1 - t0, 'score_s': t2 - t1, 'accuracy': [float(s[0]) for s in sc],
                          'test_ll': [float(s[1]) for s in sc]}), flush=True)


def part_b(a):
    # the children first, one per dimension: fresh processes started before this one opens the device
    env = dict(os.environ)
    if a.baseline_tree:
        env['BC_BENCH_TREE'] = os.path.abspath(a.baseline_tree)
    children = {}
    for d in a.dims:
        cmd = [sys.executable, os.path.abspath(__file__), '--part', 'host', '--dims', str(d), '--test-rows', str(a.test_rows), '--sizes', str(a.sizes),
               '--chains', str(a.chains), '--leapfrog', str(a.leapfrog), '--iters', str(a.iters)]
        children[d] = subprocess.Popen(cmd, env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
    import beta_cores_amd as bc
    from beta_cores_amd import samplers
    bc.default_context()
    out = []
    for d in a.dims:
        child = children[d]
        try:
            ready = json.loads(child.stdout.readline())
            probs, kw = make_problems(a.sizes, d), curve_args(a, d)
            Xt, Yt, _ = make_test(a.test_rows, d)
            held = samplers.HeldOut(Xt, Yt)
            samplers.logistic_hmc_many(probs, rng=np.random.RandomState(3), score=held, keep_samples=False, **dict(kw, n_samples=3))
            host, dev = [], []
            for _ in range(a.reps):                                # the two alternate
                child.stdin.write('go\n')
                child.stdin.flush()
                host.append(json.loads(child.stdout.readline()))
                t0 = time.perf_counter()
                res = samplers.logistic_hmc_many(probs, rng=np.random.RandomState(3), score=held, keep_samples=False, **kw)
                dev.append({'wall_s': time.perf_counter() - t0, 'hmc_gpu_ms': res.device_ms})
                print('# D = %d: host %.3f s (sampling %.3f, scoring %.3f), device %.3f s' %
                      (d, host[-1]['wall_s'], host[-1]['sample_s'], host[-1]['score_s'], dev[-1]['wall_s']), flush=True)
        finally:
            child.stdin.close()
            child.wait(timeout=60)
        acc_dev = np.array([r.accuracy for r in res])
        ll_dev = np.array([r.test_ll.mean() for r in res])
        acc_host, ll_host = np.array(host[-1].pop('accuracy')), np.array(host[-1].pop('test_ll'))
        for h in host[:-1]:
            h.pop('accuracy'), h.pop('test_ll')
        r = {'part': 'b', 'D': d, 'P': len(probs), 'C': a.chains, 'L': a.leapfrog, 'iterations': a.iters, 'Nt': a.test_rows,
             'host_tree': ready['tree'], 'host': host, 'device': dev,
             'speedup_best_of_each': min(h['wall_s'] for h in host) / min(x['wall_s'] for x in dev),
             'accuracy_max_abs_diff': float(np.abs(acc_dev - acc_host).max()),
             'test_ll_max_rel_diff': float((np.abs(ll_dev - ll_host) / np.abs(ll_host)).max())}
        out.append(r)
        print(json.dumps(r), flush=True)
    return out


def part_c(a):
    import beta_cores_amd as bc
    rng = np.random.RandomState(9)
    G, d, mg, T = 50, 9, 20, a.perms
    sizes = rng.randint(10, 51, size=G)
    n = int(sizes.sum())
    X = np.hstack((rng.randn(n, d - 1), np.ones((n, 1))))
    th = rng.randn(d)
    Y = np.where(rng.rand(n) < 1. / (1. + np.exp(-X.dot(th))), 1., -1.)
    bounds = np.concatenate(([0], np.cumsum(sizes)))
    groups = [np.arange(bounds[g], bounds[g + 1]) for g in range(G)]
    for g in range(0, G, 5):                                       # every fifth group label-flipped
        Y[groups[g]] *= -1.
    Xt = np.hstack((rng.randn(a.test_rows, d - 1), np.ones((a.test_rows, 1))))
    Yt = np.where(rng.rand(a.test_rows) < 1. / (1. + np.exp(-Xt.dot(th))), 1., -1.)
    held = bc.samplers.HeldOut(Xt, Yt)
    Z = Y[:, None] * X
    kw = dict(group_cap=50, n_samples=64, n_chains=16, warmup=100, step_size=0.1, n_leapfrog=8)
    bc.valuation.tmc_shapley(Z, groups, held, 2, mg, rng=np.random.RandomState(1), **kw)
    walls = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        res = bc.valuation.tmc_shapley(Z, groups, held, T, mg, rng=np.random.RandomState(1), **kw)
        walls.append(time.perf_counter() - t0)
        print('# tmc_shapley: %d problems in %.3f s' % (T * mg, walls[-1]), flush=True)
    flipped = np.arange(0, G, 5)
    r = {'part': 'c', 'G': G, 'D': d, 'max_groups': mg, 'T': T, 'Nt': a.test_rows, 'problems': T * mg, 'wall_s': walls,
         'problems_per_s': T * mg / min(walls), 'n_fallback': res.n_fallback, 'perms_per_batch': bc.valuation.default_perms_per_batch(groups, d, mg, 50),
         'mean_phi_flipped_groups': float(res.phi[flipped].mean()), 'mean_phi_other_groups': float(np.delete(res.phi, flipped).mean())}
    print(json.dumps(r), flush=True)
    return [r]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', default='a', choices=['a', 'bc', 'host'])
    ap.add_argument('--dims', default='128,16')
    ap.add_argument('--thetas', type=int, default=323200)
    ap.add_argument('--test-rows', type=int, default=None)
    ap.add_argument('--host-coresets', type=int, default=2)
    ap.add_argument('--sizes', type=int, default=100)
    ap.add_argument('--chains', type=int, default=16)
    ap.add_argument('--leapfrog', type=int, default=8)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--perms', type=int, default=200)
    ap.add_argument('--reps', type=int, default=None)
    ap.add_argument('--baseline-tree', default=None)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    a.dims = [int(v) for v in a.dims.split(',')]
    if a.test_rows is None:
        a.test_rows = 10000 if a.part == 'a' else 2000
    if a.reps is None:
        a.reps = 3 if a.part == 'a' else 2
    if a.part == 'host':
        return host_role(a)
    out = part_a(a) if a.part == 'a' else part_b(a) + part_c(a)
    if a.json:
        old = []
        if os.path.exists(a.json):
            with open(a.json) as f:
                old = [r for r in json.load(f) if r.get('part') not in set(x['part'] for x in out)]
        with open(a.json, 'w') as f:
            json.dump(old + out, f, indent=1)


if __name__ == '__main__':
    main()
