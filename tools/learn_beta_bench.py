#!/usr/bin/env python3
"""Per-gradient wall time of BetaCoreset(learn_beta=True) on one GPU, at the shapes of two benchmark configurations:

  config 2: linear regression,   N = 1M resident rows, D = 64,  S = 100, a coreset of M = 100 rows
  config 3: logistic regression, N = 1M resident rows, D = 128, S = 100, M = 100

Three numbers per configuration, each the median over `--repeats` runs of `_optimize()` (`--grads` gradients per run, after one
warm-up run), divided by the number of gradients:

  fused          learn_beta=True, the default route: one bc_vi_beta_gradient call per gradient
  materialising  learn_beta=True, fused_gradient=False: every gradient writes the N x S projection and reads it back for its
                 column sums, and projects the coreset rows twice (value, beta-gradient) through the host
  floor          learn_beta=False: the fixed-beta gradient, one bc_vi_gradient call -- the call the fused one extends by one
                 M-row K1 and an M x S dot.  `--root TREE` measures this number alone in another (built) checkout, e.g. the
                 commit before the feature, on the same box.

Theta is fixed (the sampler returns the same S x D matrix), the step is tiny: the numbers are the gradient's, not the
sampler's or the optimiser's.

  python tools/learn_beta_bench.py [--rows N] [--grads G] [--repeats R] [--root TREE] [--out profiles/learn_beta_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def med(xs):
    xs = np.asarray(xs, dtype=np.float64)
    return {'median_ms': float(np.median(xs)), 'min_ms': float(xs.min()), 'max_ms': float(xs.max()), 'n': int(xs.size)}


def per_gradient_ms(ctx, alg, grads, repeats):
    w0, b0 = alg.wts.copy(), alg.beta
    times = []
    for rep in range(repeats + 1):                        # the first run warms up (buffers, code objects)
        alg.wts, alg.beta = w0.copy(), b0
        ctx.sync()
        t0 = time.perf_counter()
        alg._optimize()
        ctx.sync()
        if rep:
            times.append(1e3 * (time.perf_counter() - t0) / grads)
    return med(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=1_000_000)
    ap.add_argument('--grads', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--root', default=HERE)
    ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'learn_beta_bench.json'))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import beta_cores_amd as bc
    assert os.path.abspath(os.path.dirname(os.path.dirname(bc.__file__))) == os.path.abspath(args.root)
    ctx = bc.default_context()
    n, S, M = args.rows, 100, 100
    import inspect
    has_feature = 'beta_gradient' in inspect.signature(bc.likelihoods.LinearRegression.__init__).parameters
    res = {'N': n, 'S': S, 'M': M, 'grads': args.grads, 'device': torch.cuda.get_device_name(0), 'has_feature': has_feature, 'configs': {}}
    rng = np.random.RandomState(3)
    gen = torch.Generator(device='cuda').manual_seed(3)
    for name, D, dz in (('config2_linreg_D64', 64, 65), ('config3_logistic_D128', 128, 128)):
        t = torch.randn((n, dz), dtype=torch.float64, device='cuda', generator=gen)
        torch.cuda.synchronize()                              # the rows are borrowed: written before the library reads them
        dd = bc.DeviceData.from_torch(t, ctx=ctx)
        th = rng.randn(S, D) * (0.5 / np.sqrt(D))
        core_idx = rng.choice(n, M, replace=False)
        core = dd.rows(core_idx)
        kw = {'beta_gradient': True} if has_feature else {}
        model = bc.likelihoods.LinearRegression(1.0, **kw) if dz == D + 1 else bc.likelihoods.LogisticRegression(**kw)

        def make(learn, fused):
            prj = bc.DeviceBetaProjector(lambda k, w, p: th, S, model)
            return bc.BetaCoreset(dd, prj, opt_itrs=args.grads, step_sched=lambda i: 1e-9 / (1. + i), beta=0.5, learn_beta=learn,
                                  fused_gradient=fused, wts=np.full(M, n / float(M)), idcs=core_idx.copy(), pts=core.copy())
        leg = {'floor_fixed_beta': per_gradient_ms(ctx, make(False, True), args.grads, args.repeats)}
        if has_feature:
            leg['fused'] = per_gradient_ms(ctx, make(True, True), args.grads, args.repeats)
            leg['materialising'] = per_gradient_ms(ctx, make(True, False), args.grads, args.repeats)
            f, m, fl = (leg[k]['median_ms'] for k in ('fused', 'materialising', 'floor_fixed_beta'))
            leg['materialising_over_fused'] = m / f
            leg['fused_over_floor'] = f / fl
            print('%s: fused %.3f ms  materialising %.3f ms  floor (fixed beta) %.3f ms  | materialising / fused %.1f  fused / floor %.2f'
                  % (name, f, m, fl, m / f, f / fl), flush=True)
        else:
            print('%s: floor (fixed beta) %.3f ms' % (name, leg['floor_fixed_beta']['median_ms']), flush=True)
        res['configs'][name] = leg
        del dd, t
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps({'ok': True, 'out': args.out}))
    return 0


if __name__ == '__main__':
    sys.exit(main())
