#!/usr/bin/env python3
"""Wall time per gradient of the greedy-VI weight optimisation (`_optimize()`: opt_itrs projected-ADAM steps, each with a fresh
posterior draw and a fresh projection) on one GPU, host loop against the device loop (GreedyVICoreset(device_optimize=True)):

  linreg_D64   linear regression,  N resident rows [x (64), y], LinregPosteriorSampler
  gauss_d8     Gaussian location,  N resident rows x (8),       GaussianPosteriorSampler
  logistic_D128 / logistic_D16   logistic regression, N resident rows z = y * x, LogisticLaplaceSampler(solver='newton'),
               n_subsample_opt in {200, 1000, None}; the device leg also reports the Newton steps per gradient (the seam
               bc_vi_laplace_last_mode)

each with S = 100 samples, a coreset of M = 100 rows and n_subsample_opt in {200, 1000, 100000, None}.  Per leg the median over
`--repeats` runs of `_optimize()` after one warm-up run, divided by opt_itrs:

  host     device_optimize=False: the sampler on the host, one bc_vi_gradient call per step, ADAM in NumPy.  `--root TREE` measures
           this leg alone in another (built) checkout -- the commit before the feature -- on the same box.
  device   device_optimize=True.  Also reported: the host's drawing time per step on its own (normals and indices) and the
           GPU time per step between HIP events around each chunk's steps; whichever is larger bounds the loop.

  python tools/vi_optimize_bench.py [--rows N] [--opt-itrs K] [--repeats R] [--root TREE] [--legs both|host|device]
                                    [--configs linreg_D64,gauss_d8,logistic_D128,logistic_D16]
                                    [--out profiles/vi_optimize_bench.json]"""
import argparse
import inspect
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def med(xs):
    xs = np.asarray(xs, dtype=np.float64)
    return {'median_ms': float(np.median(xs)), 'min_ms': float(xs.min()), 'max_ms': float(xs.max()), 'n': int(xs.size)}


def per_gradient(ctx, alg, itrs, repeats, device):
    w0 = alg.wts.copy()
    wall, draw, dev, newton = [], [], [], []
    prj = alg.ll_projector
    logistic = device and getattr(prj.sampler, 'solver', None) == 'newton'
    if device:
        run = prj.vi_optimize
        last = {}

        def timed(*a, **k):
            last.clear()
            return run(*a, timings=last, **k)
        prj.vi_optimize = timed
    for rep in range(repeats + 1):                        # the first run warms up (buffers, code objects)
        alg.wts = w0.copy()
        np.random.seed(rep)
        ctx.sync()
        t0 = time.perf_counter()
        alg._optimize()
        ctx.sync()
        if rep:
            wall.append(1e3 * (time.perf_counter() - t0) / itrs)
            if device:
                draw.append(1e3 * last['draw_s'] / itrs)
                dev.append(last['device_ms'] / itrs)
                if logistic:
                    newton.append(prj.vi_last_mode()['newton_total'] / float(itrs))
    out = {'wall': med(wall)}
    if device:
        assert alg.device_optimize_calls == repeats + 1, 'the device loop was not taken'
        out['host_draw'] = med(draw)
        out['device'] = med(dev)
        if logistic:
            out['newton_steps_per_gradient'] = float(np.median(newton))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=1_000_000)
    ap.add_argument('--opt-itrs', type=int, default=500)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--root', default=HERE)
    ap.add_argument('--legs', default='both', choices=['both', 'host', 'device'], help="'host' / 'device': that leg alone, in a process of its own")
    ap.add_argument('--configs', default='linreg_D64,gauss_d8,logistic_D128,logistic_D16')
    ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'vi_optimize_bench.json'))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import beta_cores_amd as bc
    assert os.path.abspath(os.path.dirname(os.path.dirname(bc.__file__))) == os.path.abspath(args.root)
    from beta_cores_amd.coreset.greedy_vi import GreedyVICoreset
    has_feature = 'device_optimize' in inspect.signature(GreedyVICoreset.__init__).parameters
    ctx = bc.default_context()
    n, S, M, itrs = args.rows, 100, 100, args.opt_itrs
    res = {'N': n, 'S': S, 'M': M, 'opt_itrs': itrs, 'device': torch.cuda.get_device_name(0), 'has_feature': has_feature,
           'root': 'this tree' if os.path.abspath(args.root) == HERE else 'other tree', 'configs': {}}
    gen = torch.Generator(device='cuda').manual_seed(3)
    known = (('linreg_D64', 64), ('gauss_d8', 8), ('logistic_D128', 128), ('logistic_D16', 16))
    for name, D in known:
        if name not in args.configs.split(','):
            continue
        rng = np.random.RandomState(3)
        lin, logit = name.startswith('linreg'), name.startswith('logistic')
        dz = D + 1 if lin else D
        t = torch.randn((n, dz), dtype=torch.float64, device='cuda', generator=gen)
        if lin:
            t[:, D] = t[:, :D] @ torch.full((D,), 1. / np.sqrt(D), dtype=torch.float64, device='cuda') + t[:, D]
        if logit:      # rows z = y * x with y ~ Bernoulli(sigmoid(x . theta / sqrt(D)))
            p = torch.sigmoid(t @ torch.full((D,), 1. / np.sqrt(D), dtype=torch.float64, device='cuda'))
            t *= torch.where(torch.rand(n, dtype=torch.float64, device='cuda', generator=gen) < p, 1., -1.)[:, None]
        torch.cuda.synchronize()                              # the rows are borrowed: written before the library reads them
        dd = bc.DeviceData.from_torch(t, ctx=ctx)
        core_idx = rng.choice(n, M, replace=False)
        core = dd.rows(core_idx)
        if lin:
            model = bc.likelihoods.LinearRegression(1.0)
            mk_sampler = lambda: bc.samplers.LinregPosteriorSampler(np.zeros(D), np.eye(D), 1.0)
        elif logit:
            model = bc.likelihoods.LogisticRegression()
            mk_sampler = lambda: bc.samplers.LogisticLaplaceSampler(np.zeros(D), solver='newton')
        else:
            model = bc.likelihoods.GaussianLocation(np.eye(D), 0.)
            mk_sampler = lambda: bc.samplers.GaussianPosteriorSampler(np.zeros(D), np.eye(D), np.eye(D))
        res['configs'][name] = {}
        for nsub in ((200, 1000, None) if logit else (200, 1000, 100000, None)):
            def make(device):
                kw = {'device_optimize': True} if device else {}
                return bc.SparseVICoreset(dd, bc.DeviceProjector(mk_sampler(), S, model), opt_itrs=itrs, n_subsample_opt=nsub,
                                          step_sched=lambda i: 1. / (1. + i), wts=np.full(M, n / float(M)), idcs=core_idx.copy(),
                                          pts=core.copy(), **kw)
            leg, line = {}, '%s n_subsample_opt=%s:' % (name, nsub)
            if args.legs != 'device':
                leg['host'] = per_gradient(ctx, make(False), itrs, args.repeats, False)
                line += ' host %.4f ms per gradient' % leg['host']['wall']['median_ms']
            if has_feature and args.legs != 'host':
                leg['device'] = per_gradient(ctx, make(True), itrs, args.repeats, True)
                d = leg['device']
                line += ' | device loop %.4f ms (host drawing alone %.4f, GPU between events %.4f)' % (
                    d['wall']['median_ms'], d['host_draw']['median_ms'], d['device']['median_ms'])
                if 'newton_steps_per_gradient' in d:
                    line += ', %.2f Newton steps per gradient' % d['newton_steps_per_gradient']
                if 'host' in leg:
                    leg['host_over_device'] = leg['host']['wall']['median_ms'] / d['wall']['median_ms']
                    line += ' | host / device %.2f' % leg['host_over_device']
            print(line, flush=True)
            res['configs'][name]['nsub_%s' % nsub] = leg
        del dd, t
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps({'ok': True, 'out': args.out}))
    return 0


if __name__ == '__main__':
    sys.exit(main())
