#!/usr/bin/env python3
"""Wall time per gradient of BatchPSVICoreset._optimize() (opt_itrs projected-ADAM steps over the weights AND the points, each
with a fresh posterior draw, a fresh projection of the data rows and the gradient with respect to weights and points) on one GPU:

  linreg_D64     linear regression,   N resident rows [x (64), y], LinregPosteriorSampler
  logistic_D128  logistic regression, N resident rows y*x (128),   LogisticLaplaceSampler(solver='newton')
  gauss_d8       Gaussian location,   N resident rows x (8),       GaussianPosteriorSampler

each with S = 100 samples, M in {10, 100} pseudo-points and n_subsample_opt in {200, None}.  ONE leg per process:

  --leg parent   another (built) checkout, given with --root: the commit before the feature, on the same box in the same session
  --leg off      this checkout, fused_gradient=False: colsum + project(grad=True) (the M x S x W tensor comes to the host) + NumPy
  --leg on       this checkout, fused_gradient=True: one bc_psvi_gradient call per gradient

Per configuration the median (min - max) over `--repeats` runs of `_optimize()` after one warm-up run, divided by opt_itrs.  Every
run starts from the same weights and points and the same seed, so the three legs do the same work.  The GPU time of
k_psvi_point_grad itself comes from a run of its own under `rocprofv3 --kernel-trace --stats` (`--leg on --profile`: one short
run per configuration, no timing reported).

  python tools/psvi_bench.py --leg off|on|parent [--root TREE] [--rows N] [--opt-itrs K] [--repeats R] [--profile]
                             [--out profiles/psvi_bench_<leg>.json]
  python tools/psvi_bench.py --merge parent.json off.json on.json [more.json ...] [--out profiles/psvi_bench.json]
                             (the table, no GPU; a leg given more than once shows the spread between processes)"""
import argparse
import inspect
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = (('linreg_D64', 64), ('logistic_D128', 128), ('gauss_d8', 8))


def med(xs):
    xs = np.asarray(xs, dtype=np.float64)
    return {'median_ms': float(np.median(xs)), 'min_ms': float(xs.min()), 'max_ms': float(xs.max()), 'n': int(xs.size)}


def per_gradient(ctx, alg, w0, p0, itrs, repeats):
    wall = []
    for rep in range(repeats + 1):                        # the first run warms up (buffers, code objects)
        alg.wts, alg.pts = w0.copy(), p0.copy()
        np.random.seed(rep)
        ctx.sync()
        t0 = time.perf_counter()
        alg._optimize()
        ctx.sync()
        if rep:
            wall.append(1e3 * (time.perf_counter() - t0) / itrs)
    return med(wall)


def merge(paths, out):
    """One table from the legs' files.  A leg given more than once (further processes of the same leg in the same session) shows
    the spread BETWEEN processes: its column is the first file's median (min - max of its 5 runs), then [the lowest - the highest
    median over all of that leg's processes]."""
    legs = {}
    for p in paths:
        r = json.load(open(p))
        legs.setdefault(r['leg'], []).append(r)
    res = {'legs': legs}
    keys = sorted(legs['on'][0]['configs'])
    print('| configuration | parent | flag off | flag on | on / parent |')
    print('|---|---|---|---|---|')

    def fmt(leg, k):
        v = legs[leg][0]['configs'][k]
        s = '%.3f (%.3f - %.3f)' % (v['median_ms'], v['min_ms'], v['max_ms'])
        meds = [r['configs'][k]['median_ms'] for r in legs[leg]]
        return s + (' [%.3f - %.3f]' % (min(meds), max(meds)) if len(meds) > 1 else '')
    for k in keys:
        on, par = legs['on'][0]['configs'][k]['median_ms'], [r['configs'][k]['median_ms'] for r in legs['parent']]
        print('| %s | %s | %s | %s | %s |' % (k, fmt('parent', k), fmt('off', k), fmt('on', k),
                                             '%.2f' % (on / par[0]) if len(par) == 1 else '%.2f - %.2f' % (on / max(par), on / min(par))))
    with open(out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--leg', choices=['parent', 'off', 'on'])
    ap.add_argument('--merge', nargs='+', metavar='JSON')
    ap.add_argument('--rows', type=int, default=1_000_000)
    ap.add_argument('--opt-itrs', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--root', default=HERE)
    ap.add_argument('--profile', action='store_true', help='one short run per configuration and no timing: for a run under rocprofv3')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.merge:
        return merge(args.merge, args.out or os.path.join(HERE, 'profiles', 'psvi_bench.json'))
    if args.leg is None:
        ap.error('--leg or --merge')
    root = os.path.abspath(args.root)
    if (args.leg == 'parent') == (root == HERE):
        ap.error("--leg parent measures ANOTHER checkout (--root TREE); the legs 'off' and 'on' measure this one")
    sys.path.insert(0, root)
    import torch
    import beta_cores_amd as bc
    assert os.path.abspath(os.path.dirname(os.path.dirname(bc.__file__))) == root
    has_feature = 'fused_gradient' in inspect.signature(bc.BatchPSVICoreset.__init__).parameters
    assert has_feature == (args.leg != 'parent'), 'the parent leg wants a checkout without the feature, the other two one with it'
    ctx = bc.default_context()
    n, S, itrs = args.rows, 100, (8 if args.profile else args.opt_itrs)
    repeats = 0 if args.profile else args.repeats
    res = {'leg': args.leg, 'N': n, 'S': S, 'opt_itrs': itrs, 'repeats': repeats, 'device': torch.cuda.get_device_name(0), 'configs': {}}
    gen = torch.Generator(device='cuda').manual_seed(3)
    for name, D in CONFIGS:
        rng = np.random.RandomState(3)
        kind = name.split('_')[0]
        dz = D + 1 if kind == 'linreg' else D
        t = torch.randn((n, dz), dtype=torch.float64, device='cuda', generator=gen)
        if kind == 'linreg':
            t[:, D] = t[:, :D] @ torch.full((D,), 1. / np.sqrt(D), dtype=torch.float64, device='cuda') + t[:, D]
        elif kind == 'logistic':      # rows z = y*x with y drawn from the model at theta = 1/sqrt(D)
            p = torch.sigmoid(t @ torch.full((D,), 1. / np.sqrt(D), dtype=torch.float64, device='cuda'))
            t *= torch.where(torch.rand(n, dtype=torch.float64, device='cuda', generator=gen) < p, 1., -1.)[:, None]
        torch.cuda.synchronize()                              # the rows are borrowed: written before the library reads them
        dd = bc.DeviceData.from_torch(t, ctx=ctx)
        if kind == 'linreg':
            model = bc.likelihoods.LinearRegression(1.0)
            mk_sampler = lambda: bc.samplers.LinregPosteriorSampler(np.zeros(D), np.eye(D), 1.0)
        elif kind == 'logistic':
            model = bc.likelihoods.LogisticRegression()
            mk_sampler = lambda: bc.samplers.LogisticLaplaceSampler(np.zeros(D), solver='newton')
        else:
            model = bc.likelihoods.GaussianLocation(np.eye(D), 0.)
            mk_sampler = lambda: bc.samplers.GaussianPosteriorSampler(np.zeros(D), np.eye(D), np.eye(D))
        for M in (10, 100):
            idcs = rng.choice(n, M, replace=False)
            p0, w0 = dd.rows(idcs), np.full(M, n / float(M))
            for nsub in (200, None):
                kw = {'fused_gradient': args.leg == 'on'} if has_feature else {}
                alg = bc.BatchPSVICoreset(dd, bc.DeviceProjector(mk_sampler(), S, model), opt_itrs=itrs, n_subsample_opt=nsub, **kw)
                alg.idcs = idcs.copy()
                key = '%s M=%d n_subsample_opt=%s' % (name, M, nsub)
                res['configs'][key] = per_gradient(ctx, alg, w0, p0, itrs, repeats) if not args.profile else None
                if args.profile:
                    alg.wts, alg.pts = w0.copy(), p0.copy()
                    np.random.seed(0)
                    alg._optimize()
                    ctx.sync()
                if has_feature:
                    want = (repeats + 1) * itrs if args.leg == 'on' else 0
                    assert alg.fused_gradient_calls == want, 'the fused route was taken %d times, expected %d' % (alg.fused_gradient_calls, want)
                if not args.profile:
                    v = res['configs'][key]
                    print('%s [%s]: %.4f ms per gradient (%.4f - %.4f)' % (key, args.leg, v['median_ms'], v['min_ms'], v['max_ms']), flush=True)
        del dd, t
    out = args.out or os.path.join(HERE, 'profiles', 'psvi_bench_%s.json' % args.leg)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps({'ok': True, 'out': out}))
    return 0


if __name__ == '__main__':
    sys.exit(main())
