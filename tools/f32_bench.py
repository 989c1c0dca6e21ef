#!/usr/bin/env python3
"""float32 data rows against float64 ones, measured in ONE process on one GPU (bench.py's data recipe and seeds, Zellner
linear regression, N = 10M, D = 128, S = 100 by default):

  (a) HilbertCoreset(ndarray, DeviceProjector) from a HOST array: construction and time to an M = 100 coreset, timed the way
      bench.py's from-host leg times them, for the float64 array, its astype(float32), and that array widened back
      (astype(float32).astype(float64): the same VALUES as the float32 run, stored as float64);
  (b) resident K1 by HIP events (kernel timer class 1), materialising and store-free, float64 and float32 rows interleaved;
  (c) resident bytes of Z;
  (d) the M = 100 selections: float32 run vs the widened-back run (must be equal), and vs the float64 run (reported only: the
      float32 array holds other numbers);
  and (b) for the logistic model at N = 1M, D = 128.

  python tools/f32_bench.py [--rows N] [--dim D] [--samples S] [--launches L] [--out profiles/f32_bench.json]

Every leg is checked; the first failure is recorded in the JSON and ends the run with a non-zero status."""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402  (the data recipe: gen_rows, posterior_samples)


def stats(xs):
    xs = np.asarray(xs, dtype=np.float64)
    return {'median_ms': float(np.median(xs)), 'min_ms': float(xs.min()), 'max_ms': float(xs.max()), 'n': int(xs.size)}


def k1_times(ctx, calls, launches, warm=3):
    """Per-launch HIP-event times of the K1 class for each callable in `calls`, launched in turn (interleaved)."""
    ctx.enable_timing(True)
    for _ in range(warm):
        for c in calls.values():
            c()
    ctx.sync()
    ctx.kernel_time_reset()
    out = {k: [] for k in calls}
    for _ in range(launches):
        for k, c in calls.items():
            ms0, n0 = ctx.kernel_time(1)
            c()
            ms1, n1 = ctx.kernel_time(1)
            if n1 != n0 + 1:
                raise RuntimeError('%s: expected one K1 launch, the timer saw %d' % (k, n1 - n0))
            out[k].append(ms1 - ms0)
    ctx.enable_timing(False)
    return {k: stats(v) for k, v in out.items()}


def from_host(bc, ctx, barrier, Z_host, theta, S, model, M=100):
    prj = bc.DeviceProjector(lambda k, w, p: theta, S, model, ctx=ctx)
    for rep in range(2):                   # the second pass is the one reported (buffers and code objects exist)
        barrier()
        t0 = time.perf_counter()
        alg = bc.HilbertCoreset(Z_host, prj, snnls=bc.snnls.GIGA)
        barrier()
        t_init = time.perf_counter() - t0
        alg.build(M, M)
        barrier()
        t_m = time.perf_counter() - t0
        tr = alg.snnls._eng.trace()[0].copy()
        idcs, wts = alg.idcs.copy(), alg.wts.copy()
        del alg
        gc.collect()
    return {'construct_ms': 1e3 * t_init, 'M100_ms': 1e3 * t_m}, (tr, idcs, wts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=10_000_000)
    ap.add_argument('--dim', type=int, default=128)
    ap.add_argument('--samples', type=int, default=100)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--logistic-rows', type=int, default=1_000_000)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'f32_bench.json'))
    args = ap.parse_args()
    import torch
    import beta_cores_amd as bc
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    ctx = bc.Context(device=0, stream=stream.cuda_stream)
    bc.set_default_context(ctx)

    def barrier():
        torch.cuda.synchronize(dev)
        ctx.sync()

    N, D, S = args.rows, args.dim, args.samples
    res = {'N': N, 'D': D, 'S': S, 'launches': args.launches, 'ok': False}
    state = {}

    def leg_data():
        g0 = torch.Generator(device=dev)
        g0.manual_seed(39)
        thstar = torch.randn((D,), generator=g0, dtype=torch.float64, device=dev)
        Z = bench.gen_rows(torch, dev, 0, N, D, thstar)
        torch.cuda.synchronize(dev)
        d64 = bc.DeviceData.from_torch(Z, ctx=ctx)
        state['theta'] = bench.posterior_samples(bc, d64, D, S, None)
        Z32 = Z.float()
        torch.cuda.synchronize(dev)
        state.update(Z=Z, Z32=Z32, d64=d64, d32=bc.DeviceData.from_torch(Z32, ctx=ctx))
        state['model'] = bc.likelihoods.LinearRegression(1.0)
        return {'Z_bytes_float64': state['d64'].nbytes, 'Z_bytes_float32': state['d32'].nbytes}

    def leg_resident_k1():
        prj = bc.DeviceProjector(lambda k, w, p: state['theta'], S, state['model'], ctx=ctx)
        d64, d32 = state['d64'], state['d32']
        mat = k1_times(ctx, {'float64': lambda: prj.project(d64), 'float32': lambda: prj.project(d32)}, args.launches)
        sf = k1_times(ctx, {'float64': lambda: prj.colsum(d64), 'float32': lambda: prj.colsum(d32)}, args.launches)
        out = {'materialising': mat, 'store_free': sf}
        for v in out.values():
            v['float64_spread_ms'] = v['float64']['max_ms'] - v['float64']['min_ms']
            v['float32_minus_float64_median_ms'] = v['float32']['median_ms'] - v['float64']['median_ms']
            v['float32_not_slower_than_spread'] = bool(v['float32_minus_float64_median_ms'] <= v['float64_spread_ms'])
        return out

    def leg_from_host():
        Zh64 = state['Z'].cpu().numpy()
        Zh32 = state['Z32'].cpu().numpy()
        for k in ('d64', 'd32', 'Z', 'Z32'):           # the resident copies are not needed any more
            state.pop(k)
        gc.collect()
        torch.cuda.empty_cache()
        out, sel = {}, {}
        out['float64'], sel['float64'] = from_host(bc, ctx, barrier, Zh64, state['theta'], S, state['model'])
        del Zh64
        gc.collect()
        out['float32'], sel['float32'] = from_host(bc, ctx, barrier, Zh32, state['theta'], S, state['model'])
        Zw = Zh32.astype(np.float64)
        del Zh32
        gc.collect()
        out['float32_widened_on_host'], sel['widened'] = from_host(bc, ctx, barrier, Zw, state['theta'], S, state['model'])
        del Zw
        gc.collect()
        same = lambda a, b: bool(all(np.array_equal(x, y) for x, y in zip(a, b)))
        out['construct_ratio_float32_over_float64'] = out['float32']['construct_ms'] / out['float64']['construct_ms']
        out['M100_ratio_float32_over_float64'] = out['float32']['M100_ms'] / out['float64']['M100_ms']
        out['float32_faster'] = bool(out['float32']['construct_ms'] < out['float64']['construct_ms'])
        out['selections_equal_float32_vs_widened'] = same(sel['float32'], sel['widened'])
        out['selections_equal_float32_vs_float64'] = same(sel['float32'], sel['float64'])
        if not out['selections_equal_float32_vs_widened']:
            raise RuntimeError('the float32 run selected differently from the same values stored as float64')
        return out

    def leg_logistic():
        n = args.logistic_rows
        g = torch.Generator(device=dev)
        g.manual_seed(50)
        X = torch.randn((n, D), generator=g, dtype=torch.float64, device=dev)
        w = torch.randn((D,), generator=g, dtype=torch.float64, device=dev)
        y = torch.where(torch.rand((n,), generator=g, dtype=torch.float64, device=dev) < torch.sigmoid(X @ w), 1., -1.)
        Z = (X * y[:, None]).contiguous()
        Z32 = Z.float()
        torch.cuda.synchronize(dev)
        theta = np.random.default_rng(41).standard_normal((S, D)) * 0.1
        prj = bc.DeviceProjector(lambda k, w_, p: theta, S, bc.likelihoods.LogisticRegression(), ctx=ctx)
        d64, d32 = bc.DeviceData.from_torch(Z, ctx=ctx), bc.DeviceData.from_torch(Z32, ctx=ctx)
        out = {'N': n, 'materialising': k1_times(ctx, {'float64': lambda: prj.project(d64), 'float32': lambda: prj.project(d32)},
                                                args.launches),
               'store_free': k1_times(ctx, {'float64': lambda: prj.colsum(d64), 'float32': lambda: prj.colsum(d32)}, args.launches)}
        return out

    rc = 0
    for name, leg in (('data', leg_data), ('resident_k1', leg_resident_k1), ('from_host', leg_from_host), ('logistic_k1', leg_logistic)):
        try:
            res[name] = leg()
            barrier()
        except Exception as e:      # the first failure ends the run: nothing more is started on the GPU
            res['failed_leg'] = name
            res['error'] = '%s: %s' % (type(e).__name__, e)
            rc = 1
            break
    res['ok'] = rc == 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(res, sort_keys=True))
    return rc


if __name__ == '__main__':
    sys.exit(main())
