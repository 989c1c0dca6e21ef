#!/usr/bin/env python3
"""Full-data logistic Laplace fit on the device: the rows pass (K5), its Hessian (K4 without a y column) beside plain weighted
K4 on the same rows, whole fits with both solvers, and the host routine on a 1M-row copy for scale.

    python tools/laplace_bench.py [--shapes 10000000x128,2000000x512] [--reps 5] [--json out.json]

Kernel times are HIP events around the launches (timer classes 6 = rows pass + block-order reduction, 2 = K4 Gram + its
reduction), after one warm-up call; fits and the host routine by a synchronised host clock.  HBM fraction of the rows pass:
8 N D bytes over the measured time against the 8 TB/s peak (the measured copy rate is ~6.3 TB/s)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np
import torch

import beta_cores_amd as bc
from beta_cores_amd import samplers

HBM_PEAK = 8.0e12


def timed(ctx, which, fn, reps):
    fn()
    ctx.kernel_time_reset()
    for _ in range(reps):
        fn()
    ms, n = ctx.kernel_time(which)
    return ms / max(n, 1)


def bench(n, d, reps, host_rows):
    dev = torch.device('cuda', 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    Z = torch.randn((n, d), dtype=torch.float64, device=dev, generator=gen)
    ths = torch.randn(d, dtype=torch.float64, device=dev, generator=gen) * (2. / np.sqrt(d))
    y = torch.where(torch.rand(n, dtype=torch.float64, device=dev, generator=gen) < torch.sigmoid(Z @ ths), 1., -1.).to(torch.float64)
    Z.mul_(y[:, None])
    del y
    w = (torch.rand(n, dtype=torch.float64, device=dev, generator=gen) * 2.).cpu().numpy()
    torch.cuda.synchronize()
    ctx = bc.default_context()
    ctx.timing_classes(0x47)
    ctx.enable_timing(True)
    dz = bc.DeviceData.from_torch(Z, ctx=ctx)
    wd = bc.posterior._weights_on_device(w, n, ctx)
    th = ths.cpu().numpy() * 0.5
    r = {'N': n, 'D': d}
    r['rows_pass_ms'] = timed(ctx, 6, lambda: bc.logistic_newton_pass(dz, th, w=wd, hessian=False), reps)
    r['rows_pass_hbm_fraction'] = 8. * n * d / (r['rows_pass_ms'] * 1e-3) / HBM_PEAK
    r['rows_pass_diag_ms'] = timed(ctx, 6, lambda: bc.logistic_newton_pass(dz, th, w=wd, hessian=False, diag=True), reps)
    r['hessian_ms'] = timed(ctx, 2, lambda: bc.logistic_newton_pass(dz, th, w=wd, hessian=True), reps)
    # plain weighted K4 over the same rows (the last column taken as y: one column fewer in the Gram, the same tiles)
    r['k4_weighted_same_rows_ms'] = timed(ctx, 2, lambda: bc.weighted_gram(dz, w), reps)
    r['hessian_over_k4'] = r['hessian_ms'] / r['k4_weighted_same_rows_ms']
    t0 = time.perf_counter()
    bc.logistic_newton_pass(dz, th, w=wd, hessian=True)
    r['newton_pass_wall_ms'] = (time.perf_counter() - t0) * 1e3
    ctx.enable_timing(False)

    calls = {'n': 0}
    real = samplers.logistic_newton_pass

    def counting(*a, **k):
        calls['n'] += 1
        return real(*a, **k)
    samplers.logistic_newton_pass = counting
    try:
        for solver in ('newton', 'bfgs'):
            samplers.logistic_laplace(w, dz, np.zeros(d), solver=solver)       # warm-up
            calls['n'] = 0
            t0 = time.perf_counter()
            mu = samplers.logistic_laplace(w, dz, np.zeros(d), solver=solver)[0]
            r['fit_%s_ms' % solver] = (time.perf_counter() - t0) * 1e3
            r['fit_%s_passes' % solver] = calls['n']
            r['fit_%s_mu_norm' % solver] = float(np.linalg.norm(mu))
    finally:
        samplers.logistic_newton_pass = real
    if host_rows:
        m = min(host_rows, n)
        Zh, wh = Z[:m].cpu().numpy(), w[:m]
        t0 = time.perf_counter()
        samplers.logistic_laplace(wh, Zh, np.zeros(d), solver='newton')
        r['host_newton_%d_rows_ms' % m] = (time.perf_counter() - t0) * 1e3
        del Zh
    del dz, wd, Z
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='10000000x128,2000000x512')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host-rows', type=int, default=1_000_000)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    out = []
    for s in a.shapes.split(','):
        n, d = (int(v) for v in s.split('x'))
        r = bench(n, d, a.reps, a.host_rows)
        out.append(r)
        print(json.dumps(r), flush=True)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
