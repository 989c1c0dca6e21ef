#!/usr/bin/env python3
"""The multi-chain logistic rows pass (k_lr_rows_mc) beside K5, and whole HMC runs on the device beside a Python loop.

    python tools/hmc_bench.py [--shapes 10000000x128,2000000x256] [--chains 1,16,32,64] [--reps 5] [--json out.json]

Rows pass: HIP events around the launches (timer class 6 = a logistic rows pass + its block-order reduction, the class K5 is
timed with), mean of `reps` after one warm-up call; gradient-only and with the value.  K5: one bc_logistic_newton_pass without
Hessian at the same rows; C chains cost C of them.  Fractions: of the HBM bound 8 N D bytes at 8 TB/s, and of the fp64 matrix
peak (4 N D C_padded flops: two contractions of 2 N D C each) at the 78.6 TFLOP/s spec, quoted at 2.4 GHz -- under fp64
matrix load the chip holds ~1.8 GHz, where no kernel exceeds 0.75 of that figure.
Whole run: wall time per HMC iteration of samplers.logistic_hmc against a loop that calls logistic_logjoint_batch once per
leapfrog step and does the leapfrog arithmetic in NumPy, on the same draws."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np
import torch

import beta_cores_amd as bc
from beta_cores_amd import posterior, samplers

HBM_PEAK = 8.0e12
FP64_MATRIX_PEAK = 78.6e12


def timed(ctx, fn, reps):
    fn()
    ctx.kernel_time_reset()
    for _ in range(reps):
        fn()
    ms, n = ctx.kernel_time(6)
    return ms / max(n, 1)


def make_rows(n, d):
    dev = torch.device('cuda', 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    Z = torch.randn((n, d), dtype=torch.float64, device=dev, generator=gen)
    ths = torch.randn(d, dtype=torch.float64, device=dev, generator=gen) * (2. / np.sqrt(d))
    y = torch.where(torch.rand(n, dtype=torch.float64, device=dev, generator=gen) < torch.sigmoid(Z @ ths), 1., -1.).to(torch.float64)
    Z.mul_(y[:, None])
    w = (torch.rand(n, dtype=torch.float64, device=dev, generator=gen) * 2.).cpu().numpy()
    torch.cuda.synchronize()
    return Z, ths.cpu().numpy(), w


def bench_pass(n, d, chains, reps):
    Z, ths, w = make_rows(n, d)
    ctx = bc.default_context()
    ctx.timing_classes(0x47)
    ctx.enable_timing(True)
    dz = bc.DeviceData.from_torch(Z, ctx=ctx)
    wd = posterior._weights_on_device(w, n, ctx)
    r = {'N': n, 'D': d}
    r['k5_ms'] = timed(ctx, lambda: bc.logistic_newton_pass(dz, ths * 0.5, w=wd, hessian=False), reps)
    r['k5_hbm_fraction'] = 8. * n * d / (r['k5_ms'] * 1e-3) / HBM_PEAK
    rng = np.random.RandomState(1)
    for c in chains:
        th = ths[None, :] * 0.5 + rng.randn(c, d) * (0.1 / np.sqrt(d))
        for value in (False, True):
            ms = timed(ctx, lambda: posterior.logistic_logjoint_batch(dz, th, wd, value=value), reps)
            k = 'c%d_%s' % (c, 'value' if value else 'grad')
            r[k + '_ms'] = ms
            r[k + '_ms_per_chain'] = ms / c
            r[k + '_over_k5_calls'] = ms / (c * r['k5_ms'])
            r[k + '_hbm_fraction'] = 8. * n * d / (ms * 1e-3) / HBM_PEAK
            r[k + '_mfma_fraction'] = 4. * n * d * (16 * ((c + 15) // 16)) / (ms * 1e-3) / FP64_MATRIX_PEAK
    ctx.enable_timing(False)
    del dz, wd, Z
    torch.cuda.empty_cache()
    return r


def python_loop(dz, wd, start, im, eps, L, E, logU):
    """The sampler of include/beta_cores_hmc.h with one logistic_logjoint_batch call per leapfrog step."""
    th = start.copy()
    lj, g = posterior.logistic_logjoint_batch(dz, th, wd)
    acc_n = 0
    for t in range(E.shape[0]):
        r = E[t] / np.sqrt(im)
        h0 = -lj + 0.5 * (im * r * r).sum(axis=1)
        r = r + 0.5 * eps * g
        thp = th + eps * (im * r)
        for l in range(1, L + 1):
            ljp, gp = posterior.logistic_logjoint_batch(dz, thp, wd, value=(l == L))
            if l < L:
                r = r + eps * gp
                thp = thp + eps * (im * r)
            else:
                r = r + 0.5 * eps * gp
        h1 = -ljp + 0.5 * (im * r * r).sum(axis=1)
        acc = np.logical_and(np.isfinite(h1), logU[t] < h0 - h1)
        th, g, lj = np.where(acc[:, None], thp, th), np.where(acc[:, None], gp, g), np.where(acc, ljp, lj)
        acc_n += int(acc.sum())
    return th, acc_n


def bench_run(n, d, c, L, T, eps):
    Z, ths, w = make_rows(n, d)
    ctx = bc.default_context()
    dz = bc.DeviceData.from_torch(Z, ctx=ctx)
    rng = np.random.RandomState(2)
    start, im = ths[None, :] + rng.randn(c, d) * 0.01, np.ones(d)
    out = {'N': n, 'D': d, 'C': c, 'L': L, 'T': T, 'step': eps}
    for rep in range(2):                                 # (the first round warms both paths up)
        t0 = time.perf_counter()
        res = samplers.logistic_hmc(dz, w, n_samples=T, n_chains=c, step_size=eps, n_leapfrog=L, inv_mass=im, start=start,
                                    rng=np.random.RandomState(3))
        out['device_run_ms_per_iteration'] = (time.perf_counter() - t0) * 1e3 / T
        out['device_run_gpu_ms_per_iteration'] = res.device_ms / T
        r = np.random.RandomState(3)
        E, U = r.randn(T, c, d), np.log(r.rand(T, c))
        wd = posterior._weights_on_device(w, n, ctx)
        t0 = time.perf_counter()
        th, acc_n = python_loop(dz, wd, start, im, eps, L, E, U)
        out['python_loop_ms_per_iteration'] = (time.perf_counter() - t0) * 1e3 / T
    out['accept_rate'] = float(res.accept_rate.mean())
    out['same_decisions'] = bool(acc_n == int(res.accept.sum()))
    out['final_position_max_abs_diff'] = float(np.abs(th - res.samples[-1]).max())
    del dz, Z
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='10000000x128,2000000x256')
    ap.add_argument('--chains', default='1,16,32,64')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--runs', default='10000000x128x16x8x3,1000x128x16x8x200')      # N x D x C x L x T
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    out = {'rows_pass': [], 'runs': []}
    for s in [v for v in a.shapes.split(',') if v]:
        n, d = (int(v) for v in s.split('x'))
        r = bench_pass(n, d, [int(v) for v in a.chains.split(',')], a.reps)
        out['rows_pass'].append(r)
        print(json.dumps(r), flush=True)
    for s in [v for v in a.runs.split(',') if v]:
        n, d, c, L, T = (int(v) for v in s.split('x'))
        r = bench_run(n, d, c, L, T, 0.5 / np.sqrt(n))
        out['runs'].append(r)
        print(json.dumps(r), flush=True)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
