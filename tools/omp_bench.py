#!/usr/bin/env python3
"""OrthoPursuit with the NNLS refit on the host (SciPy, bc.snnls.OrthoPursuit) against the refit on the device
(bc.snnls.DeviceOrthoPursuit), measured in ONE process on one GPU over the same resident Phi:

  Phi        seeded, 1M x 100 by default: the correlated recipe of tests/test_gpu_snnls.py::test_seeded_parity_vs_oracle
             (rank-12 part + 0.3 noise, rows centred), uploaded once
  for M in {25, 50, 100}:
    wall time of build(M) from an empty solver (reset() before each repeat), host refit and device refit: one warm-up
    build, then the median / min / max of `--repeats` timed ones, each closed by a stream synchronisation
    step kernel time of the device path from the library's kernel timers (class 5, a pass of its own with timing on)
    solves per refit from bc_snnls_refit_stats
    whether the two runs selected the same rows, and the largest relative weight difference

  python tools/omp_bench.py [--rows N] [--samples S] [--repeats R] [--out profiles/omp_bench.json]

The host path is not touched by the device refit, so its figure stands for the library before it, in the same run."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def stats(xs):
    xs = np.asarray(xs, dtype=np.float64)
    return {'median_ms': float(np.median(xs)), 'min_ms': float(xs.min()), 'max_ms': float(xs.max()), 'n': int(xs.size)}


def timed_builds(ctx, solver, M, repeats):
    out = []
    for rep in range(repeats + 1):                  # the first one warms up (code objects, buffers, SciPy's import)
        solver.reset()
        ctx.sync()
        t0 = time.perf_counter()
        solver.build(M)
        ctx.sync()
        if rep:
            out.append(1e3 * (time.perf_counter() - t0))
    return stats(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=1_000_000)
    ap.add_argument('--samples', type=int, default=100)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'omp_bench.json'))
    args = ap.parse_args()
    import beta_cores_amd as bc
    ctx = bc.default_context()
    N, S = args.rows, args.samples
    rng = np.random.RandomState(11)
    mix = rng.randn(12, S)
    phi = np.empty((N, S))
    for lo in range(0, N, 100_000):                  # in slabs: the temporaries stay small
        hi = min(N, lo + 100_000)
        blk = rng.randn(hi - lo, 12).dot(mix) + 0.3 * rng.randn(hi - lo, S)
        phi[lo:hi] = blk - blk.mean(axis=1)[:, None]
    dphi = bc.DevicePhi.from_host(phi)
    b = dphi.colsum()
    del phi
    host = bc.snnls.OrthoPursuit(dphi.T, b)
    dev = bc.snnls.DeviceOrthoPursuit(dphi.T, b)
    res = {'N': N, 'S': S, 'repeats': args.repeats, 'prefilter': dev._eng.prefilter, 'prefilter_form': dev._eng.prefilter_form, 'M': {}}
    for M in (25, 50, 100):
        leg = {'host_refit_build': timed_builds(ctx, host, M, args.repeats)}
        leg['device_refit_build'] = timed_builds(ctx, dev, M, args.repeats)
        leg['speedup_median'] = leg['host_refit_build']['median_ms'] / leg['device_refit_build']['median_ms']
        ih, vh = host.sparse_weights()
        idv, vd = dev.sparse_weights()
        leg['same_rows'] = bool(np.array_equal(ih, idv))
        leg['selected'] = int(idv.shape[0])
        leg['max_rel_weight_diff'] = float(np.abs(vd / vh - 1.).max()) if leg['same_rows'] else None
        leg['error_host'], leg['error_device'] = host.error(), dev.error()
        # step kernel (select-from-record + refit + guard + prep) by HIP events, in a pass of its own
        r0, s0, _ = dev._eng.refit_stats()
        ctx.timing_classes(0x3f)
        ctx.enable_timing(True)
        ctx.kernel_time_reset()
        dev.reset()
        dev.build(M)
        ctx.sync()
        ms, n = ctx.kernel_time(5)
        ms3, n3 = ctx.kernel_time(3)
        ms0, n0 = ctx.kernel_time(0)
        ctx.enable_timing(False)
        ctx.timing_classes(0x7)
        r1, s1, rej = dev._eng.refit_stats()
        leg['step_kernel_mean_us'] = 1e3 * ms / max(1, n)
        leg['step_kernel_launches'] = int(n)
        leg['sweep_mean_us'] = 1e3 * ms0 / max(1, n0)
        leg['rescore_mean_us'] = 1e3 * ms3 / max(1, n3)
        leg['solves_per_refit'] = (s1 - s0) / max(1, r1 - r0)
        leg['rejected_total'] = int(rej)
        res['M'][str(M)] = leg
        print('M = %3d  host refit %9.2f ms   device refit %8.2f ms   x%.1f   step kernel %.1f us   solves/refit %.2f   same rows %s'
              % (M, leg['host_refit_build']['median_ms'], leg['device_refit_build']['median_ms'], leg['speedup_median'],
                 leg['step_kernel_mean_us'], leg['solves_per_refit'], leg['same_rows']), flush=True)
    res['ok'] = all(leg['same_rows'] for leg in res['M'].values())      # recorded, not enforced: at M = S the error is at rounding level
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps({'ok': res['ok'], 'out': args.out}))
    return 0


if __name__ == '__main__':
    sys.exit(main())
