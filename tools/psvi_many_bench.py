#!/usr/bin/env python3
"""The BatchPSVI evaluation curve -- pseudo-coresets of sizes 1 .. M, `opt_itrs` joint ADAM steps each -- by ONE batched device
run (BatchPSVICoreset.build_many(route='batched'), bc_psvi_many_*) beside the loop of single builds it replaces.

    python tools/psvi_many_bench.py [--dims 128,16] [--n 1000000] [--sizes 100] [--steps 500] [--loop-sizes 1,25,50,75,100]
                                    [--loop-steps 20] [--skip-loop] [--json out.json]
                                    [--model gauss [--f64] [--skip-batched] [--package-root DIR]]

Per D: N resident rows (float32 storage), S = 100, n_sub = 200, a LogisticLaplaceSampler(solver='newton') on its own stream.
  batched   one warm run of ONE step (buffers, code objects; its seam gives the Newton steps of the cold first fits), then the
            timed run of `--steps` steps: host wall clock around build_many, the GPU milliseconds of its chunks
            (bc_psvi_many_device_ms), and from the seam the Newton steps per fit after the first step.
  loop      the single builds the library already had -- build(1, m) with fused_gradient=True and the same sampler kind, same
            seeds -- on `--loop-sizes` for `--loop-steps` steps each (one warm build first): milliseconds per gradient step at each
            size, interpolated linearly over m = 1 .. M and scaled to `--steps` steps.  The whole loop is M x steps gradients
            (50 000 at the defaults): the subset is what is timed, the total is an extrapolation and is labelled so.
The per-stage split of a step is not measured here: run a short leg (--steps 50 --skip-loop) under a kernel trace and divide the
per-kernel totals by the step count (profiles/psvi_many_notes.md).

--model gauss: the Gaussian-location kind (profiles/psvi_many_gauss_notes.md) -- the model of examples/zellner_gaussian.py (Sigma =
500 I, prior N(0, I), steps 0.1 / (1 + i)), rows ~ N(0, Sigma) in float32 storage or, with --f64, float64, a
GaussianPosteriorSampler on its own stream; `--dims` are its dimensions.  The same two legs (no Newton statistics: the fit is a
closed form).  --skip-batched times the loop alone, and --package-root imports beta_cores_amd from another checkout: together they
time the loop of an earlier commit, which has no batched route for this model, with this file.  --post chains runs the batched
leg with BC_PSVI_POST=chains: the posterior stage's three products as bc_vi_sampler forms them, beside the matrix-core form."""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))
import numpy as np


def make_rows(n, d, seed=3):
    rng = np.random.RandomState(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    x[:, -1] = 1.
    th = rng.randn(d) / np.sqrt(d)
    y = np.where(rng.rand(n) < 1. / (1. + np.exp(-x.dot(th.astype(np.float32)))), 1., -1.).astype(np.float32)
    return y[:, None] * x


def coreset(bc, dd, d, s, n_sub, steps, seed):
    smp = bc.samplers.LogisticLaplaceSampler(np.zeros(d), rng=np.random.RandomState(seed), solver='newton')
    prj = bc.DeviceProjector(smp, s, bc.likelihoods.LogisticRegression())
    return bc.BatchPSVICoreset(dd, prj, opt_itrs=steps, n_subsample_opt=n_sub, fused_gradient=True)


def make_gauss_rows(n, d, f64, seed=3):
    x = np.sqrt(500.) * np.random.RandomState(seed).standard_normal((n, d))
    return x if f64 else x.astype(np.float32)


def gauss_coreset(bc, dd, d, s, n_sub, steps, seed):
    Sig = 500 * np.eye(d)
    Siginv = np.linalg.inv(Sig)
    smp = bc.samplers.GaussianPosteriorSampler(np.zeros(d), np.eye(d), Siginv, rng=np.random.RandomState(seed))
    prj = bc.DeviceProjector(smp, s, bc.likelihoods.GaussianLocation(Siginv, np.linalg.slogdet(Sig)[1]))
    return bc.BatchPSVICoreset(dd, prj, opt_itrs=steps, n_subsample_opt=n_sub, fused_gradient=True, step_sched=lambda m: lambda i: 0.1 / (1. + i))


def main_gauss(a):
    if a.package_root:
        sys.path.insert(0, os.path.abspath(a.package_root))
    import beta_cores_amd as bc
    bc.default_context()
    sizes = list(range(1, a.sizes + 1))
    out = []
    for d in [int(v) for v in a.dims.split(',')]:
        rows = make_gauss_rows(a.n, d, a.f64)
        dd = bc.DeviceData(rows) if a.f64 else bc.DeviceData(rows, dtype=np.float32)
        rec = {'model': 'gauss', 'post': a.post or 'matrix cores', 'D': d, 'N': a.n, 'S': a.samples, 'n_sub': a.n_sub, 'sizes': a.sizes, 'steps': a.steps, 'rows': 'float64' if a.f64 else 'float32',
               'package': os.path.dirname(os.path.dirname(os.path.abspath(bc.__file__)))}
        if not a.skip_batched:
            np.random.seed(5)
            gauss_coreset(bc, dd, d, a.samples, a.n_sub, 1, seed=5).build_many(sizes, route='batched')      # warm: buffers, code objects
            alg = gauss_coreset(bc, dd, d, a.samples, a.n_sub, a.steps, seed=5)
            np.random.seed(5)
            t0 = time.perf_counter()
            curve = alg.build_many(sizes, route='batched')
            rec['batched_wall_s'] = time.perf_counter() - t0
            rec['batched_device_ms'] = curve.device_ms
            rec['marked'] = curve.marked
            print('gauss D %3d: batched %d sizes x %d steps: wall %.3f s, GPU %.1f ms (%.3f ms per step); marked %s'
                  % (d, a.sizes, a.steps, rec['batched_wall_s'], curve.device_ms, curve.device_ms / a.steps, curve.marked or 'none'), flush=True)
        if not a.skip_loop:
            ms_at = {}
            for m in [int(v) for v in a.loop_sizes.split(',') if int(v) <= a.sizes]:
                for timed in (False, True):                   # (one warm build of the same shape first)
                    one = gauss_coreset(bc, dd, d, a.samples, a.n_sub, a.loop_steps, seed=5)
                    np.random.seed(5)
                    t0 = time.perf_counter()
                    one.build(1, m)
                    dt = time.perf_counter() - t0
                assert one.fused_gradient_calls == a.loop_steps
                ms_at[m] = 1e3 * dt / a.loop_steps
            ms = np.interp(sizes, sorted(ms_at), [ms_at[k] for k in sorted(ms_at)])
            rec['loop_ms_per_step_at'] = ms_at
            rec['loop_extrapolated_s'] = float(ms.sum() * a.steps / 1e3)
            print('gauss D %3d: loop of single builds (fused gradient), %d steps timed at m = %s: %s ms per step; extrapolated to %d sizes x %d '
                  'steps: %.1f s' % (d, a.loop_steps, sorted(ms_at), ['%.2f' % ms_at[k] for k in sorted(ms_at)], a.sizes, a.steps,
                                     rec['loop_extrapolated_s']), flush=True)
            if 'batched_wall_s' in rec:
                rec['speedup_extrapolated'] = rec['loop_extrapolated_s'] / rec['batched_wall_s']
                print('gauss D %3d: that is %.1f times the batched wall clock' % (d, rec['speedup_extrapolated']), flush=True)
        out.append(rec)
        del dd
    print(json.dumps({'psvi_many_gauss_bench': out}))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump({'psvi_many_gauss_bench': out}, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dims', default='128,16')
    ap.add_argument('--n', type=int, default=1_000_000)
    ap.add_argument('--sizes', type=int, default=100)
    ap.add_argument('--steps', type=int, default=500)
    ap.add_argument('--samples', type=int, default=100)
    ap.add_argument('--n-sub', type=int, default=200)
    ap.add_argument('--loop-sizes', default='1,25,50,75,100')
    ap.add_argument('--loop-steps', type=int, default=20)
    ap.add_argument('--skip-loop', action='store_true')
    ap.add_argument('--json', default=None)
    ap.add_argument('--model', default='logistic', choices=('logistic', 'gauss'))
    ap.add_argument('--f64', action='store_true')
    ap.add_argument('--skip-batched', action='store_true')
    ap.add_argument('--package-root', default=None)
    ap.add_argument('--post', default=None, choices=('chains',), help="gauss: BC_PSVI_POST for the run (the posterior stage's products by per-thread chains)")
    a = ap.parse_args()
    if a.model == 'gauss':
        if a.post:
            os.environ['BC_PSVI_POST'] = a.post
        return main_gauss(a)
    import beta_cores_amd as bc
    from beta_cores_amd.coreset import bpsvi
    bc.default_context()
    sizes = list(range(1, a.sizes + 1))
    out = []
    for d in [int(v) for v in a.dims.split(',')]:
        dd = bc.DeviceData(make_rows(a.n, d), dtype=np.float32)
        rec = {'D': d, 'N': a.n, 'S': a.samples, 'n_sub': a.n_sub, 'sizes': a.sizes, 'steps': a.steps}
        warm = coreset(bc, dd, d, a.samples, a.n_sub, 1, seed=5)
        np.random.seed(5)
        warm.build_many(sizes, route='batched')
        first = bpsvi.psvi_many_last_step(dd.ctx, sizes, d, a.samples)['newton'][:, 0]
        alg = coreset(bc, dd, d, a.samples, a.n_sub, a.steps, seed=5)
        np.random.seed(5)
        t0 = time.perf_counter()
        curve = alg.build_many(sizes, route='batched')
        rec['batched_wall_s'] = time.perf_counter() - t0
        rec['batched_device_ms'] = curve.device_ms
        rec['marked'] = curve.marked
        newton = bpsvi.psvi_many_last_step(dd.ctx, sizes, d, a.samples)['newton']
        rec['newton_first_fit_mean'] = float(first.mean())
        rec['newton_per_later_fit_mean'] = float((newton[:, 1] - first).mean() / max(a.steps - 1, 1))
        rec['newton_last_fit_max'] = int(newton[:, 0].max())
        print('D %3d: batched %d sizes x %d steps: wall %.3f s, GPU %.1f ms (%.3f ms per step); Newton steps: first fit %.1f, later fits %.2f on '
              'average; marked %s' % (d, a.sizes, a.steps, rec['batched_wall_s'], curve.device_ms, curve.device_ms / a.steps,
                                      rec['newton_first_fit_mean'], rec['newton_per_later_fit_mean'], curve.marked or 'none'), flush=True)
        if not a.skip_loop:
            ms_at = {}
            for m in [int(v) for v in a.loop_sizes.split(',') if int(v) <= a.sizes]:
                for timed in (False, True):                   # (one warm build of the same shape first)
                    one = coreset(bc, dd, d, a.samples, a.n_sub, a.loop_steps, seed=5)
                    np.random.seed(5)
                    t0 = time.perf_counter()
                    one.build(1, m)
                    dt = time.perf_counter() - t0
                assert one.fused_gradient_calls == a.loop_steps
                ms_at[m] = 1e3 * dt / a.loop_steps
            ms = np.interp(sizes, sorted(ms_at), [ms_at[k] for k in sorted(ms_at)])
            rec['loop_ms_per_step_at'] = ms_at
            rec['loop_extrapolated_s'] = float(ms.sum() * a.steps / 1e3)
            rec['speedup_extrapolated'] = rec['loop_extrapolated_s'] / rec['batched_wall_s']
            print('D %3d: loop of single builds (fused gradient), %d steps timed at m = %s: %s ms per step; extrapolated to %d sizes x %d '
                  'steps: %.1f s -- %.1f times the batched wall clock' % (d, a.loop_steps, sorted(ms_at), ['%.2f' % ms_at[k] for k in sorted(ms_at)],
                                                                        a.sizes, a.steps, rec['loop_extrapolated_s'], rec['speedup_extrapolated']), flush=True)
        out.append(rec)
        del dd
    print(json.dumps({'psvi_many_bench': out}))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump({'psvi_many_bench': out}, f, indent=1)


if __name__ == '__main__':
    main()
