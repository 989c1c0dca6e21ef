#!/usr/bin/env python3
"""The evaluation curve of the logistic drivers -- the posteriors of the weighted coresets of sizes 0 .. 100 -- sampled by
samplers.logistic_hmc_many with the per-chain warm-up (adapt='stan': include/beta_cores_hmc_adapt.h) beside the per-problem warm-up
in chunks (adapt='chunks'), in one process, alternating the two in every repeat.

    python tools/hmc_adapt_bench.py [--dims 128,16] [--sizes 100] [--chains 16] [--leapfrog 8] [--warmup 200] [--iters 200]
                                    [--reps 5] [--json out.json]

Problems: tools/hmc_many_bench.py's.  Every wall figure is a host clock around a call that returns with its results on the host,
after one warm call with the very arguments of the timed ones (so that no buffer grows inside the clock); every repeat is
recorded.  Per dimension and per inv_mass in (None, 'laplace' -- from
the batched Laplace fit, which is inside the clock):
  whole      logistic_hmc_many(warmup, iters, summary=True, keep_samples=False): wall seconds, the GPU milliseconds of all the
             chunk launches, the worst split-R-hat and the smallest ESS over the curve, and that ESS per wall second
  warmup     the same call with ONE kept iteration and a given start: the warm-up alone, but for that iteration; its chunk
             launches and host waits, COUNTED at the library's boundary (calls of *_chunk_begin and *_chunk_end), the kept
             iteration's one of each included
and per dimension
  stage      one chunk of `warmup` iterations three ways, GPU milliseconds of the launch: an ordinary chunk at a fixed step; a warm-up
             chunk whose plan has ONE window of ONE iteration (the rule admits none shorter from 20 iterations on): the
             dual averaging and the per-iteration barrier alone; a warm-up chunk with the default windows: the folds in addition"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))
sys.path.insert(0, HERE)
import numpy as np

from hmc_many_bench import make_problems


def spread(x):
    x = [float(v) for v in x]
    return {'min': min(x), 'median': float(np.median(x)), 'max': max(x), 'all': x}


class CallCounter:
    """Counts the library calls that samplers makes through _native.call, by name."""

    def __init__(self, native):
        self.native, self.inner, self.seen = native, native.call, {}

    def __enter__(self):
        def call(name, *args):
            self.seen[name] = self.seen.get(name, 0) + 1
            return self.inner(name, *args)
        self.native.call = call
        return self

    def __exit__(self, *exc):
        self.native.call = self.inner

    def launches_and_waits(self):
        return {'launches': sum(v for k, v in self.seen.items() if k.endswith('_chunk_begin')),
                'host_waits': sum(v for k, v in self.seen.items() if k.endswith('_chunk_end'))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dims', default='128,16')
    ap.add_argument('--sizes', type=int, default=100)
    ap.add_argument('--chains', type=int, default=16)
    ap.add_argument('--leapfrog', type=int, default=8)
    ap.add_argument('--warmup', type=int, default=200)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--step', type=float, default=0.004)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    import beta_cores_amd as bc
    from beta_cores_amd import _native as N
    from beta_cores_amd import samplers
    ctx = bc.default_context()
    out = []
    for d in [int(v) for v in a.dims.split(',')]:
        probs = make_problems(a.sizes, d)
        P, c = len(probs), a.chains
        start = np.random.RandomState(11).randn(c, d) * 0.05
        base = dict(n_chains=c, step_size=a.step, n_leapfrog=a.leapfrog, warmup=a.warmup, start=start)
        auto = int(N.load().bc_hmc_auto_chunk(c, d))
        r = {'D': d, 'P': P, 'C': c, 'L': a.leapfrog, 'warmup': a.warmup, 'iterations': a.iters, 'start_step': a.step, 'auto_chunk': auto}
        for mass in (None, 'laplace'):
            runs = {'whole': dict(base, n_samples=a.iters, inv_mass=mass, summary=True, keep_samples=False, laplace='batched'),
                    'warmup': dict(base, n_samples=1, inv_mass=mass, laplace='batched')}
            for what, kw in runs.items():
                rec = {m: {'wall_s': [], 'gpu_ms': [], 'worst_rhat': [], 'least_ess': [], 'accept': []} for m in ('stan', 'chunks')}
                for m in rec:      # the warm call, counted
                    with CallCounter(N) as counted:
                        samplers.logistic_hmc_many(probs, rng=np.random.RandomState(3), adapt=m, **kw)
                    rec[m]['calls'] = counted.launches_and_waits()
                for rep in range(a.reps):
                    for m in (('stan', 'chunks') if rep % 2 == 0 else ('chunks', 'stan')):
                        t0 = time.perf_counter()
                        res = samplers.logistic_hmc_many(probs, rng=np.random.RandomState(3 + rep), adapt=m, **kw)
                        rec[m]['wall_s'].append(time.perf_counter() - t0)
                        rec[m]['gpu_ms'].append(res.device_ms)
                        rec[m]['accept'].append(np.mean([x.accept_rate.mean() for x in res]))
                        if what == 'whole':
                            rec[m]['worst_rhat'].append(max(float(np.nanmax(x.summary.rhat)) for x in res))
                            rec[m]['least_ess'].append(min(float(np.nanmin(x.summary.ess)) for x in res))
                for m, v in rec.items():
                    s = {'wall_s': spread(v['wall_s']), 'gpu_ms': spread(v['gpu_ms']), 'kept_accept_rate': spread(v['accept']),
                         'chunk_launches_and_host_waits': v['calls']}
                    if what == 'whole':
                        s.update(worst_rhat=spread(v['worst_rhat']), least_ess=spread(v['least_ess']),
                                 ess_per_s=spread([e / w for e, w in zip(v['least_ess'], v['wall_s'])]))
                    r['%s_%s_%s' % (what, 'laplace' if mass else 'none', m)] = s
        # the cost of the adaptation stage: one chunk of `warmup` iterations, three ways
        rng = np.random.RandomState(5)
        e, u = rng.randn(a.warmup, c, d), np.log(rng.rand(a.warmup, c))
        starts, ims = np.ascontiguousarray(np.broadcast_to(start, (P, c, d))), np.ones((P, d))
        log_steps = np.full(P, np.log(a.step))
        stage = {'ordinary': [], 'stage_only': [], 'default_windows': []}
        for rep in range(a.reps + 1):      # (the first pass is the warm one)
            for how in stage:
                eng = samplers._DeviceHMCMany(ctx, samplers._small_problems(probs)[0])
                eng.begin(starts, ims, a.leapfrog, a.warmup)
                try:
                    if how == 'ordinary':
                        eng.chunk_scored(e, u, np.full(P, a.step), True, None, False)
                    else:
                        bufs = (a.warmup // 2, a.warmup - a.warmup // 2 - 1, 1) if how == 'stage_only' else (75, 50, 25)
                        N.call('bc_hmc_adapt_begin', ctx.h, samplers._ptr(log_steps), 0.8, 0.05, 10., 0.75, a.warmup, *bufs)
                        eng.adapt_chunk(e, u, True)
                finally:
                    ms = eng.end()
                if rep:
                    stage[how].append(ms)
        r['stage_gpu_ms'] = {k: spread(v) for k, v in stage.items()}
        r['stage_us_per_iteration_and_chain'] = {k: (min(stage[k]) - min(stage['ordinary'])) * 1e3 / (a.warmup * P * c)
                                                 for k in ('stage_only', 'default_windows')}
        out.append(r)
        print(json.dumps(r), flush=True)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
