"""Measurements of the chain summary (include/beta_cores_diag.h) for profiles/diag_notes.md.  One JSON line per measurement.

  --part a   the summary alone, stand-alone: 101 coresets x 200 kept iterations x 16 chains at D = 128 and D = 16 (the README's
             curve) and 2 000 problems of 64 x 16 x 9 (tmc_shapley's shape).  Device: the wall time of chain_summary (upload of
             the samples, kernels, copies of the results).  Host: the NumPy float64 restatement below with the threads the
             environment gives (OMP_NUM_THREADS is printed), PLUS a device-to-host copy of the samples, which is what a run
             without the summary has to make to obtain the same numbers.
  --part b   the added cost inside a sampler run: logistic_hmc_many(score=held, keep_samples=False) with and without
             summary=True at the same shapes; wall and device_ms (the sampler's chunks), the ratio, and the wall time of the
             summary's end.
  --part c   the covariance kernel alone at D = 128: its GPU time over --reps calls from `rocprofv3 --kernel-trace --stats` run
             around `--part c` (in a run of its own), against 2 N D^2 / 2 executed flops (the tiles on or above the diagonal,
             padded to 16) and the 78.6 TF fp64 matrix spec figure of DESIGN.md.

NumPy restatement (numpy_summary): the header's definitions, vectorised over problems and coordinates, float64, every lag up to
n // 2 - 1 evaluated (NumPy has no early exit per coordinate; the device stops at the first non-positive pair)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.score_bench import make_problems, make_test      # noqa: E402  (the curve and the held-out rows of the score figures)


def numpy_summary(x, max_lag=None):
    """x: P x n x C x D float64 -> (mean, cov, rhat, ess) by the header's definitions"""
    P, n, c, d = x.shape
    h, N, S = n // 2, n * c, 2 * c
    flat = x.reshape(P, N, d)
    mean = flat.mean(axis=1)
    cen = flat - mean[:, None]
    cov = np.matmul(cen.transpose(0, 2, 1), cen) / (N - 1)
    seq = np.concatenate((x[:, :h], x[:, n - h:]), axis=2)      # P x h x 2C x D (the order of the sequences does not matter to the sums)
    m = seq.mean(axis=1)
    t = seq - m[:, None]
    v = (t * t).sum(axis=1) / (h - 1)
    W = v.mean(axis=1)
    Bh = m.var(axis=1, ddof=1)
    vp = (h - 1.) / h * W + Bh
    with np.errstate(invalid='ignore', divide='ignore'):
        rhat = np.sqrt(vp / W)
        L = h - 1 if max_lag is None else min(max_lag, h - 1)
        rho = np.ones((L + 1, P, d))
        for lag in range(1, L + 1):
            ab = ((t[:, :h - lag] * t[:, lag:]).sum(axis=1) / h).mean(axis=1)
            rho[lag] = 1. - (W - ab) / vp
        pairs = (L + 1) // 2
        Pk = rho[0:2 * pairs:2] + rho[1:2 * pairs:2]
        alive = np.logical_and.accumulate(Pk > 0, axis=0)
        mono = np.minimum.accumulate(np.where(alive, Pk, np.inf), axis=0)
        tau = -1. + 2. * np.where(alive, mono, 0.).sum(axis=0)
        ess = np.where(alive[0], S * h / tau, np.nan)
    return mean, cov, rhat, ess


def shapes(a):
    out = []
    for d in [int(s) for s in a.dims.split(',')]:
        out.append(('curve D=%d' % d, a.sizes + 1, a.iters, a.chains, d))
    out.append(('tmc_shapley shape', a.problems, 64, 16, 9))
    return out


def ar_samples(P, n, c, d, phi=0.6, seed=3):
    rng = np.random.RandomState(seed)
    x = np.empty((P, n, c, d))
    x[:, 0] = rng.randn(P, c, d)
    for i in range(1, n):
        x[:, i] = phi * x[:, i - 1] + np.sqrt(1. - phi * phi) * rng.randn(P, c, d)
    return x


def part_a(a):
    import beta_cores_amd as bc
    ctx = bc.default_context()
    for name, P, n, c, d in shapes(a):
        x = ar_samples(P, n, c, d)
        bc.samplers.chain_summary(x[:1], ctx=ctx)
        bc.samplers.chain_summary(x, ctx=ctx)                  # (grows the work space once)
        walls = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            s = bc.samplers.chain_summary(x, ctx=ctx)
            walls.append(time.perf_counter() - t0)
        import torch
        dev = torch.from_numpy(x).cuda()
        torch.cuda.synchronize()
        copies = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            back = dev.cpu()
            copies.append(time.perf_counter() - t0)
        hosts = []
        for _ in range(max(1, a.reps // 2)):
            t0 = time.perf_counter()
            ref = numpy_summary(back.numpy())
            hosts.append(time.perf_counter() - t0)
        ok = np.isfinite(ref[3]) & np.isfinite(s.ess)
        r = dict(part='a', shape=name, P=P, n=n, C=c, D=d, device_wall_ms=1e3 * min(walls), d2h_copy_ms=1e3 * min(copies), numpy_ms=1e3 * min(hosts),
                 host_total_ms=1e3 * (min(copies) + min(hosts)), speedup=(min(copies) + min(hosts)) / min(walls),
                 max_rel_mean=float(np.max(np.abs(s.mean - ref[0]) / (1e-300 + np.abs(ref[0])))),
                 max_rel_ess=float(np.max(np.abs(s.ess[ok] / ref[3][ok] - 1.))) if ok.any() else None,
                 worst_rhat=float(np.nanmax(s.rhat)), threads=os.environ.get('OMP_NUM_THREADS'))
        print(json.dumps(r), flush=True)


def part_b(a):
    import beta_cores_amd as bc
    for name, P, n, c, d in shapes(a):
        if name.startswith('curve'):
            probs = make_problems(P - 1, d)
            step = 0.004
        else:
            rng = np.random.RandomState(5)
            probs = []
            for p in range(P):
                m = 1 + (p % 20) * 25
                z = rng.randn(m, d)
                z[:, -1] = 1.
                probs.append((z * np.where(rng.rand(m) < 0.5, 1., -1.)[:, None], None))
            step = 0.05
        Xt, Yt, _ = make_test(a.test_rows, d)
        held = bc.samplers.HeldOut(Xt, Yt)
        rng = np.random.RandomState(11)
        kw = dict(n_samples=n, n_chains=c, step_size=step, n_leapfrog=a.leapfrog, inv_mass=np.ones(d), start=rng.randn(c, d) * 0.05, warmup=a.warmup,
                  score=held, keep_samples=False)
        out = {}
        for summary in (False, True, False, True):
            t0 = time.perf_counter()
            res = bc.samplers.logistic_hmc_many(probs, rng=np.random.RandomState(2), summary=summary, **kw)
            wall = time.perf_counter() - t0
            key = 'with' if summary else 'without'
            if key not in out or wall < out[key][0]:
                out[key] = (wall, res.device_ms, res)
        with_, without = out['with'], out['without']
        rh = np.array([r.summary.worst_rhat() for r in with_[2]])
        es = np.array([r.summary.least_ess() for r in with_[2]])
        r = dict(part='b', shape=name, P=len(probs), n=n, C=c, D=d, wall_without_ms=1e3 * without[0], wall_with_ms=1e3 * with_[0],
                 ratio=with_[0] / without[0], sampler_device_ms_without=without[1], sampler_device_ms_with=with_[1],
                 added_ms=1e3 * (with_[0] - without[0]), worst_rhat=float(np.nanmax(rh)), least_ess=float(np.nanmin(es)),
                 same_scores=bool(all(np.array_equal(x.correct, y.correct) for x, y in zip(with_[2], without[2]))))
        print(json.dumps(r), flush=True)


def part_c(a):
    import beta_cores_amd as bc
    P, n, c, d = a.sizes + 1, a.iters, a.chains, 128
    x = ar_samples(P, n, c, d)
    for _ in range(a.reps + 1):
        bc.samplers.chain_summary(x)
    N = n * c
    tiles = (d // 16) * (d // 16 + 1) // 2
    print(json.dumps(dict(part='c', P=P, N=N, D=d, calls=a.reps + 1, executed_flops_per_call=2. * P * N * tiles * 256,
                          spec_tf=78.6, note='k_diag_cov share = executed_flops_per_call / (its average time from the kernel stats) / 78.6e12')),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', default='a', choices=['a', 'b', 'c'])
    ap.add_argument('--dims', default='128,16')
    ap.add_argument('--sizes', type=int, default=100)
    ap.add_argument('--chains', type=int, default=16)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--problems', type=int, default=2000)
    ap.add_argument('--leapfrog', type=int, default=8)
    ap.add_argument('--warmup', type=int, default=100)
    ap.add_argument('--test-rows', type=int, default=2000)
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()
    {'a': part_a, 'b': part_b, 'c': part_c}[a.part](a)


if __name__ == '__main__':
    main()
