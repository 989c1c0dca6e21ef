#!/usr/bin/env python3
"""Sub-sampling resident rows on the device (DeviceData.take / k_take_rows), measured on one GPU over a resident
N x 129 data set (10M rows by default), stored as float64 and as float32:

  (a) take() of m = 1e4 .. 1e7 random rows into a re-used buffer: GPU time of the call between two events on the
      context's stream (index upload + k_take_rows), the GPU time of a pinned host -> device copy of the same m indices
      (so: kernel ~ call - index copy), and a device-to-device copy of as many bytes as the gather writes, on the same box;
      rows() (bc_data_gather_rows: rows to the host as doubles) at m = 1e4 for comparison
  (b) one sub-sampled gradient of SparseVICoreset (linear regression, S = 100, a coreset of 100 rows) at
      n_subsample_opt = 1e5 and 1e6: wall time per gradient over `--grads` gradients after a warm-up run
  (c) HilbertCoreset(data, prj, n_subsample=1e6): wall time of the construction
  (d) the short-row form of the kernel: take() of 1e6 and 1e7 random rows of a resident N x 3 set (the Gaussian model's
      rows: 24 / 12 bytes), measured like (a)

  python tools/take_bench.py [--rows N] [--legs abcd] [--root TREE] [--baseline FILE] [--out profiles/take_bench.json]

--root TREE imports the package from another (built) checkout, e.g. the commit before take() existed: the tool then
measures what that tree offers -- (a) rows() only, (b) and (c) through the host detour.  --baseline FILE merges the JSON of
such a run into this run's output, with the ratios.  --tables-from FILE needs no GPU: it prints the tables of
profiles/take_notes.md from such a JSON file."""
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


def gpu_ms(torch, fn, repeats):
    """GPU time of fn() between two events on the current stream; one warm-up call first."""
    out = []
    for rep in range(repeats + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if rep:
            out.append(a.elapsed_time(b))
    return med(out)


def wall_ms(ctx, fn, repeats):
    out = []
    for rep in range(repeats + 1):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        if rep:
            out.append(1e3 * (time.perf_counter() - t0))
    return med(out)


def take_leg(torch, ctx, dd, t, rng, ms, repeats, label):
    """take() of m random rows of dd (borrowing tensor t) for m in ms: see (a) in the module docstring."""
    n, row_bytes = t.shape[0], t.shape[1] * t.element_size()
    out, buf = {}, None
    for m in ms:
        if m > n:
            continue
        idx = rng.randint(n, size=m)
        buf = dd.take(idx, out=buf)
        call = gpu_ms(torch, lambda: dd.take(idx, out=buf), repeats)
        wall = wall_ms(ctx, lambda: dd.take(idx, out=buf), repeats)
        pinned = torch.from_numpy(idx).pin_memory()
        didx = torch.empty(m, dtype=torch.int64, device='cuda')
        h2d = gpu_ms(torch, lambda: didx.copy_(pinned, non_blocking=True), repeats)
        src = t[:m]
        dst = torch.empty_like(src)
        d2d = gpu_ms(torch, lambda: dst.copy_(src), repeats)
        moved = 2. * m * row_bytes                      # read + written, as for the copy
        kern = max(call['median_ms'] - h2d['median_ms'], 1e-6)
        out[str(m)] = {
            'call_gpu': call, 'call_wall': wall, 'index_h2d_gpu': h2d, 'd2d_copy_gpu': d2d,
            'kernel_ms_est': kern, 'kernel_TBps_est': moved / kern / 1e9, 'call_TBps': moved / call['median_ms'] / 1e9,
            'd2d_TBps': moved / d2d['median_ms'] / 1e9, 'kernel_over_copy_rate': d2d['median_ms'] / kern}
        print('%s take m=%-9d call %.3f ms (wall %.3f)  idx copy %.3f ms  kernel ~%.3f ms = %.2f TB/s   d2d copy %.3f ms = %.2f TB/s'
              % (label, m, call['median_ms'], wall['median_ms'], h2d['median_ms'], kern, moved / kern / 1e9,
                 d2d['median_ms'], moved / d2d['median_ms'] / 1e9), flush=True)
        del dst, didx, pinned
    return out


def tables(res):
    """The markdown tables of profiles/take_notes.md from a result object."""
    out = []
    base = res.get('baseline')
    for name, leg in sorted(res['dtypes'].items(), reverse=True):
        for key, dz in (('take', res['dz']), ('take_short_rows_dz3', 3)):
            if not leg.get(key):
                continue
            out += ['', '`take()`, %s rows of %d columns (%d bytes); GPU time, median of %d:'
                    % (name, dz, dz * (8 if name == 'float64' else 4), next(iter(leg[key].values()))['call_gpu']['n']), '',
                    '| m | call (index copy + kernel) | index copy alone | kernel = difference | kernel rate | copy of the same bytes | copy rate | kernel / copy | call, wall clock |',
                    '|---|---|---|---|---|---|---|---|---|']
            for m, t in sorted(leg[key].items(), key=lambda kv: int(kv[0])):
                out.append('| %s | %.3f ms | %.3f ms | %.3f ms | %.2f TB/s | %.3f ms | %.2f TB/s | %.2f | %.3f ms |' % (
                    '{:,}'.format(int(m)).replace(',', ' '), t['call_gpu']['median_ms'], t['index_h2d_gpu']['median_ms'], t['kernel_ms_est'],
                    t['kernel_TBps_est'], t['d2d_copy_gpu']['median_ms'], t['d2d_TBps'], t['kernel_over_copy_rate'], t['call_wall']['median_ms']))
    if base:
        out += ['', 'Against the previous commit (same box, same run; wall clock, median):', '',
                '| rows | what | previous commit | this commit | ratio |', '|---|---|---|---|---|']
        for name, leg in sorted(res['dtypes'].items(), reverse=True):
            b = base['dtypes'][name]
            if '10000' in leg.get('take', {}):
                p, t = b['rows_to_host_1e4']['median_ms'], leg['take']['10000']['call_wall']['median_ms']
                out.append('| %s | 10 000 rows: `rows()` to the host / `take()` | %.3f ms | %.3f ms | %.1f |' % (name, p, t, p / t))
            for m, v in sorted(leg['gradient'].items(), key=lambda kv: int(kv[0])):
                p = b['gradient'][m]['median_ms']
                out.append('| %s | one gradient, `n_subsample_opt` = %s | %.2f ms | %.2f ms | %.1f |'
                           % (name, '{:,}'.format(int(m)).replace(',', ' '), p, v['median_ms'], p / v['median_ms']))
            if 'hilbert_construct_1e6' in leg:
                p, t = b['hilbert_construct_1e6']['median_ms'], leg['hilbert_construct_1e6']['median_ms']
                out.append('| %s | `HilbertCoreset(n_subsample=1 000 000)` construction | %.1f ms | %.1f ms | %.1f |' % (name, p, t, p / t))
    return '\n'.join(out) + '\n'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tables-from', default=None)
    ap.add_argument('--rows', type=int, default=10_000_000)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--grads', type=int, default=3)
    ap.add_argument('--legs', default='abcd')
    ap.add_argument('--root', default=HERE)
    ap.add_argument('--baseline', default=None)
    ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'take_bench.json'))
    args = ap.parse_args()
    if args.tables_from:
        sys.stdout.write(tables(json.load(open(args.tables_from))))
        return 0
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import beta_cores_amd as bc
    assert os.path.abspath(os.path.dirname(os.path.dirname(bc.__file__))) == os.path.abspath(args.root)
    # the library launches on torch's current stream, so torch's events bracket its work
    stream = torch.cuda.Stream()                          # (not the null stream: its handle is what the context is bound to)
    torch.cuda.set_stream(stream)
    ctx = bc.Context(stream=stream.cuda_stream)
    bc.set_default_context(ctx)
    has_take = hasattr(bc.DeviceData, 'take')
    n, D, S = args.rows, 128, 100
    dz = D + 1
    res = {'N': n, 'dz': dz, 'S': S, 'has_take': has_take, 'device': torch.cuda.get_device_name(0), 'dtypes': {}}
    rng = np.random.RandomState(3)
    gen = torch.Generator(device='cuda').manual_seed(3)
    t64 = torch.randn((n, dz), dtype=torch.float64, device='cuda', generator=gen)
    for name, t in (('float64', t64), ('float32', None)):
        if t is None:
            t = t64.to(torch.float32)
            del t64
        dd = bc.DeviceData.from_torch(t, ctx=ctx)
        leg = {'take': {}, 'gradient': {}}
        # ---- (a)
        idx = rng.randint(n, size=10_000)
        leg['rows_to_host_1e4'] = wall_ms(ctx, lambda: dd.rows(idx), args.repeats)
        if has_take and 'a' in args.legs:
            leg['take'] = take_leg(torch, ctx, dd, t, rng, (10_000, 100_000, 1_000_000, 10_000_000), args.repeats, name)
        # ---- (b)
        core_idx = rng.choice(n, 100, replace=False)
        core = dd.rows(core_idx)
        for m in (100_000, 1_000_000):
            if m > n or 'b' not in args.legs:
                continue
            prj = bc.DeviceProjector(bc.samplers.LinregPosteriorSampler(np.zeros(D), np.eye(D), 1.0), S, bc.likelihoods.LinearRegression(1.0))
            np.random.seed(7)
            alg = bc.SparseVICoreset(dd, prj, n_subsample_select=1000, n_subsample_opt=m, opt_itrs=args.grads,
                                     step_sched=lambda i: 1e-6 / (1. + i), wts=np.full(100, n / 100.), idcs=core_idx.copy(), pts=core.copy())
            w0 = alg.wts.copy()
            times = []
            for rep in range(3):                              # the first run warms up (buffers, code objects)
                alg.wts = w0.copy()
                ctx.sync()
                t0 = time.perf_counter()
                alg._optimize()
                ctx.sync()
                if rep:
                    times.append(1e3 * (time.perf_counter() - t0) / args.grads)
            leg['gradient'][str(m)] = med(times)
            print('%s gradient n_subsample_opt=%-8d %.2f ms per gradient' % (name, m, np.median(times)), flush=True)
            del alg, prj
        # ---- (c)
        m = min(n, 1_000_000)
        th = rng.randn(S, D) * 0.1
        prj = bc.DeviceProjector(lambda k, w, p: th, S, bc.likelihoods.LinearRegression(1.0))

        def hilbert():
            np.random.seed(9)
            bc.HilbertCoreset(dd, prj, n_subsample=m)
        if 'c' in args.legs:
            leg['hilbert_construct_1e6'] = wall_ms(ctx, hilbert, 3)
            print('%s HilbertCoreset(n_subsample=%d) construction %.2f ms' % (name, m, leg['hilbert_construct_1e6']['median_ms']), flush=True)
        if has_take and 'd' in args.legs:
            short = t[:, :3].contiguous()
            leg['take_short_rows_dz3'] = take_leg(torch, ctx, bc.DeviceData.from_torch(short, ctx=ctx), short, rng,
                                                  (1_000_000, 10_000_000), args.repeats, name + ' dz=3')
            del short
        res['dtypes'][name] = leg
        del dd, prj
    if args.baseline:
        base = json.load(open(args.baseline))
        res['baseline'] = base
        res['ratio_baseline_over_this'] = {}
        for name, leg in res['dtypes'].items():
            b = base['dtypes'][name]
            r = {'gradient': {m: b['gradient'][m]['median_ms'] / v['median_ms'] for m, v in leg['gradient'].items()}}
            if 'hilbert_construct_1e6' in leg:
                r['hilbert_construct_1e6'] = b['hilbert_construct_1e6']['median_ms'] / leg['hilbert_construct_1e6']['median_ms']
            if '10000' in leg['take']:
                r['rows_to_host_1e4_over_take_1e4_wall'] = b['rows_to_host_1e4']['median_ms'] / leg['take']['10000']['call_wall']['median_ms']
            res['ratio_baseline_over_this'][name] = r
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps({'ok': True, 'out': args.out}))
    return 0


if __name__ == '__main__':
    sys.exit(main())
