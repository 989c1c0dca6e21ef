#!/usr/bin/env python3
"""The logistic drivers' evaluation with exact-posterior samples drawn on the GPU.

    python examples/logistic_mcmc_eval.py [--n 200000] [--d 10] [--m 200] [--samples 250] [--chains 16] [--seed 1] [--curve K [--laplace] [--summary]] [--bpsvi M]

The reference's logistic drivers end by drawing ~1 000 posterior samples with MCMC -- of the full data as ground truth
(examples/common/mcmc.py:21), of the weighted coreset as the thing to judge (zellner_logreg/main.py:225-230) -- and scoring them
on a held-out split.  Here both come from samplers.logistic_hmc (multi-chain HMC, every pass over the rows on the device), next
to samples of the coreset's Laplace approximation:

  full      HMC over all N resident training rows                          (the ground truth)
  coreset   HMC over the M weighted coreset rows (GIGA on a Laplace tangent space), an ndarray through the same call
  laplace   mu + randn . LSig^T from the coreset's Laplace fit

Scores, in plain NumPy on the small test split as the drivers compute them (model_lr.py:32-42, main.py:229-230): the accuracy
of the max-likelihood prediction under each sampled theta, averaged (compute_accuracy), and the test log-likelihood summed over
the points and averaged over the samples.  Also the distance of each sample set's mean from the ground truth's, in units of the
ground truth's posterior standard deviations.

--curve K (opt-in) adds the drivers' evaluation curve (zellner_logreg/main.py:219-230: `for m in range(M + 1)`): K nested coreset
sizes between 0 and M -- the coresets after m greedy steps of the same construction -- sampled by ONE batched call,
samplers.logistic_hmc_many, on common random numbers, and scored as above.

--laplace (with --curve) prints the Laplace curve beside the HMC one: the same K coresets fitted, drawn and scored on the device
by samplers.logistic_laplace_many(..., score=held, keep_draws=False) -- as many draws per coreset as the HMC leg keeps, in calls
of at most 256 draws each (the call's limit); no draw is copied to the host.

--bpsvi M (opt-in) adds the drivers' BatchPSVI curve (zellner_logreg/main.py:173-186: `build_per_m` for m = 1 .. M over a Pool): the
pseudo-coresets of all M sizes from ONE BatchPSVICoreset.build_many -- stepped in lock-step on the device, common random numbers --
handed to the same two batched calls, samplers.logistic_laplace_many and samplers.logistic_hmc_many, each scoring where its
samples lie (score=held).
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import beta_cores_amd as bc


def log_likelihood(z, th):
    """model_lr.py:72-79"""
    m = -np.atleast_2d(z).dot(np.atleast_2d(th).T)
    small = m < 100
    m[small] = -np.log1p(np.exp(m[small]))
    m[np.logical_not(small)] = -m[np.logical_not(small)]
    return m


def compute_accuracy(Xt, Yt, thetas):
    """model_lr.py:32-42"""
    loglikep, logliken = log_likelihood(Xt, thetas), log_likelihood(-Xt, thetas)
    predictions = np.ones(loglikep.shape)
    predictions[logliken > loglikep] = -1
    return np.mean(Yt[:, np.newaxis] == predictions)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=200_000)
    ap.add_argument('--n-test', type=int, default=2000)
    ap.add_argument('--d', type=int, default=10)
    ap.add_argument('--m', type=int, default=200, help='coreset size')
    ap.add_argument('--samples', type=int, default=250, help='kept iterations per chain')
    ap.add_argument('--warmup', type=int, default=150)
    ap.add_argument('--chains', type=int, default=16)
    ap.add_argument('--leapfrog', type=int, default=8)
    ap.add_argument('--proj-dim', type=int, default=200)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--curve', type=int, default=0, help='score this many nested coreset sizes 0 .. m from one batched call (0: off)')
    ap.add_argument('--summary', action='store_true', help='with --curve: the worst split-R-hat and the smallest ESS of every coreset size, reduced on the device')
    ap.add_argument('--laplace', action='store_true', help='with --curve: the Laplace posteriors of the same coresets, fitted, drawn and scored on the device')
    ap.add_argument('--adapt', default='chunks', choices=['chunks', 'stan'],
                    help="the warm-up of the batched calls: 'stan' adapts step and mass per chain on the device (logistic_hmc_many)")
    ap.add_argument('--bpsvi', type=int, default=0, help='the BatchPSVI pseudo-coresets of sizes 1 .. M from one build_many, Laplace-fitted and sampled in one call each (0: off)')
    ap.add_argument('--bpsvi-itrs', type=int, default=100, help='with --bpsvi: joint ADAM steps on weights and points')
    a = ap.parse_args()
    rng = np.random.RandomState(a.seed)
    X = rng.randn(a.n + a.n_test, a.d)
    X[:, -1] = 1.                                              # the intercept is the last column
    th_true = rng.randn(a.d) * 2. / np.sqrt(a.d)
    Y = np.where(rng.rand(X.shape[0]) < 1. / (1. + np.exp(-X.dot(th_true))), 1., -1.)
    Xt, Yt = X[a.n:], Y[a.n:]
    Z, Zt = Y[:a.n, None] * X[:a.n], Yt[:, None] * Xt
    dz = bc.DeviceData(Z)
    mu0 = np.zeros(a.d)
    hmc = dict(n_samples=a.samples, n_chains=a.chains, n_leapfrog=a.leapfrog, step_size=0.3, inv_mass='laplace', warmup=a.warmup)

    t0 = time.perf_counter()
    full = bc.samplers.logistic_hmc(dz, None, rng=rng, **hmc)
    t_full = time.perf_counter() - t0
    truth = full.pooled()
    mu_t, sd_t = truth.mean(axis=0), truth.std(axis=0)

    smp = bc.samplers.LaplaceFullDataSampler(dz, mu0, rng=rng)
    alg = bc.HilbertCoreset(Z, bc.DeviceProjector(smp, a.proj_dim, bc.likelihoods.LogisticRegression()))
    curve_at = sorted(set(int(round(v)) for v in np.linspace(0, a.m, a.curve))) if a.curve > 0 else []
    nested = []
    done = 0
    for m in curve_at:                                         # (the greedy construction is incremental: m - done more steps)
        if m > done:
            alg.build(m - done, m)
            done = m
        w_m, p_m, _ = alg.get() if done > 0 else (np.zeros(0), np.zeros((0, a.d)), None)      # (m = 0: the empty coreset, the prior)
        nested.append((np.array(p_m, dtype=np.float64).reshape(-1, a.d), np.array(w_m, dtype=np.float64)))
    if a.m > done:
        alg.build(a.m - done, a.m)
    wts, pts, _ = alg.get()
    t0 = time.perf_counter()
    core = bc.samplers.logistic_hmc(pts, wts, rng=rng, **hmc)
    t_core = time.perf_counter() - t0
    mu_c, LSig_c, _ = bc.samplers.logistic_laplace(wts, pts, mu0, solver='newton')
    lap = mu_c + rng.randn(truth.shape[0], a.d).dot(LSig_c.T)

    print('N = %d, D = %d, test split %d; coreset of %d points (Hilbert error %.3e)' % (a.n, a.d, a.n_test, len(wts), alg.error()))
    print('HMC: %d chains x (%d warm-up + %d kept) iterations of %d leapfrog steps: full data %.2f s (step %.4g, acceptance %.2f), '
          'coreset %.2f s (step %.4g, acceptance %.2f)' % (a.chains, a.warmup, a.samples, a.leapfrog, t_full, full.step_size,
                                                           full.accept_rate.mean(), t_core, core.step_size, core.accept_rate.mean()))
    for name, th in (('full', truth), ('coreset', core.pooled()), ('laplace', lap)):
        print('%-8s accuracy %.4f   test log-likelihood %.3f   |mean - truth| / sd: max %.3f' %
              (name, compute_accuracy(Xt, Yt, th), log_likelihood(Zt, th).sum(axis=0).mean(), np.abs((th.mean(axis=0) - mu_t) / sd_t).max()))
    if nested:
        t0 = time.perf_counter()
        curve = bc.samplers.logistic_hmc_many(nested, rng=rng, summary=a.summary, adapt=a.adapt, **hmc)
        t_curve = time.perf_counter() - t0
        print('curve: %d coreset sizes in one batched call, %.2f s (%.1f ms on the GPU); through the single-problem engine: %s' %
              (len(nested), t_curve, curve.device_ms or 0., curve.fallback or 'none'))
        lap_curve = None
        if a.laplace:
            held = bc.samplers.HeldOut(Xt, Yt)
            total = a.samples * a.chains
            calls = -(-total // bc.samplers.LAPLACE_SMALL_MAX_DRAWS)
            per = -(-total // calls)
            t0 = time.perf_counter()
            parts = [bc.samplers.logistic_laplace_many(nested, n_draws=per, rng=rng, score=held, keep_draws=False) for _ in range(calls)]
            t_lap = time.perf_counter() - t0
            lap_curve = [(held.accuracy(np.concatenate([q[k].correct for q in parts])), np.concatenate([q[k].test_ll for q in parts]).mean(),
                          parts[0][k].mu, parts[0][k].newton) for k in range(len(nested))]
            print('laplace curve: %d coreset sizes x %d draws fitted, drawn and scored in %d call(s), %.3f s (%.2f ms on the GPU)' %
                  (len(nested), per * calls, calls, t_lap, sum(q.device_ms for q in parts)))
        for k, (m, (p_m, w_m), res) in enumerate(zip(curve_at, nested, curve)):
            th = res.pooled()
            print('m = %-4d points %-4d accuracy %.4f   test log-likelihood %.3f   |mean - truth| / sd: max %.3f   step %.4g' %
                  (m, len(w_m), compute_accuracy(Xt, Yt, th), log_likelihood(Zt, th).sum(axis=0).mean(),
                   np.abs((th.mean(axis=0) - mu_t) / sd_t).max(), res.step_size))
            if a.summary:      # (can these chains be trusted?  R-hat near 1 and an ESS of hundreds say yes)
                print('         chains      worst R-hat %.4f   smallest ESS %.0f of %d draws%s' %
                      (res.summary.worst_rhat(), res.summary.least_ess(), th.shape[0], '   (ESS sum cut at max_lag)' if res.summary.ess_truncated.any() else ''))
            if lap_curve:
                acc, tll, mu_l, newton = lap_curve[k]
                print('         laplace     accuracy %.4f   test log-likelihood %.3f   |mode - truth| / sd: max %.3f   Newton steps %d' %
                      (acc, tll, np.abs((mu_l - mu_t) / sd_t).max(), newton))
    if a.bpsvi > 0:
        sizes = list(range(1, a.bpsvi + 1))
        smp_w = bc.samplers.LogisticLaplaceSampler(mu0, rng=rng, solver='newton')
        psvi = bc.BatchPSVICoreset(dz, bc.DeviceProjector(smp_w, min(a.proj_dim, 256), bc.likelihoods.LogisticRegression()), opt_itrs=a.bpsvi_itrs,
                                   n_subsample_opt=200, fused_gradient=True)
        np.random.seed(a.seed)
        t0 = time.perf_counter()
        pcurve = psvi.build_many(sizes)
        t_build = time.perf_counter() - t0
        print('bpsvi: %d sizes x %d steps by route %r in %.2f s (%.1f ms on the GPU); marked: %s' %
              (len(sizes), a.bpsvi_itrs, pcurve.route, t_build, pcurve.device_ms, pcurve.marked or 'none'))
        kept = [(m, e) for m, e in zip(sizes, pcurve) if e is not None]
        probs = [(np.asarray(p, dtype=np.float64), np.asarray(w, dtype=np.float64)) for _, (w, p, _) in kept]
        held = bc.samplers.HeldOut(Xt, Yt)
        laps = bc.samplers.logistic_laplace_many(probs, n_draws=min(a.samples, bc.samplers.LAPLACE_SMALL_MAX_DRAWS), rng=rng, score=held, keep_draws=False)
        many = bc.samplers.logistic_hmc_many(probs, rng=rng, score=held, keep_samples=False, adapt=a.adapt, **hmc)
        for (m, (w, _, _)), fit, res in zip(kept, laps, many):
            print('m = %-4d points %-4d laplace: accuracy %.4f  test log-likelihood %.3f   hmc: accuracy %.4f  test log-likelihood %.3f' %
                  (m, len(w), held.accuracy(fit.correct), fit.test_ll.mean(), held.accuracy(res.correct.ravel()), res.test_ll.mean()))


if __name__ == '__main__':
    main()
