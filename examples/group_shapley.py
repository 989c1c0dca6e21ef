#!/usr/bin/env python3
"""Group selection by data valuation: the `DShapley` baseline of the reference's group experiment
(examples/zellner_logreg/group_selection.py:145-174) beside `RAND`, on synthetic groups.

    python examples/group_shapley.py [--groups 30] [--d 6] [--perms 100] [--max-groups 10] [--select 8] [--flip 0.3] [--seed 1]

Data: `gen_synthetic`-style logistic data restated here (standard normal covariates, the intercept as the last column, labels
drawn from the logistic model of a random theta), cut into groups of 10 .. 50 rows; a fraction `--flip` of the groups has its
labels flipped -- the contaminated groups a valuation should rank last.  bc.valuation.tmc_shapley values every group by
truncated Monte-Carlo Shapley: per permutation the posteriors of the first 1, 2, ... groups are sampled in one batched device
run and scored against the held-out rows where their samples lie; nothing but one accuracy per problem comes back.

Printed: the held-out accuracy of the posterior of `--select` groups chosen by Shapley rank against the same number chosen
uniformly at random (RAND, averaged over `--rand-trials` draws), each sampled by logistic_hmc_many and scored with
bc.samplers.logistic_score; and how many of the flipped groups each selection took."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import beta_cores_amd as bc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--groups', type=int, default=30)
    ap.add_argument('--d', type=int, default=6)
    ap.add_argument('--n-test', type=int, default=2000)
    ap.add_argument('--perms', type=int, default=100)
    ap.add_argument('--max-groups', type=int, default=10)
    ap.add_argument('--select', type=int, default=8)
    ap.add_argument('--flip', type=float, default=0.3)
    ap.add_argument('--rand-trials', type=int, default=20)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--adapt', default='chunks', choices=['chunks', 'stan'], help="the samplers' warm-up: 'stan' adapts step and mass per chain on the device")
    ap.add_argument('--summary', action='store_true', help="the worst split-R-hat and the smallest ESS over all the run's posteriors, reduced on the device")
    a = ap.parse_args()
    rng = np.random.RandomState(a.seed)
    sizes = rng.randint(10, 51, size=a.groups)
    n = int(sizes.sum())
    X = np.hstack((rng.randn(n + a.n_test, a.d - 1), np.ones((n + a.n_test, 1))))      # the intercept is the last column
    th_true = rng.randn(a.d) * 2. / np.sqrt(a.d)
    Y = np.where(rng.rand(n + a.n_test) < 1. / (1. + np.exp(-X.dot(th_true))), 1., -1.)
    Xt, Yt = X[n:], Y[n:]
    X, Y = X[:n], Y[:n].copy()
    bounds = np.concatenate(([0], np.cumsum(sizes)))
    groups = [np.arange(bounds[g], bounds[g + 1]) for g in range(a.groups)]
    flipped = np.sort(rng.choice(a.groups, int(round(a.flip * a.groups)), replace=False))
    for g in flipped:
        Y[groups[g]] *= -1.
    Z = Y[:, None] * X
    held = bc.samplers.HeldOut(Xt, Yt)
    hmc = dict(n_samples=64, n_chains=16, warmup=100, step_size=0.1, n_leapfrog=8, adapt=a.adapt)

    t0 = time.perf_counter()
    val = bc.valuation.tmc_shapley(Z, groups, held, a.perms, min(a.max_groups, a.groups), group_cap=50, rng=rng, summary=a.summary, **hmc)
    t_val = time.perf_counter() - t0
    print('%d groups (%d rows, D = %d), %d flipped; %d permutations x %d prefixes = %d posteriors valued in %.2f s (%d through the '
          'single-problem engine)' % (a.groups, n, a.d, len(flipped), a.perms, val.values.shape[1] - 1, a.perms * (val.values.shape[1] - 1),
                                      t_val, val.n_fallback))
    if a.summary:
        print('chains: worst R-hat %.4f, smallest ESS %.0f of %d draws, over all %d posteriors' %
              (np.nanmax(val.max_rhat), np.nanmin(val.min_ess), hmc['n_samples'] * hmc['n_chains'], val.max_rhat.size))
    order = np.argsort(-val.phi)
    print('Shapley values: flipped groups mean %+.4f, the others mean %+.4f' % (val.phi[flipped].mean(), np.delete(val.phi, flipped).mean()))

    def accuracy_of(selections):
        """The held-out accuracy of the posterior of each selection of groups: one batched run, scored with logistic_score."""
        problems = [(Z[np.concatenate([groups[g] for g in sel])], None) for sel in selections]
        res = bc.samplers.logistic_hmc_many(problems, rng=np.random.RandomState(a.seed + 1), start=np.zeros((16, a.d)), **hmc)
        return np.array([held.accuracy(bc.samplers.logistic_score(held, r.pooled())[0]) for r in res])
    k = min(a.select, a.groups)
    rand = [rng.choice(a.groups, k, replace=False) for _ in range(a.rand_trials)]
    acc = accuracy_of([order[:k]] + rand + [np.arange(a.groups)])
    print('select %d groups:  Shapley-ranked accuracy %.4f (%d flipped among them)   RAND accuracy %.4f +- %.4f (%.1f flipped on average)   '
          'all groups %.4f' % (k, acc[0], len(np.intersect1d(order[:k], flipped)), acc[1:-1].mean(), acc[1:-1].std(),
                               np.mean([len(np.intersect1d(s, flipped)) for s in rand]), acc[-1]))


if __name__ == '__main__':
    main()
