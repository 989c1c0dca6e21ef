#!/usr/bin/env python3
"""Hilbert coresets for logistic regression, tangent space from a full-data Laplace fit on the GPU.

    python examples/logistic_hilbert.py [--n 1000000] [--d 10] [--sizes 10,20,50,100] [--seed 1]

Synthetic rows z = y*x (the logistic layout, model_lr.py:29).  Two projections, in the style of the reference's Gaussian
driver (zellner_gaussian/main.py:71-84, 106-114):
  GIGAO  Theta from the Laplace approximation of the FULL data (logistic_laplace on the resident rows: K5 + K4 per Newton step)
  GIGAR  Theta from the Laplace approximation of a 1 000-row uniform sub-sample, weighted N/1000
For every coreset size the coreset's own Laplace posterior is compared with the full-data one by KL(coreset || full).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import beta_cores_amd as bc


def gaussian_KL(mu0, Sig0, mu1, Sig1inv):
    t1 = np.dot(Sig1inv, Sig0).trace()
    t2 = np.dot((mu1 - mu0), np.dot(Sig1inv, mu1 - mu0))
    t3 = -np.linalg.slogdet(Sig1inv)[1] - np.linalg.slogdet(Sig0)[1]
    return 0.5 * (t1 + t2 + t3 - mu0.shape[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1_000_000)
    ap.add_argument('--d', type=int, default=10)
    ap.add_argument('--sizes', default='10,20,50,100')
    ap.add_argument('--proj-dim', type=int, default=200)
    ap.add_argument('--seed', type=int, default=1)
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(',')]
    rng = np.random.RandomState(a.seed)
    X = rng.randn(a.n, a.d)
    th_true = rng.randn(a.d) * 2. / np.sqrt(a.d)
    y = np.where(rng.rand(a.n) < 1. / (1. + np.exp(-X.dot(th_true))), 1., -1.)
    Z = y[:, None] * X
    mu0 = np.zeros(a.d)
    dz = bc.DeviceData(Z)

    # full-data posterior: the reference the coresets are judged against, and GIGAO's tangent space
    full = bc.samplers.LaplaceFullDataSampler(dz, mu0, rng=rng)
    H_full = full.LSigInv.dot(full.LSigInv.T)                 # the Laplace precision, I + Z^T diag(c) Z at the mode
    sub = rng.choice(a.n, min(1000, a.n), replace=False)
    w_sub = np.zeros(a.n)
    w_sub[sub] = a.n / float(len(sub))
    realistic = bc.samplers.LaplaceFullDataSampler(dz, mu0, wts=w_sub, rng=rng)
    model = bc.likelihoods.LogisticRegression()
    print('N = %d, D = %d: full-data Laplace mode |mu| = %.4f; sub-sample mode |mu| = %.4f'
          % (a.n, a.d, np.linalg.norm(full.mu), np.linalg.norm(realistic.mu)))
    for name, smp in (('GIGAO', full), ('GIGAR', realistic)):
        alg = bc.HilbertCoreset(Z, bc.DeviceProjector(smp, a.proj_dim, model))
        for m in sizes:
            if m > alg.size():
                alg.build(m - alg.size(), m)              # (GIGA adds at most one point per iteration)
            wts, pts, _ = alg.get()
            mu_c, _, LSigInv_c = bc.samplers.logistic_laplace(wts, pts, mu0, solver='newton')
            Sig_c = np.linalg.inv(LSigInv_c.dot(LSigInv_c.T))
            print('%s  M = %4d  points %4d  Hilbert error %.4e  KL(coreset || full) %.6e'
                  % (name, m, len(wts), alg.error(), gaussian_KL(mu_c, Sig_c, full.mu, H_full)))


if __name__ == '__main__':
    main()
