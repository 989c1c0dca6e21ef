#!/usr/bin/env python3
"""Batch coreset construction for a neural-linear model on RAW resident rows, the feature map on the device.

    python examples/neural_linear.py [--n 200000] [--alg BCORES|SVI] [--batches 5] [--seed 1] [--held 20000]

The loop of the reference's neural-linear driver (zellner_neural_linear/main.py) on synthetic data: a small torch network
x -> 20 features (Linear -> BatchNorm1d -> ReLU, twice) with a Bayesian linear head; every batch acquires one group of 20
rows with BetaCoreset / SparseVICoreset (groups, an initial set, sub-sampled selection and optimisation), then retrains the
network on the weighted coreset and hands the new parameters to the device encoder (`enc.update_from_torch`).  The raw
rows [x, y] stay resident as float32; the projector encodes between the gather and K1 (`DeviceProjector(encoder=enc)`),
the sampler sees the device's features of the coreset points (`enc(pts)`), and `get()` returns raw rows.

After every batch the Bayesian head is judged as the driver's `nl.test(...)` judges it: `--held` further rows, drawn from the same
process with a stream of their own and never handed to the coreset, stay resident as raw float32 rows
(`RegressionHeldOut(encoder=enc)` re-encodes them once per retrained network), the head's posteriors come from `weighted_post` and
`weighted_post_corrected` on `enc(pts)`, and one `linreg_predictive` call returns for both the mean negative log density of its Gaussian predictive and the RMSE -- on the device.
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import beta_cores_amd as bc


def make_network(d, out_features, seed):
    torch.manual_seed(seed)
    return nn.Sequential(nn.Linear(d, out_features), nn.BatchNorm1d(out_features), nn.ReLU(),
                         nn.Linear(out_features, out_features), nn.BatchNorm1d(out_features), nn.ReLU())


def train(net, head, wts, pts, epochs=30):
    """Weighted least squares through the network and a linear read-out: the stand-in for the driver's nl.optimize()."""
    x, y, w = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)) for a in (pts[:, :-1], pts[:, -1], wts))
    opt = torch.optim.Adam(list(net.parameters()) + list(head.parameters()), lr=1e-2, weight_decay=1e-3)
    net.train()
    for _ in range(epochs):
        opt.zero_grad()
        ((head(net(x)).squeeze(1) - y) ** 2 * w).sum().div(w.sum()).backward()
        opt.step()
    net.eval()                                     # the encoder reads the running statistics: eval mode before every build


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=200000)
    ap.add_argument('--d', type=int, default=13)
    ap.add_argument('--alg', default='BCORES', choices=['BCORES', 'SVI'])
    ap.add_argument('--batches', type=int, default=5)
    ap.add_argument('--proj-dim', type=int, default=100)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--held', type=int, default=20000)
    a = ap.parse_args()
    np.random.seed(a.seed)
    out_features, group, init_size, sigsq = 20, 20, 20, 1.0
    X = np.random.randn(a.n, a.d)
    y = np.tanh(X[:, 0]) + 0.5 * X[:, 1] * X[:, 2] + 0.1 * np.random.randn(a.n)
    Z = np.hstack((X, y[:, None])).astype(np.float32)
    groups = [list(range(g, min(g + group, a.n))) for g in range(0, a.n, group)]
    init_idcs = np.random.choice(a.n, init_size, replace=False)
    Z_init = Z[init_idcs].astype(np.float64)

    net, head = make_network(a.d, out_features, a.seed), nn.Linear(out_features, 1)
    train(net, head, np.ones(init_size), Z_init)
    enc = bc.encoders.MLPEncoder.from_torch(net)
    data = bc.DeviceData(Z, dtype=np.float32)      # the raw rows, uploaded once, 4 bytes an entry
    hrng = np.random.RandomState(a.seed + 1)       # the held-out split: its own stream, so the draws above and below are unchanged
    Xh = hrng.randn(a.held, a.d)
    yh = np.tanh(Xh[:, 0]) + 0.5 * Xh[:, 1] * Xh[:, 2] + 0.1 * hrng.randn(a.held)
    held = bc.RegressionHeldOut(np.hstack((Xh, yh[:, None])).astype(np.float32), encoder=enc, dtype=np.float32)

    Sig0inv = np.eye(out_features)

    def sampler_w(n, wts, pts):                    # main.py:126-136 over the device's features of the coreset points
        if pts.shape[0] == 0:
            wts, pts = np.zeros(1), np.zeros((1, Z.shape[1]))
        z = enc(pts)
        Xf, Yf = z[:, :-1], z[:, -1]
        Sigp = np.linalg.inv(Sig0inv + (wts[:, None] * Xf).T.dot(Xf) / sigsq)
        mup = Sigp.dot(Sig0inv.dot(np.ones(out_features)) + (wts[:, None] * Yf[:, None] * Xf).sum(axis=0) / sigsq)
        return np.random.multivariate_normal(mup, Sigp, n)

    model = bc.likelihoods.LinearRegression(sigsq)
    common = dict(opt_itrs=50, n_subsample_opt=1000, n_subsample_select=50, step_sched=lambda i: 0.1 / (1. + i),
                  wts=np.ones(init_size), idcs=init_idcs.copy(), pts=Z_init, groups=groups, initialized=True)
    if a.alg == 'BCORES':
        prj = bc.DeviceBetaProjector(sampler_w, a.proj_dim, model, encoder=enc)
        alg = bc.BetaCoreset(data, prj, beta=0.2, learn_beta=False, **common)
    else:
        prj = bc.DeviceProjector(sampler_w, a.proj_dim, model, encoder=enc)
        alg = bc.SparseVICoreset(data, prj, **common)
    for m in range(1, a.batches + 1):
        alg.build(1, a.n)
        wts, pts, idcs = alg.get()[:3]
        assert pts.shape[1] == Z.shape[1]          # raw rows, ready for the network
        train(net, head, wts, pts)
        enc.update_from_torch(net)                 # the next build projects with the new features
        with torch.no_grad():
            rmse = float(torch.sqrt(torch.mean((head(net(torch.from_numpy(Z[:5000, :-1]))).squeeze(1) - torch.from_numpy(Z[:5000, -1])) ** 2)))
        print('batch %d: %d points, %d groups, rmse on 5000 rows %.4f, encoder version %d, bulk encodes so far %d'
              % (m, len(idcs), len(alg.selected_groups), rmse, enc.version, prj.encode_launches))
        # two posteriors of the head in ONE call: weighted_post's (the covariance LSigp LSigp^T the reference's samplers draw
        # from, its quirk included) and weighted_post_corrected's (the true posterior: covariance LSigp^T LSigp, so F = LSigp^T)
        z = enc(pts)
        mu_q, L_q, _ = bc.weighted_post(np.ones(out_features), Sig0inv, sigsq, z, wts)
        mu_c, L_c, _ = bc.weighted_post_corrected(np.ones(out_features), Sig0inv, sigsq, z, wts)
        scores = bc.linreg_predictive(held, np.array([mu_q, mu_c]), np.array([L_q, L_c.T]), sigsq)      # re-encodes the held-out rows once
        print('         Bayesian head on %d held-out rows: nll %.4f, rmse %.4f (weighted_post); nll %.4f, rmse %.4f (true posterior)'
              % (a.held, scores.nll()[0], scores.rmse()[0], scores.nll()[1], scores.rmse()[1]))


if __name__ == '__main__':
    main()
