#!/usr/bin/env python3
"""Generate tests/golden/f23_neural_encoder.npz by RUNNING THE REFERENCE's neural-linear feature extractor.

Run in the build container only (the reference never travels):   python tests/golden/make_golden_encoder.py

Like make_golden.py, nothing of the reference is modified, copied or byte-compiled: `examples/common/neural.py` is imported
from where it lies (it needs only NumPy and torch, so no stub parent packages are involved), a seeded `NeuralLinear`
(13 inputs, out_features = 20) is trained for a few `optimize` epochs so that every parameter and both batch norms' running
statistics have moved, switched to eval mode, and its `encode` is recorded on a seeded input.  The fixture is data only:
the state_dict arrays (float32), eps, the 257 x 13 float32 input, torch's float32 features of it, and the library versions.
"""
import os
import sys

os.environ['PYTHONDONTWRITEBYTECODE'] = '1'
sys.dont_write_bytecode = True
import numpy as np
import torch

REF = os.environ.get('BC_REFERENCE', '/root/reference')
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF + '/examples/common')
import neural  # noqa: E402


def main():
    rng = np.random.RandomState(23)
    n, d, out_features = 400, 13, 20
    X = rng.randn(n, d).astype(np.float32)
    y = (np.tanh(X[:, 0]) + 0.5 * X[:, 1] * X[:, 2] + 0.1 * rng.randn(n)).astype(np.float32)
    Z = np.hstack((X, y[:, None])).astype(np.float32)
    nl = neural.NeuralLinear(Z, out_features=out_features, seed=23)
    before = {k: v.detach().clone() for k, v in nl.feature_extractor.state_dict().items()}
    nl.optimize(torch.ones(n), torch.from_numpy(Z), num_epochs=5, initial_lr=1e-2)
    nl.eval()
    fe = nl.feature_extractor
    sd = fe.state_dict()
    moved = [k for k in sd if not torch.equal(sd[k], before[k])]
    assert sorted(moved) == sorted(sd.keys()), 'not every parameter / statistic has moved: %s' % sorted(set(sd) - set(moved))
    # the recorded input: ordinary rows, a zero row, entries of 1e4, and rows whose pre-activations of the FIRST layer are all
    # negative (found by gradient descent on the input; the last layer's cannot all be made negative for this network), so that
    # the hidden activations are exact zeros and the features those of a zero hidden vector
    x = rng.randn(257, d).astype(np.float32)
    x[3] = 0.
    x[10, 4] = 1e4
    x[11, [0, 7, 12]] = [1e4, -1e4, 1e4]
    pre = fe[:2]                                   # up to the first batch norm: the first layer's pre-activations
    cand = torch.from_numpy((rng.randn(64, d) * 2).astype(np.float32)).requires_grad_(True)
    opt = torch.optim.Adam([cand], lr=0.05)
    for _ in range(500):                           # push every pre-activation of the candidates below -0.1
        opt.zero_grad()
        torch.relu(pre(cand) + 0.1).sum().backward()
        opt.step()
    cand = cand.detach()
    with torch.no_grad():
        dead = np.flatnonzero(((pre(cand) < 0).all(dim=1) & (fe[:3](cand) == 0).all(dim=1)).numpy())
    assert dead.size >= 3, 'no candidate row with all-negative pre-activations'
    neg_rows = np.array([20, 21, 22])
    x[neg_rows] = cand[dead[:3]].numpy()
    with torch.no_grad():
        feats = nl.encode(torch.from_numpy(x)).numpy()
    assert feats.dtype == np.float32 and feats.shape == (257, out_features) and (feats[neg_rows] == feats[neg_rows[0]]).all()
    arrs = {'sd_' + k: v.detach().numpy() for k, v in sd.items()}
    arrs.update(eps=np.array(fe[1].eps), x=x, features=feats, all_negative_rows=neg_rows,
                meta_numpy=np.array(np.__version__), meta_torch=np.array(torch.__version__))
    path = os.path.join(OUT, 'f23_neural_encoder.npz')
    np.savez_compressed(path, **arrs)
    print('%-28s %8.1f KB' % ('f23_neural_encoder.npz', os.path.getsize(path) / 1024.))


if __name__ == '__main__':
    main()
