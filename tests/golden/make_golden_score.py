#!/usr/bin/env python3
"""Generate tests/golden/score_f20.npz by RUNNING THE REFERENCE's held-out scoring: `compute_accuracy` and `log_likelihood` of
examples/common/model_lr.py (model_lr.py:32-42, 72-79), as the logistic drivers call them on the sampled thetas.

Run in the build container only (the reference never travels):   python tests/golden/make_golden_score.py

Like make_golden_encoder.py, nothing of the reference is modified, copied or byte-compiled: model_lr.py is imported from where it
lies (the `examples/common` entry of the import recipe of SURVEY 8(c); the module needs NumPy and SciPy only, so no stub parent
packages are involved).  The fixture is data only: Xt (120 x 6, the last column the intercept), Yt, 40 thetas, and what the
reference computes from them -- compute_accuracy over all thetas, per theta (one call each), and the per-theta sums of
log_likelihood(Yt[:, None] * Xt, thetas).  The inputs hold two all-zero rows (y = +1 and y = -1: the tie) and thetas scaled so
that margins lie on both sides of +-100 and beyond +-745; every other (row, theta) margin is at least 1e-9 in size (asserted),
where the reference's prediction is the sign's.
"""
import os
import sys

os.environ['PYTHONDONTWRITEBYTECODE'] = '1'
sys.dont_write_bytecode = True
import numpy as np
import scipy

REF = os.environ.get('BC_REFERENCE', '/root/reference')
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF + '/examples/common')
import model_lr  # noqa: E402


def main():
    rng = np.random.RandomState(20)
    nt, d, t = 120, 6, 40
    Xt = np.hstack((rng.randn(nt, d - 1), np.ones((nt, 1))))
    Yt = np.where(rng.rand(nt) < 0.5, 1., -1.)
    Xt[0], Xt[1] = 0., 0.
    Yt[0], Yt[1] = 1., -1.
    thetas = rng.randn(t, d) * 0.8
    thetas[1] *= 150.
    thetas[2] *= 3000.
    s = Xt.astype(np.longdouble).dot(thetas.astype(np.longdouble).T)
    nz = np.any(Xt != 0, axis=1)
    assert np.abs(s[nz]).min() >= 1e-9
    assert ((np.abs(s) > 100) & (np.abs(s) < 745)).any() and (s > 745).any() and (s < -745).any()
    acc = model_lr.compute_accuracy(Xt, Yt, thetas)
    acc_each = np.array([model_lr.compute_accuracy(Xt, Yt, thetas[i:i + 1]) for i in range(t)])
    ll = model_lr.log_likelihood(Yt[:, np.newaxis] * Xt, thetas).sum(axis=0)
    np.savez_compressed(os.path.join(OUT, 'score_f20.npz'), Xt=Xt, Yt=Yt, thetas=thetas, accuracy=np.float64(acc), accuracy_each=acc_each,
                        ll_sum=ll, numpy=np.__version__, scipy=scipy.__version__)
    print('score_f20.npz: accuracy %.6f, ll sums %.6g .. %.6g' % (acc, ll.min(), ll.max()))


if __name__ == '__main__':
    main()
