#!/usr/bin/env python3
"""Generate tests/golden/predict_f24.npz by RUNNING THE REFERENCE's held-out evaluation of the neural-linear model's Bayesian head:
`BayesianRegressionDense([D, 1], sigmasq, s).forward` (examples/common/neural.py:33-62: the posterior of the head and its Gaussian
predictive) and `NeuralLinear.gaussian_log_density`, `get_unnormalized` and `rmse` (neural.py:253-292), as `_evaluate` combines
them: the mean negative log density and the RMSE of the un-normalised predictions.

Run in the build container only (the reference never travels):   python tests/golden/make_golden_predict.py

Like make_golden_score.py, nothing of the reference is modified, copied or byte-compiled: neural.py is imported from where it lies
(it needs NumPy and torch only) and is run on float64 tensors.  The methods of NeuralLinear used here do not touch the network, so
they are called on a stand-in that carries the three attributes get_unnormalized reads; no network is built.  The density is
evaluated with column shapes (y, mean and variance all Nt x 1), which gives the per-row Gaussian log density the docstring of
gaussian_log_density states.  (Called as `_evaluate` calls it -- y and mean of shape Nt, the variance Nt x 1 -- the same method
broadcasts to Nt x Nt and returns -1/2 (sum_j r_j^2 / var_i + log var_i + Nt log 2 pi) per row i: a quirk of the driver that the
library does not reproduce; it is recorded here as `nll_as_driver_broadcasts` for the record only, no test reads it.)

The fixture is data only: Xt (120 x 6), yt, the 60 training rows, and per setting (sigmasq, s) in ((1, 1), (0.25, 0.25)) what the
reference computes: theta_mean, theta_cov, the per-row pred_mean, pred_var and log_density, the driver's nll and rmse with
output_std = 2.5 and output_mean = -1.25, the versions, and host_gap: the largest per-row |restatement - reference| /
(|reference| + 1) over pred_mean, pred_var and log_density, where the restatement is tests/predict_cases.py's long-double one
through numpy.linalg.cholesky(theta_cov).  host_gap <= 1e-12 is asserted here (measured at generation: 5.65e-16); the tests allow
the derived bound plus 8 host_gap (|golden| + 1), the factor 8 for another LAPACK's Cholesky on the testing host.
"""
import os
import sys
import types

os.environ['PYTHONDONTWRITEBYTECODE'] = '1'
sys.dont_write_bytecode = True
import numpy as np
import torch

REF = os.environ.get('BC_REFERENCE', '/root/reference')
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF + '/examples/common')
sys.path.insert(0, os.path.dirname(OUT))
import neural  # noqa: E402
import predict_cases as pc  # noqa: E402


def main():
    rng = np.random.RandomState(24)
    nt, ntrain, d = 120, 60, 6
    w = rng.randn(d)
    Xtr, Xt = rng.randn(ntrain, d), rng.randn(nt, d)
    ytr, yt = Xtr.dot(w) + 0.4 * rng.randn(ntrain), Xt.dot(w) + 0.4 * rng.randn(nt)
    out_std, out_mean = 2.5, -1.25
    stand_in = types.SimpleNamespace(normalize=True, output_std=torch.FloatTensor([out_std]), output_mean=torch.FloatTensor([out_mean]))
    tXtr, tytr, tXt, tyt = (torch.from_numpy(a) for a in (Xtr, ytr, Xt, yt))
    rec = dict((k, []) for k in ('sigmasq', 's', 'theta_mean', 'theta_cov', 'pred_mean', 'pred_var', 'log_density', 'nll', 'rmse',
                                 'nll_as_driver_broadcasts'))
    host_gap = 0.
    for sigmasq, s in ((1.0, 1.0), (0.25, 0.25)):
        head = neural.BayesianRegressionDense([d, 1], sigmasq=sigmasq, s=s)
        with torch.no_grad():
            theta_mean, theta_cov = head._compute_posterior(tXtr, tytr)
            pred_mean, pred_var = head.forward(tXt, tXtr, tytr)
            assert pred_mean.dtype == torch.float64 and pred_var.dtype == torch.float64 and pred_var.shape == (nt, 1)
            ld = neural.NeuralLinear.gaussian_log_density(stand_in, tyt[:, None], pred_mean[:, None], pred_var)
            nll = torch.sum(-ld) / nt
            rmse = neural.NeuralLinear.rmse(stand_in, neural.NeuralLinear.get_unnormalized(stand_in, pred_mean),
                                            neural.NeuralLinear.get_unnormalized(stand_in, tyt))
            quirk = torch.sum(-neural.NeuralLinear.gaussian_log_density(stand_in, tyt, pred_mean, pred_var)) / nt
        assert ld.shape == (nt,) and ld.dtype == torch.float64
        F = np.linalg.cholesky(theta_cov.numpy())
        ref = pc.restate(np.hstack((Xt, yt[:, None])), theta_mean.numpy(), F, sigmasq, 1.)
        l2pi = pc.log_2pi()
        term = -0.5 * (((yt.astype(pc.LD) - ref['mean'][0]) ** 2) / ref['var'][0] + np.log(ref['var'][0]) + l2pi)
        for mine, theirs in ((ref['mean'][0], pred_mean.numpy()), (ref['var'][0], pred_var.numpy()[:, 0]), (term, ld.numpy())):
            host_gap = max(host_gap, float((np.abs(mine - theirs.astype(pc.LD)) / (np.abs(theirs) + 1.)).max()))
        for k, v in (('sigmasq', sigmasq), ('s', s), ('theta_mean', theta_mean.numpy()), ('theta_cov', theta_cov.numpy()),
                     ('pred_mean', pred_mean.numpy()), ('pred_var', pred_var.numpy()[:, 0]), ('log_density', ld.numpy()),
                     ('nll', nll.item()), ('rmse', rmse.item()), ('nll_as_driver_broadcasts', quirk.item())):
            rec[k].append(v)
    assert host_gap <= 1e-12, host_gap
    np.savez_compressed(os.path.join(OUT, 'predict_f24.npz'), Xt=Xt, yt=yt, Xtrain=Xtr, ytrain=ytr, output_std=np.float64(out_std),
                        output_mean=np.float64(out_mean), host_gap=np.float64(host_gap), numpy=np.__version__, torch=torch.__version__,
                        **dict((k, np.array(v)) for k, v in rec.items()))
    print('predict_f24.npz: host_gap %.3g, nll %s, rmse %s (the driver\'s broadcast would report nll %s)'
          % (host_gap, rec['nll'], rec['rmse'], rec['nll_as_driver_broadcasts']))


if __name__ == '__main__':
    main()
