"""The batch cases the tests of the batched small-problem HMC run share (include/beta_cores_hmc_small.h, csrc/bc_hmc_small_dev.h),
their references from the restatement of tests/hmc_cases.py, and the build of tests/hmc_small_harness.cpp.
Test infrastructure only: the product never imports this module."""
import functools
import os
import subprocess

import numpy as np

import hmc_cases as hc

ROOT = hc.ROOT

# (name, D, n_p, C, L, T, eps, seed).  Problem p: rows and weights hc.make_data(n_p, D, seed + p); r = RandomState(seed + 200 + p):
# start = r.randn(C, D) * 0.1, inv_mass = 0.5 + r.rand(D); its step eps (1 + 0.25 p).  The shared draws: RandomState(seed + 100),
# randn(T, C, D) then log(rand(T, C)).  Covered: one-row problems, both sides of the 64-row segment edge (64 | 65), the largest
# square problem (128 x 128), both dimension limits, a problem that rejects everything beside one that accepts everything (d1).
# On the float64 restatement: 56 / 90, 228 / 256, 15 / 16 and 6 / 12 proposals accepted, the smallest |logU - (H0 - H1)| 6.2e-3,
# 1.7e-4, 0.13 and 0.26 (asserted by check_batch_condition below: > 1e-6 per problem, both kinds of decision per batch).
BATCH_CASES = [
    ('ragged5', 5, (1, 7, 64, 65, 300), 3, 4, 6, 0.25, 21),
    ('wide128', 128, (1, 33, 100, 128), 16, 4, 4, 0.08, 22),
    ('d256', 256, (2, 60), 2, 3, 4, 0.06, 23),
    ('d1', 1, (1, 1000), 1, 2, 6, 0.6, 24),
    # a batch whose block of FOUR chains fits the LDS (D = 128, at most 100 rows, C = 4): the case of the chain-packing test,
    # 43 / 48 accepted, smallest margin 2.4e-2
    ('pack128', 128, (5, 40, 100), 4, 3, 4, 0.08, 25),
]
BATCH_NAMES = [t[0] for t in BATCH_CASES]


@functools.lru_cache(maxsize=None)
def make_batch_case(name):
    """dict(name, d, c, L, T, E, logU, problems): every problem a case dict as hc.make_trace_case's (the shared E, logU in each)."""
    return build_batch(*[t for t in BATCH_CASES if t[0] == name][0])


def build_batch(name, d, ns, c, L, T, eps, seed):
    """The recipe of BATCH_CASES for any shape."""
    rng = np.random.RandomState(seed + 100)
    E = rng.randn(T, c, d)
    logU = np.log(rng.rand(T, c))
    problems = []
    for p, n in enumerate(ns):
        Z, w = hc.make_data(n, d, seed + p)
        r = np.random.RandomState(seed + 200 + p)
        start = r.randn(c, d) * 0.1
        problems.append(dict(name='%s[%d]' % (name, p), Z=Z, w=w, start=start, inv_mass=0.5 + r.rand(d), eps=eps * (1. + 0.25 * p), L=L,
                             E=E, logU=logU))
    return dict(name=name, d=d, c=c, L=L, T=T, E=E, logU=logU, problems=problems)


@functools.lru_cache(maxsize=None)
def batch_reference(name):
    """Per problem (reference, tol_samples, tol_logjoint) of hc.trace_tolerance: computed once, shared, never modified."""
    return [hc.trace_tolerance(pr) for pr in make_batch_case(name)['problems']]


def check_batch_condition(refs):
    """The conditions on the inputs: per problem no decision within 1e-6 of flipping, per batch decisions of both kinds."""
    for ref, _, _ in refs:
        assert np.all(np.isfinite(ref['margin'])) and np.abs(ref['margin']).min() > 1e-6, np.abs(ref['margin']).min()
    acc = np.concatenate([ref['accept'].ravel() for ref, _, _ in refs])
    assert acc.any() and not acc.all(), 'the batch needs accepted and rejected proposals'


def pack(problems):
    """(rows, w, row_ptr, start [P, C, D], inv_mass [P, D], eps [P]) of a list of problem dicts; w=None becomes ones."""
    rows = np.ascontiguousarray(np.concatenate([pr['Z'] for pr in problems], axis=0), dtype=np.float64)
    w = np.concatenate([np.ones(pr['Z'].shape[0]) if pr['w'] is None else np.asarray(pr['w'], dtype=np.float64) for pr in problems])
    row_ptr = np.concatenate(([0], np.cumsum([pr['Z'].shape[0] for pr in problems]))).astype(np.int64)
    start = np.ascontiguousarray(np.array([pr['start'] for pr in problems]), dtype=np.float64)
    im = np.ascontiguousarray(np.array([pr['inv_mass'] for pr in problems]), dtype=np.float64)
    return rows, w, row_ptr, start, im, np.array([pr['eps'] for pr in problems], dtype=np.float64)


def compare_with_reference(got, ref, tol_s, tol_l, start, label=''):
    """Accept flags equal; positions and log-joints within the trace tolerance; a rejected chain keeps its bits."""
    acc = got['accept'] != 0
    assert np.array_equal(acc, ref['accept']), label
    ds, dl = hc.rel_dev(got['samples'], ref['samples']), hc.rel_dev(got['logjoint'], ref['logjoint'])
    print('%s: samples %.3g (tol %.3g), logjoint %.3g (tol %.3g)' % (label, ds, tol_s, dl, tol_l))
    assert ds <= tol_s and dl <= tol_l, (label, ds, tol_s, dl, tol_l)
    prev = np.vstack((np.asarray(start)[None], got['samples'][:-1]))
    assert np.array_equal(got['samples'][~acc], prev[~acc]), label
    assert np.array_equal(got['logjoint'][1:][~acc[1:]], got['logjoint'][:-1][~acc[1:]]), label


# ------------------------------------------------------------------ the host build of csrc/bc_hmc_small_dev.h + csrc/bc_hmc_dev.h
def build_harness(outdir, extra=()):
    exe = os.path.join(str(outdir), 'hmc_small_harness')
    cmd = ['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-Wall', '-Werror'] + list(extra) \
        + [os.path.join(ROOT, 'tests', 'hmc_small_harness.cpp'), '-o', exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def run_harness(exe, problems, tmp):
    """The host build on a batch with shared draws: a list with, per problem, dict(status, samples, logjoint, accept)."""
    rows, w, row_ptr, start, im, eps = pack(problems)
    P, c, d = start.shape
    E, logU, L = problems[0]['E'], problems[0]['logU'], problems[0]['L']
    T = E.shape[0]
    head = np.array([P, d, c, L, T], dtype=np.float64)
    parts = [head, row_ptr, rows, w, start, im, eps, E, logU]
    fin, fout = os.path.join(str(tmp), 'hmc_small_in.bin'), os.path.join(str(tmp), 'hmc_small_out.bin')
    np.concatenate([np.asarray(x, dtype=np.float64).ravel() for x in parts]).tofile(fin)
    out = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stderr == '', (out.returncode, out.stderr[-2000:])
    res = np.fromfile(fout)
    assert res.size == P + P * T * c * (d + 2)
    status = res[:P].astype(int)
    s = res[P:P + P * T * c * d].reshape(P, T, c, d)
    lj = res[P + P * T * c * d:P + P * T * c * (d + 1)].reshape(P, T, c)
    acc = res[P + P * T * c * (d + 1):].reshape(P, T, c) != 0
    return [dict(status=int(status[p]), samples=s[p], logjoint=lj[p], accept=acc[p]) for p in range(P)]


# ------------------------------------------------------------------ the restatement behind samplers.logistic_hmc_many
class MarginEngine(hc.NumpyHMCEngine):
    """NumpyHMCEngine that also keeps logU - (H0 - H1) of every decision it made (the condition of an agreement test)."""

    def __init__(self, Z, wts):
        super().__init__(Z, wts)
        self.margins = []

    def chunk(self, normals, log_u, step):
        self.margins.append(hc.hmc_run(self.Z, self.w, self.th, self.im, step, self.L, normals, log_u, dtype=np.float64)['margin'])
        return super().chunk(normals, log_u, step)


class MarginEngines:
    """An engine factory that keeps the MarginEngines it made, in order."""

    def __init__(self):
        self.made = []

    def __call__(self, Z, wts):
        self.made.append(MarginEngine(Z, wts))
        return self.made[-1]

    def min_margin(self):
        m = np.concatenate([np.abs(x).ravel() for e in self.made for x in e.margins])
        assert np.all(np.isfinite(m))
        return float(m.min())


# ------------------------------------------------------------------ the statistical guard
GUARD = dict(P=8, n=40, d=4, c=16, L=8, step=0.3, n_samples=300, drop=100, seed=40, weight_scale=25., rng_seed=90)


@functools.lru_cache(maxsize=None)
def guard_problems():
    # The Laplace variance here is diag(LSig^T LSig), NOT the diag(LSig LSig^T) of tests/test_gpu_hmc.py::test_statistical_guard.
    # logistic_laplace returns LSig = chol(H)^-1 (lower triangular), so the covariance of the Laplace approximation, H^-1, is
    # LSig^T LSig; LSig LSig^T is the covariance of mu + randn . LSig^T, the drivers' draw.  The two have the same diagonal only
    # when H is close to diagonal, as it is for that test's 20 000 unit-weight rows; for these 40-row weighted coresets the
    # coordinates are correlated, and measured against diag(LSig LSig^T) the float64 restatement itself -- an exact-posterior
    # sampler -- shows variance ratios of 0.54 .. 1.6.  HMC samples the posterior, so H^-1 is what its variance is compared with.
    """Eight weighted coresets of 40 rows, D = 4, with weights of coreset size (x 25: they sum to about 800, which makes each
    posterior close to its Laplace approximation -- the guard compares against that), and per problem the Newton mode, the
    Laplace VARIANCES diag(H^-1) (H minus the Hessian at the mode; LSig = chol(H)^-1, so H^-1 = LSig^T LSig) and LSig."""
    from beta_cores_amd import samplers
    g = GUARD
    probs, fits = [], []
    for p in range(g['P']):
        Z, w = hc.make_data(g['n'], g['d'], g['seed'] + p)
        w = w * g['weight_scale']
        mode, LSig, _ = samplers.logistic_laplace(w, Z, np.zeros(g['d']), solver='newton')
        probs.append((Z, w))
        fits.append((mode, np.diag(LSig.T.dot(LSig)), LSig))
    return probs, fits


def check_guard(results, fits, label):
    """test_statistical_guard's bars, per problem: the pooled mean within 0.25 Laplace sd of the Newton mode, the pooled variance
    within [0.8, 1.25] of the Laplace variance, over the iterations after the dropped ones."""
    for p, (r, (mode, var, _)) in enumerate(zip(results, fits)):
        kept = r.samples[GUARD['drop']:].reshape(-1, GUARD['d'])
        shift, ratio = (kept.mean(axis=0) - mode) / np.sqrt(var), kept.var(axis=0) / var
        print('%s guard, problem %d: mean shift %s sd, variance ratio %s, acceptance %.3f' %
              (label, p, np.round(shift, 3), np.round(ratio, 3), r.accept_rate.mean()))
        assert np.all(np.abs(shift) <= 0.25) and np.all(ratio >= 0.8) and np.all(ratio <= 1.25), (p, shift, ratio)
