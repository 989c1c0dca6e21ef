"""Shared by tests/test_laplace_many_cpu.py and tests/test_gpu_laplace_many.py (no test collects from this file): batches of
the cases of tests/vi_laplace_cases.py, the bounds the factors of a batched Laplace fit are held to, and a runner for
tests/laplace_many_harness.cpp.

The factor bounds.  With S_jk = sum_n w_n |z_nj z_nk| and H*, C* = chol(H*), L* = C*^-1 evaluated in long double around the
RETURNED mu (as lc.reference_draw does: the mode's own error is lc.mode_bound's business):

    |H - H*|_jk        <= K_H 2^-53 (1 + S_jk)
    max |C - C*|       <= K_C budget ||C*||_2,     budget = D 2^-53 (1 + max_jk (1 + S_jk) ||L*||_2^2)
    max |L - L*|       <= K_L budget ||L*||_2

The H term: w p (1 - p) evaluated in double carries an absolute error of a few ulps of w per row, so an entry of H is off by a
few ulps of S_jk whatever the summation order.  The factor terms are the perturbation bound of a Cholesky factor,
||dC|| <~ ||dH|| ||L||^2 ||C||, with dH from the line above plus the factorisation's own D eps ||H||; at weights of 1e4 the
first dominates.  The constants are not fitted to the code under test: each is 16 x the worst ratio of the EXISTING host code,
samplers.logistic_laplace(solver='newton') on host arrays, over lc.grid() + lc.extra_cases(), rounded up to a power of two --
the rule that produced lc.C_MODE.  test_host_newton_sets_the_factor_constants recomputes the ratios and pins the constants."""
import os
import subprocess

import numpy as np

import vi_laplace_cases as lc
import vi_sampler_cases as vc

ROOT = lc.ROOT
ld = np.longdouble
K_H, K_C, K_L = 32., 4., 4.
# (H, C, L) ratios of the host fit at K = 1, as the test prints them (profiles/laplace_many_notes.md).  The C ratio is that of
# D = 1, m = 1, where C = sqrt(H) is half an ulp off and the budget is two ulps; from D = 2 on it stays below 0.085.
HOST_WORST = (1.517, 0.220, 0.158)


def constant_of(worst_ratio):
    """16 x the worst ratio, rounded up to a power of two."""
    return 2. ** np.ceil(np.log2(16. * worst_ratio))


def factor_refs(c, mu):
    """(H*, C*, L*, S) around the given mu; the first three in long double."""
    H = lc.hessian_ld(c, mu)
    Cf = lc._chol_ld(H)
    d = c['d']
    L = np.zeros((d, d), dtype=ld)
    for i in range(d):
        e = np.zeros(d, dtype=ld)
        e[i] = 1.
        L[i] = (e - Cf[i, :i].dot(L[:i])) / Cf[i, i]
    keep = c['w'] > 0
    aZ = np.abs(c['Z'][keep])
    S = (aZ * c['w'][keep][:, None]).T.dot(aZ)
    return H, Cf, L, S


def factor_ratios(c, mu, H=None, hdiag=None, C=None, L=None):
    """error / bound at K = 1 of what is given: a dict with keys among 'H' (the full matrix, or its diagonal hdiag), 'C', 'L'."""
    assert vc.LD_OK
    Hs, Cs, Ls, S = factor_refs(c, mu)
    out = {}
    if H is not None:
        out['H'] = float((np.abs(np.asarray(H, dtype=ld) - Hs) / (2. ** -53 * (1. + S))).max())
    if hdiag is not None:
        out['H'] = float((np.abs(np.asarray(hdiag, dtype=ld) - np.diag(Hs)) / (2. ** -53 * (1. + np.diag(S)))).max())
    nC, nL = np.linalg.norm(Cs.astype(np.float64), 2), np.linalg.norm(Ls.astype(np.float64), 2)
    budget = c['d'] * 2. ** -53 * (1. + (1. + S).max() * nL ** 2)
    if C is not None:
        out['C'] = float(np.abs(np.asarray(C, dtype=ld) - Cs).max() / (budget * nC))
    if L is not None:
        out['L'] = float(np.abs(np.asarray(L, dtype=ld) - Ls).max() / (budget * nL))
    return out


def check_factors(c, mu, hdiag, C=None, L=None, label=''):
    """Holds hdiag (and C, L when given) to the three bounds; returns the ratios error / bound (with the constants in)."""
    r = factor_ratios(c, mu, hdiag=hdiag, C=C, L=L)
    K = {'H': K_H, 'C': K_C, 'L': K_L}
    r = {k: v / K[k] for k, v in r.items()}
    print('%s D %3d m %3d max w %g: error / bound %s' % (label, c['d'], c['m'], c['w'].max(), ', '.join('%s %.3g' % kv for kv in sorted(r.items()))))
    for k, v in r.items():
        assert v <= 1., (label, c.get('key'), k, v)
    return r


def with_normals(c, E, diag=None):
    """Case c with the draw's normals replaced (the rows, weights, start and key -- hence the cached reference mode -- stay)."""
    c = dict(c)
    c['E'], c['s'] = E, E.shape[0]
    if diag is not None:
        c['diag'] = bool(diag)
    return c


def cases_of_dim(d):
    """The batch of dimension d: lc.make_case(d, m, s, variant) for (m, s) in the first three of lc.SHAPES with the grid's own
    variants, and at d = 16 the far start and the large margins."""
    cs = [lc.make_case(d, m, s, variant=i + d) for i, (m, s) in enumerate(lc.SHAPES[:3])]
    return cs + (lc.extra_cases() if d == 16 else [])


def problems_of(cases):
    return [(c['Z'], c['w']) for c in cases], np.array([c['start'] for c in cases])


def build_harness(outdir, extra=(), name='laplace_many_harness'):
    exe = os.path.join(str(outdir), name)
    cmd = ['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-Wall', '-Werror'] + list(extra) \
        + [os.path.join(ROOT, 'tests', 'laplace_many_harness.cpp'), '-o', exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def run_harness(exe, cases, E, tmp, diag=False, env=None):
    """The host build of the four stages over the packed batch `cases` (common D).  E: S x D (all problems read it) or
    P x S x D.  Returns one dict per problem: status, and for status 0 mu, value, hdiag, chol, inv (None with diag), counts,
    draws; for a refused problem `untouched` (its block kept the filler)."""
    d, P = cases[0]['d'], len(cases)
    shared = E.ndim == 2
    s = E.shape[-2]
    row_ptr = np.concatenate(([0], np.cumsum([c['m'] for c in cases])))
    parts = [np.array([d, P, s, 1. if diag else 0., 1. if shared else 0.]), row_ptr] + [c['Z'].ravel() for c in cases] \
        + [c['w'] for c in cases] + [c['start'] for c in cases] + [E.ravel()]
    fin, fout = os.path.join(str(tmp), 'lm_in.bin'), os.path.join(str(tmp), 'lm_out.bin')
    np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in parts]).tofile(fin)
    out = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and out.stderr == '', (out.returncode, out.stderr[-2000:])
    block = 1 + d + 1 + d + 2 * d * d + 3 + s * d
    res = np.fromfile(fout).reshape(P, block)
    outs = []
    for r in res:
        if int(r[0]) != 0:
            outs.append({'status': int(r[0]), 'untouched': bool(np.all(r[1:] == 7.0))})
            continue
        o = 1
        mu = r[o:o + d]; o += d
        value = r[o]; o += 1
        hd = r[o:o + d]; o += d
        chol = r[o:o + d * d].reshape(d, d); o += d * d
        inv = r[o:o + d * d].reshape(d, d); o += d * d
        counts = r[o:o + 3].astype(int); o += 3
        if diag:
            assert np.all(chol == 7.0) and np.all(inv == 7.0)
        outs.append({'status': 0, 'mu': mu, 'value': value, 'hdiag': hd, 'chol': None if diag else chol, 'inv': None if diag else inv,
                     'counts': counts, 'draws': r[o:].reshape(s, d)})
    return outs
