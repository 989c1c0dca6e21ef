"""Shared by tests/test_psvi_many_cpu.py, tests/test_psvi_many_sanitized_cpu.py and tests/test_gpu_psvi_many.py (no test collects
from this file): a runner for tests/psvi_many_harness.cpp, a long-double restatement of stages 3-4 of one step of the batched
BatchPSVI run (include/beta_cores_psvi_many.h) with the bounds both builds are held to, and the ADAM stage as util/opt.py writes
it.  Stage 2 (mode, Theta) is held to tests/vi_laplace_cases.py, the point-gradient to tests/psvi_cases.py; nothing of theirs
is changed.

The bounds of stages 3-4, to first order with u = 2^-53.  Write A[n, s] = |ll(z_n, th_s)| + sum_k |z_nk th_sk|.
  ll[n, s]      the D-term contraction has gamma_D sum_k |z th|, handed on by |dll/dm| <= 1; exp and log1p at <= 2 ulp each
                give 4 u |ll|:  <= (D + 4) u A[n, s].
  c[n, s]       = ll - mean_s ll: the S-term mean adds gamma_S mean |ll| and one division, the subtraction one rounding:
                <= (S + D + 6) u Ac[n, s],   Ac[n, s] = A[n, s] + mean_s A[n, .]   (and |c| <= Ac).
  target[s]     = scale sum_n c[n, s], n_sub terms in a fixed order (tile by tile), one product:
                <= (n_sub + S + D + 7) u scale sum_n Ac[n, s]                                              =: bt[s]
  resid[s]      = target - sum_i w_i cv[i, s], an m-term fma chain and one subtraction, cv the c of the points:
                <= bt[s] + (S + D + m + 8) u sum_i |w_i| Ac_p[i, s] + u scale sum_n Ac[n, s]                =: br[s]
  g_w[i]        = -(sum_s cv[i, s] resid[s]) / S:
                <= (1 / S) sum_s ((S + D + 6) u Ac_p[i, s] |resid_s| + Ac_p[i, s] br[s] + (S + 2) u Ac_p[i, s] |resid_s|)
Every bound is the gamma_k sum |terms| form of tests/psvi_cases.py with k the summation lengths added up; K_SECOND = 2 covers
the second-order terms (gamma_k = k u / (1 - k u), products of two first-order errors).  The reference is evaluated in
np.longdouble: its own error is three decimal orders below."""
import os
import subprocess

import numpy as np

import psvi_cases as pc
import vi_laplace_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ld = np.longdouble
U = 2. ** -53
K_SECOND = 2.
B1, B2, EPS = 0.9, 0.999, 1e-8


def build_harness(outdir, extra=()):
    exe = os.path.join(str(outdir), 'psvi_many_harness')
    cmd = ['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-Wall', '-Werror', '-Wno-unknown-pragmas'] + list(extra) \
        + [os.path.join(ROOT, 'tests', 'psvi_many_harness.cpp'), '-o', exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def make_step(d, m, s, n_sub, seed=0, diag=False, variant=0, step_i=2):
    """One step's inputs: the rows, weights, start and normals of vi_laplace_cases.make_case as the points of a pseudo-coreset,
    n_sub data rows of the same model, moments as a few earlier steps would leave them, the step arrays at iteration step_i."""
    c = lc.make_case(d, m, s, variant=variant, diag=diag)
    rng = np.random.RandomState(77000 + 1000 * d + 10 * m + s + n_sub + seed)
    x = rng.randn(n_sub, d)
    y = np.where(rng.rand(n_sub) < 0.5, 1., -1.)
    return {'key': c['key'], 'd': d, 'm': m, 's': s, 'diag': bool(diag), 'n_sub': n_sub, 'scale': 600. / n_sub, 'pts': c['Z'], 'w': c['w'], 'start': c['start'],
            'E': c['E'], 'rows': y[:, None] * x, 'step_i': step_i, 'step': 1. / (1. + step_i), 'c1': 1. - B1 ** (step_i + 1), 'c2': 1. - B2 ** (step_i + 1),
            'm1w': rng.randn(m) * 0.1, 'm1p': rng.randn(m, d) * 0.1, 'm2w': rng.rand(m) * 0.01, 'm2p': rng.rand(m, d) * 0.01}


def psvi_step_case(kind_case, n_sub=37, seed=1):
    """The same from a LOGISTIC case of tests/psvi_cases.py (its points reach the branch at -z.th >= 100): start = 0."""
    d, m, s = kind_case['d'], kind_case['m'], kind_case['s']
    st = make_step(d, m, s, n_sub, seed=seed)
    st['pts'], st['w'] = kind_case['pts'], kind_case['w']
    del st['key']
    return st


def run_step(exe, st, tmp):
    d, m, s, n_sub = st['d'], st['m'], st['s'], st['n_sub']
    parts = [np.array([d, m, s, 1. if st['diag'] else 0., n_sub, st['scale'], st['step'], st['c1'], st['c2']]), st['pts'], st['w'], st['start'],
             st['E'], st['rows'], st['m1w'], st['m1p'], st['m2w'], st['m2p']]
    fin, fout = os.path.join(str(tmp), 'pm_in.bin'), os.path.join(str(tmp), 'pm_out.bin')
    np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in parts]).tofile(fin)
    out = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stderr == '', (out.returncode, out.stderr[-2000:])
    res = np.fromfile(fout)
    shapes = [('mode', (d,)), ('theta', (s, d)), ('target', (s,)), ('resid', (s,)), ('gw', (m,)), ('gp', (m, d)), ('w', (m,)), ('pts', (m, d)),
              ('m1w', (m,)), ('m1p', (m, d)), ('m2w', (m,)), ('m2p', (m, d))]
    r, at = {'status': int(res[0])}, 1
    for k, shp in shapes:
        n = int(np.prod(shp))
        r[k] = res[at:at + n].reshape(shp)
        at += n
    assert at == res.size
    return r


# ---------------------------------------------------------------- stages 3-4 in long double
def _centred_ld(Z, theta):
    """(c, Ac) of the module docstring for rows Z (float64 values) under theta, both in long double"""
    Zl, Tl = np.asarray(Z, dtype=ld), np.asarray(theta, dtype=ld)
    prod = Zl[:, None, :] * Tl[None, :, :]
    mm, pabs = -prod.sum(axis=2), np.abs(prod).sum(axis=2)
    small = mm < 100
    ll = -mm
    ll[small] = -np.log1p(np.exp(mm[small]))
    A = np.abs(ll) + pabs
    return ll - ll.mean(axis=1)[:, None], A + A.mean(axis=1)[:, None]


def reference_stage34(rows, scale, pts, w, theta):
    """dict of target, resid, gw (long double) and their bounds bt, br, bg for the GIVEN theta (the device's own draw)"""
    n_sub, d = rows.shape
    m, s = pts.shape[0], theta.shape[0]
    c, Ac = _centred_ld(rows, theta)
    cv, Acp = _centred_ld(pts, theta)
    wl, sc = np.asarray(w, dtype=ld), ld(scale)
    tabs = sc * Ac.sum(axis=0)
    target = sc * c.sum(axis=0)
    resid = target - wl.dot(cv)
    gw = -cv.dot(resid) / s
    bt = (n_sub + s + d + 7) * U * tabs
    br = bt + (s + d + m + 8) * U * np.abs(wl).dot(Acp) + U * tabs
    bg = ((2 * s + d + 8) * U * Acp.dot(np.abs(resid)) + Acp.dot(br)) / s
    return dict(target=target, resid=resid, gw=gw, cv=cv, bt=K_SECOND * bt, br=K_SECOND * br, bg=K_SECOND * bg)


def check_stage34(label, rows, scale, pts, w, theta, target, resid, gw):
    """Asserts the three against reference_stage34; returns the worst error / bound ratios (target, resid, g_w)."""
    assert pc.LD_OK
    ref = reference_stage34(rows, scale, pts, w, theta)
    out = []
    for name, got, bound in (('target', target, ref['bt']), ('resid', resid, ref['br']), ('gw', gw, ref['bg'])):
        err = np.abs(np.asarray(got, dtype=ld) - ref[name])
        ratio = float((err / np.maximum(bound, np.finfo(np.float64).tiny)).max())
        print('%s %s: worst error %.3e, worst error / bound %.3e' % (label, name, float(err.max()), ratio))
        assert np.all(err <= bound), (label, name, ratio)
        out.append(ratio)
    return out


def check_point_grad(label, pts, w, theta, resid, gp):
    """g_p under tests/psvi_cases.py's reference and bound on the GIVEN resid (the device's own)."""
    c = {'kind': pc.LOGISTIC, 'm': pts.shape[0], 's': theta.shape[0], 'd': pts.shape[1], 'sigsq': 1., 'pts': pts, 'theta': theta, 'w': w, 'resid': resid}
    ref, bound = pc.reference(c)
    err = np.abs(np.asarray(gp, dtype=ld) - ref)
    ratio = float((err / np.maximum(bound, np.finfo(np.float64).tiny)).max())
    print('%s g_p: worst error %.3e, worst error / bound %.3e' % (label, float(err.max()), ratio))
    assert np.all(err <= bound), (label, ratio)
    return ratio


def reference_mode(c):
    """mu* in long double for points and weights that are no case of vi_laplace_cases' grid: that module's iteration (damped
    Newton from 0, its backtracking -- but a full step once the decrement is below the rounding floor of f), ended where its step
    has reached long double's rounding floor -- it no longer halves from one iteration to the next and is below
    1e-13 (1 + max|mu|), four orders under the smallest mode bound -- instead of at that module's fixed threshold, which the
    weights N / m of a pseudo-coreset (600 on one point) put below the floor."""
    keep = c['w'] > 0
    Z, w = np.asarray(c['Z'][keep], dtype=ld), np.asarray(c['w'][keep], dtype=ld)
    mu = np.zeros(c['d'], dtype=ld)

    def value(th):
        mm = -Z.dot(th)
        return -(w * (np.maximum(mm, 0.) + np.log1p(np.exp(-np.fabs(mm))))).sum() - ld(0.5) * th.dot(th)
    f, last = value(mu), np.inf
    for _ in range(500):
        mm = -Z.dot(mu)
        p = ld(0.5) * (ld(1.) + np.tanh(ld(0.5) * mm))
        g = -mu + Z.T.dot(w * p)
        Cf = lc._chol_ld(lc.hessian_ld(c, mu))
        step = lc._solve_upper(Cf.T, lc._solve_lower(Cf, g))
        t, dec = ld(1.), g.dot(step)
        while True:
            cand = mu + t * step
            fc = value(cand)
            # (a decrement below the rounding floor of f: the comparison would backtrack in noise -- with 600 on one point
            # f is ~5e3 and a step of 1e-12 changes it by 1e-21 -- so Newton's full step is taken, which converges
            # quadratically this close to the mode)
            if fc >= f + ld(1e-4) * t * dec or t < 1e-10 or dec <= 1e3 * np.finfo(ld).eps * (1. + np.fabs(f)):
                break
            t *= ld(0.5)
        mu, f = cand, fc
        size, scale = float(np.fabs(step).max()), 1. + float(np.fabs(mu).max())
        if size <= 1e-17 * scale or (size <= 1e-13 * scale and size > 0.5 * last):
            return mu
        last = size
    raise AssertionError('the long-double Newton iteration did not converge')


def check_mode_and_draw(label, pts, w, E, diag, mode, theta, key=None):
    """mode and Theta under tests/vi_laplace_cases.py's bounds (mode_bound; vi_sampler_cases.draw_bound around the GIVEN mode).
    `key`: the points and weights are that case of its grid, whose cached reference mode is used; otherwise reference_mode."""
    import vi_sampler_cases as vc
    assert vc.LD_OK
    c = {'d': pts.shape[1], 'm': pts.shape[0], 's': E.shape[0], 'Z': pts, 'w': w, 'start': np.zeros(pts.shape[1]), 'E': E, 'diag': bool(diag)}
    if key is not None:
        c['key'] = key
        return lc.check_mode_and_draw(c, mode, theta, label)
    mu_ref = reference_mode(c).astype(np.float64)
    err_m, bound_m = np.abs(mode - mu_ref).max(), lc.mode_bound(c, mu_ref)
    ref, kappa = lc.reference_draw(c, mode)
    err_d, bound_d = np.abs((theta - mode) - ref).max(), vc.draw_bound(c['d'], kappa, ref)
    print('%s: mode error %.3e (bound %.3e), draw error %.3e (bound %.3e), kappa %.3e' % (label, err_m, bound_m, err_d, bound_d, kappa))
    assert err_m <= bound_m, (label, err_m, bound_m)
    assert err_d <= bound_d, (label, err_d, bound_d)
    return err_m / bound_m, err_d / bound_d


# ---------------------------------------------------------------- stage 5 as util/opt.py writes it
def adam_step(x, g, mom1, mom2, step, i, nn):
    """One iteration of beta_cores_amd.util.opt._adam_loop on x (its statements, NumPy doubles): returns (x, mom1, mom2).
    step: step_sched(i); nn: the indices projected to >= 0."""
    mom1 = B1 * mom1 + (1. - B1) * g
    mom2 = B2 * mom2 + (1. - B2) * g ** 2
    upd = step * mom1 / (1. - B1 ** (i + 1)) / (EPS + np.sqrt(mom2 / (1. - B2 ** (i + 1))))
    x = x - upd
    x[nn] = np.maximum(x[nn], 0.)
    return x, mom1, mom2


def ulps(a, b):
    """|a - b| in units of the spacing of b (0 where both are equal, zeros of either sign included)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.where(a == b, 0., np.abs(a - b) / np.spacing(np.maximum(np.abs(b), np.finfo(np.float64).tiny)))
