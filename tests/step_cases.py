"""Reference, running error bound, planted list states, case lists and a loop model for the tests of the greedy step: the
single-block kernels k_step_finish_pf<alg, RS>, k_step_finish<alg>, k_reweight<alg> and k_set_weights of
beta_cores_amd/csrc/bc_snnls.hip and their stages in bc_snnls_dev.h (dev_xw_err_t, dev_step_sizes, dev_apply, dev_prep); no test in
here.  tests/test_step_cases_cpu.py holds the cases themselves (conditions, not measurements) and three mutants of the xw
rebuild; tests/test_gpu_step.py runs the cases on the device in every form of the finish kernel.

THE REFERENCE STEP is giga.py:20-64 / frankwolfe.py:16-40 from a list state (idx, val), the columns Phi[idx], b and the picked row
f, written once (ref_step) over a number type that carries a value and an absolute error bound (class E).  Run in np.longdouble
the values are the reference and the bounds say how far honest float64 may land; run in float64 the values are what NumPy gives
for the same formulas (the CPU test holds them inside the bound).

THE BOUND is first order, u = 2^-53, with every input error propagated:
    a sum of L products, in any order, fma or not     (L + 2) u sum |a_k b_k|  + sum (|a_k| e_b + |b_k| e_a + e_a e_b)
    a product, a sum, a difference                    u |result| + the propagated terms
    a quotient a / b                                  u |result| + (e_a + |result| e_b) / (|b| - e_b)
    a square root                                     u |result| + e_a / (sqrt(a) + sqrt(a - e_a))
so gA = bxf - bxw xwxf, gB, gA + gB and FrankWolfe's num and den carry ABSOLUTE errors through their cancellations.  The device
forms its quantities as the reference step does: xw by G = 512 / S group chains over the list combined in group order (a sum of
nnz products), ||xw||^2 and ||xw - b||^2 from that xw (sums of S products), the row norms and GIGA's nf as sqrt of S squares, the
sum of the norms over the n rows, bn = b / ||b|| on the host, and dev_step_sizes term by term.  The final factor 1.01 (as in
k1_cases.py) covers the second order and the reference's own rounding (2^-64 per operation).  Derived, not tuned: a weight or an
error outside it is a finding.  A second step is bounded from the list the device returned after the first, so bounds do not
compound.

THE PLANTED STATE (planted).  n = nnz + 256 rows, correlated like test_seeded_parity_vs_oracle's Phi plus a common mean, NOT centred
(a centred row of S = 2 or 3 elements has one or two degrees of freedom).  The list is the first nnz rows of a permutation
(scrambled, not ascending); its weights are (n / nnz) U(0.5, 1.5), for FrankWolfe scaled onto the polytope sum w_j |x_j| =
sum |x_i| (then the exact line search cannot leave [0, 1]: the iterate is a convex combination of the vertices).  The winner is
MADE.  A unit vector e is drawn to be the sweep direction (GIGA's cdir, FrankWolfe's residual), every row's component a along e is
cut to at most CUT = 0.4 of the norm of its part orthogonal to the sweep vectors, so that it scores at most 0.372 of the largest
score possible, and the chosen row is e + 0.3 g (g a unit vector orthogonal to the sweep vectors; GIGA: + 0.5 xw / |xw|), which
scores 0.958 of it and leaves a new error well above rounding.  Then b is GIVEN to the solver so that e is the direction: for
FrankWolfe b = xw + rho e; for GIGA the negative a of the listed rows are scaled until sum_j w_j a_j = 0, so that xw is
orthogonal to e, and b = |xw| (cos 0.3 xw / |xw| + sin 0.3 e).  xw is rounded when b is formed, which turns the direction by
1e-13 at the most; the outcome is checked, not assumed: the CPU test holds the margin in np.longdouble for every case.
"""
import functools

import numpy as np

from sweep_cases import LD, LONGDOUBLE_OK, LONGDOUBLE_WHY, U      # noqa: F401  (the guard is sweep_cases.py's)

FIN_THREADS = 512        # BC_FIN_THREADS
PF_NC = 16               # BC_PF_NC
PF_MAXNNZ = 1024         # BC_PF_MAXNNZ: the one-round kernels serve nnz_upper + 1 <= 1024
FACTOR = 1.01
PLAIN, ONE_ROUND, ONE_ROUND_RESCORE, ONE_ROUND_BB = 1, 2, 3, 4       # include/beta_cores.h: BC_FINISH_*
ALGS = ('giga', 'fw')
KINDS = ('fresh', 'revisit_head', 'revisit_behind', 'zeros', 'all_zero')
EXTRA_ROWS = 256
CUT = 0.4


def groups(S):
    return max(1, FIN_THREADS // S)


# ------------------------------------------------------------------ a value with its error bound
class E(object):
    """value v (array or scalar of the run's dtype) and a bound e on |device value - v|, first order (module docstring)"""
    __slots__ = ('v', 'e')
    __array_ufunc__ = None               # ndarray (op) E defers to E's reflected method

    def __init__(self, v, e=None):
        self.v = v
        self.e = np.zeros_like(v) if e is None else e

    @staticmethod
    def of(x):
        return x if isinstance(x, E) else E(np.asarray(x))

    def __add__(self, o):
        o = E.of(o)
        v = self.v + o.v
        return E(v, U * np.abs(v) + self.e + o.e)

    def __sub__(self, o):
        o = E.of(o)
        v = self.v - o.v
        return E(v, U * np.abs(v) + self.e + o.e)

    def __rsub__(self, o):
        return E.of(o) - self

    def __radd__(self, o):
        return self + o

    def __rmul__(self, o):
        return self * o

    def __rtruediv__(self, o):
        return E.of(o) / self

    def __mul__(self, o):
        o = E.of(o)
        v = self.v * o.v
        return E(v, U * np.abs(v) + np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    def __truediv__(self, o):
        o = E.of(o)
        v = self.v / o.v
        lo = np.abs(o.v) - o.e
        assert np.all(lo > 0), 'a divisor that its own error bound lets reach zero'
        return E(v, U * np.abs(v) + (self.e + np.abs(v) * o.e) / lo)

    def __getitem__(self, k):
        return E(self.v[k], self.e[k])

    def bound(self):
        return FACTOR * self.e


def esqrt(a):
    v = np.sqrt(a.v)
    s = v + np.sqrt(np.maximum(a.v - a.e, 0))
    pos = s > 0
    return E(v, U * v + np.where(pos, a.e / np.where(pos, s, 1), np.sqrt(a.e)))


def edot(a, b, axis=None):
    """sum of L products in any order, fma or not"""
    a, b = E.of(a), E.of(b)
    t = a.v * b.v
    L = t.shape[-1] if axis is not None else t.size
    return E(t.sum(axis=axis), (L + 2) * U * np.abs(t).sum(axis=axis)
             + (np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e).sum(axis=axis))


def esum(a):
    return E(a.v.sum(), (a.v.size + 2) * U * np.abs(a.v).sum() + a.e.sum())


def xw_of(w, cols, shared=None):
    """xw = sum_j w_j cols_j and its bound: nnz products per element, the weights' errors propagated -- entry by entry, or,
    where the weights are alpha w_j (+ beta at one entry) with ONE alpha and beta, as what these two move in common:
    shared = (|alpha's error| |old xw| + |beta's error| |xf|, the weights' own rounding errors)"""
    nnz, S = cols.shape
    if nnz == 0:
        return E(np.zeros(S, dtype=cols.dtype))
    t = w.v[:, None] * cols
    chain = (nnz + 2) * U * np.abs(t).sum(axis=0)
    if shared is None:
        return E(t.sum(axis=0), chain + (np.abs(cols) * w.e[:, None]).sum(axis=0))
    common, own = shared
    return E(t.sum(axis=0), chain + common + (np.abs(cols) * own[:, None]).sum(axis=0))


# ------------------------------------------------------------------ the reference step
def list_state(b, w, cols, shared=None):
    """what dev_xw_err leaves for a list: xw, err = ||xw - b||, ||xw||^2, the positive count"""
    xw = xw_of(w, cols, shared)
    d = xw - b
    return dict(xw=xw, err=esqrt(edot(d, d)), xw_sq=edot(xw, xw), npos=int((w.v > 0).sum()))


def next_vectors(alg, b, bn, st):
    """dev_prep: the vectors of the next sweep -- (cdir, xw / |xw|) and whether _select raises (|cdir| below tol is the caller's
    business: the norm is returned), or the residual"""
    if alg == 'giga':
        nw = esqrt(st['xw_sq'])
        if nw.v == 0:
            nw = E(np.ones_like(nw.v))
        xn = st['xw'] / nw
        c = bn - edot(bn, xn) * xn
        cn = esqrt(edot(c, c))
        return dict(v0=c / cn, v1=xn, cn=cn)
    return dict(v0=b - st['xw'])


def ref_step(alg, phi, b, idx, val, f, dtype=None):
    """One reweight from the list (idx, val), columns phi[idx], for the picked row f.  Returns a dict: pre (list_state before),
    ok (the reference would not raise), g (gA, gB or num, den), alpha, beta, idx1, w1 (E), at_new (the appended slot or -1), post
    (list_state after), nxt (next_vectors after).  dtype np.longdouble (default): reference and bounds; np.float64: NumPy's own
    evaluation of the same formulas."""
    dtype = LD if dtype is None else dtype
    idx = np.asarray(idx, dtype=np.int64)
    P = np.asarray(phi, dtype=dtype)
    b = np.asarray(b, dtype=dtype)
    w = E(np.asarray(val, dtype=dtype))
    cols = P[idx]
    xf = P[f]
    bnorm = esqrt(edot(b, b))
    bn = E.of(b) / bnorm
    pre = list_state(b, w, cols)
    xw = pre['xw']
    out = dict(pre=pre, f=int(f))
    if alg == 'giga':
        nw = esqrt(pre['xw_sq'])
        if nw.v == 0:
            nw = E(np.ones_like(nw.v))
        nf = esqrt(edot(xf, xf))
        fn, wn = E.of(xf) / nf, xw / nw
        bxf, bxw, xwxf = edot(bn, fn), edot(bn, wn), edot(wn, fn)
        gA = bxf - bxw * xwxf
        gB = bxw - bxf * xwxf
        out['g'] = (gA, gB)
        out['ok'] = bool(gA.v > 0 and gB.v >= 0)
        out['safe'] = bool(gA.v - gA.bound() > 0 and (gB.v - gB.bound() >= 0 or (gB.v == 0 and gB.e == 0)))
        if not out['ok']:
            return out
        den = gA + gB
        a_ = gB / den / nw
        b_ = gA / den / nf
        x = a_ * xw + b_ * xf
        nx = esqrt(edot(x, x))
        scale = bnorm / nx * edot(x / nx, bn)
        alpha, beta = a_ * scale, b_ * scale
    else:
        nrm = esqrt(edot(P, P, axis=1))
        nsum = esum(nrm)
        nf = nrm[f]
        if pre['npos'] == 0:
            alpha, beta = E(np.zeros((), dtype=dtype)), nsum / nf
            out['g'] = None
            out['ok'] = out['safe'] = True
        else:
            c = nsum / nf
            d = c * xf - xw
            num, den = edot(d, b - xw), edot(d, d)
            out['g'] = (num, den)
            out['ok'] = bool(0 <= num.v <= den.v and den.v > 0)
            out['safe'] = bool(num.v - num.bound() >= 0 and den.v - den.bound() > 0 and num.v + num.bound() <= den.v - den.bound())
            if not out['ok']:
                return out
            q = num / den
            alpha, beta = 1 - q, c * num / den
    out['alpha'], out['beta'] = alpha, beta
    w1 = alpha * w
    own = U * np.abs(w1.v)                                     # each product alpha w_j rounds on its own ...
    common = alpha.e * np.abs(xw.v) + alpha.e * xw.e           # ... and alpha's error moves the old xw as a whole
    hit = np.flatnonzero(idx == f)
    at_new = -1
    idx1 = idx
    if hit.size:
        j = int(hit[0])
        nv = w1[j] + beta
        w1.v[j], w1.e[j] = max(nv.v, 0), nv.e
        own[j] += U * np.abs(nv.v)
        common = common + beta.e * np.abs(xf)
    elif beta.v > 0:
        at_new = idx.shape[0]
        idx1 = np.append(idx, np.int64(f))
        w1 = E(np.append(w1.v, beta.v), np.append(w1.e, beta.e))       # (0. + beta is exact)
        own = np.append(own, 0)
        common = common + beta.e * np.abs(xf)
        cols = P[idx1]
    out.update(idx1=idx1, w1=w1, at_new=at_new, post=list_state(b, w1, cols, (common, own)))
    out['nxt'] = next_vectors(alg, b, bn, out['post'])
    return out


def scores(alg, phi, b, idx, val):
    """the sweep's exact-formula score of every row for the list state (idx, val), in np.longdouble; -inf where GIGA masks"""
    P = np.asarray(phi, dtype=LD)
    b = np.asarray(b, dtype=LD)
    bn = E.of(b) / esqrt(edot(b, b))
    st = list_state(b, E(np.asarray(val, dtype=LD)), P[np.asarray(idx, dtype=np.int64)])
    nv = next_vectors(alg, b, bn, st)
    nr = np.sqrt((P * P).sum(axis=1))
    if alg == 'fw':
        return P.dot(nv['v0'].v) / nr
    s0, s1 = P.dot(nv['v0'].v) / nr, P.dot(nv['v1'].v) / nr
    good = np.logical_and(s1 > -1. + 1e-14, 1 - s1 * s1 > 0)
    return np.where(good, s0 / np.sqrt(np.where(good, 1 - s1 * s1, 1)), -np.inf)


def margin(sc, f):
    """(score of f) - (the best other score)"""
    rest = np.delete(sc, f)
    return float(sc[f] - rest.max()) if rest.size else float('inf')


def ratio(got, ref):
    """max |got - ref.v| / bound over the entries (0 / 0 counts as 0: an exact zero stays exact); inf for a NaN"""
    got = np.atleast_1d(np.asarray(got, dtype=np.float64))
    if np.isnan(got).any():
        return float('inf')
    d = np.abs(got.astype(LD) - np.atleast_1d(ref.v))
    bd = np.atleast_1d(ref.bound())
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(d == 0, 0, d / bd)
    return float(r.max()) if r.size else 0.


# ------------------------------------------------------------------ planted states
def _seed(S, nnz, alg, kind):
    return (7919 * S + 104729 * nnz + 31 * ALGS.index(alg) + 1000003 * KINDS.index(kind)) % (2 ** 31)


def _fw_scale(phi, idx, val):
    nrm = np.sqrt((phi ** 2).sum(axis=1))
    t = (val * nrm[idx]).sum()
    return val * (nrm.sum() / t) if t > 0 else val


def _unit(x):
    return x / np.sqrt((x ** 2).sum())


@functools.lru_cache(maxsize=4)
def planted(S, nnz, alg, kind):
    """dict(phi [n x S], b, idx, val, f, S, nnz, alg, kind): module docstring.  Read-only arrays."""
    assert S >= (3 if alg == 'giga' else 2) and kind in KINDS
    assert nnz > 0 or kind == 'fresh'
    rng = np.random.RandomState(_seed(S, nnz, alg, kind))
    n = nnz + EXTRA_ROWS
    r = min(12, S)
    phi = rng.randn(n, r).dot(rng.randn(r, S)) + 0.3 * rng.randn(n, S) + 2.0 * rng.randn(S)[None, :]
    perm = rng.permutation(n)
    idx = perm[:nnz].astype(np.int64)
    val = rng.uniform(0.5, 1.5, size=nnz) * (float(n) / max(nnz, 1))
    G = groups(S)
    if kind == 'zeros':
        val[rng.permutation(nnz)[:max(1, nnz // 4)]] = 0.
    if kind == 'all_zero':
        val[:] = 0.
    if kind == 'revisit_head':
        slot = min(nnz - 1, PF_NC * G - 1, 3 + G // 2)
    elif kind == 'revisit_behind':
        slot = nnz - 2
        assert slot >= PF_NC * G, 'no list slot behind the up-front loads at this length'
    f = int(idx[slot]) if kind.startswith('revisit') else int(perm[nnz + 17])
    scale = np.sqrt((phi ** 2).sum(axis=1)).mean()
    e = _unit(rng.randn(S))
    a = phi.dot(e)
    perp = phi - a[:, None] * e[None, :]                   # (what a row keeps whatever happens to its component along e)
    live = np.zeros(n, dtype=bool)                         # listed with a positive weight: these rows make xw
    live[idx[val > 0]] = True
    w_of = np.zeros(n)
    w_of[idx] = val
    g = rng.randn(S)
    g -= g.dot(e) * e
    x = None
    if alg == 'giga' and live.any():
        # xw / |xw|, given sum_j w_j a_j = 0 below.  A listed winner's part along g is taken out of another listed row, so
        # that the direction is the other rows' own
        rest = live.copy()
        rest[f] = False
        x = _unit((w_of[:, None] * perp)[rest].sum(axis=0))
        g -= g.dot(x) * x
    g = _unit(g)
    win = scale * (e + 0.3 * g + (0.5 * x if x is not None else 0.))
    if x is not None and live[f]:
        k = int(idx[[j for j in range(nnz) if val[j] > 0 and idx[j] != f][0]])
        perp[k] -= (w_of[f] / w_of[k]) * scale * 0.3 * g
    perp[f] = win - win.dot(e) * e
    orth = perp if x is None else perp - perp.dot(x)[:, None] * x[None, :]
    a = np.minimum(a, CUT * np.sqrt((orth ** 2).sum(axis=1)))
    a[f] = win.dot(e)
    if x is not None:
        free = live.copy()
        free[f] = False
        fixed = w_of[f] * a[f] if live[f] else 0.
        pos = (w_of * a)[free & (a > 0)].sum() + fixed
        neg = -(w_of * a)[free & (a < 0)].sum()
        if neg > 0:
            a[free & (a < 0)] *= pos / neg
        else:
            assert fixed == 0., 'no listed row to balance the winner with'
            a[free & (a > 0)] = 0.
    phi = perp + a[:, None] * e[None, :]
    if alg == 'fw':
        val = _fw_scale(phi, idx, val)
    xw = (val[:, None] * phi[idx]).sum(axis=0) if nnz else np.zeros(S)
    nw = np.sqrt((xw ** 2).sum())
    if alg == 'fw':
        b = xw + 0.05 * max(nw, scale * n) * e
    elif nw == 0.:
        b = scale * n * e
    else:
        b = nw * (np.cos(0.3) * xw / nw + np.sin(0.3) * _unit(e - e.dot(xw / nw) * xw / nw))
    for arr in (phi, b, idx, val):
        arr.setflags(write=False)
    return dict(phi=phi, b=b, idx=idx, val=val, f=f, S=S, nnz=nnz, alg=alg, kind=kind)


def colinear(S, nnz, alg):
    """the design of test_finish_kernels_agree_on_failure_branches (every row a positive multiple of one vector) with a planted
    list of nnz rows: GIGA's _select raises at once, FrankWolfe's line search is decided by rounding"""
    rng = np.random.RandomState(3 + S + nnz)
    n = nnz + 40
    phi = np.abs(rng.randn(n, 1)) * rng.randn(1, S)
    idx = rng.permutation(n)[:nnz].astype(np.int64)
    val = rng.uniform(0.5, 1.5, size=nnz) * (float(n) / nnz)
    if alg == 'fw':
        val = _fw_scale(phi, idx, val)
    return dict(phi=phi, b=phi.sum(axis=0), idx=idx, val=val, S=S, nnz=nnz, alg=alg, kind='colinear')


# ------------------------------------------------------------------ the loops of dev_xw_err_t, restated from the kernel text
def xw_walk(S, nnz, pf):
    """{loop: [(group, list entry)]} for a list of nnz entries: 'c16' (PF only: the slots of the up-front loads), 'x16', 'x4',
    'tail', or 'serial' alone where S > 512 (every thread walks the whole list)"""
    out = dict(c16=[], x16=[], x4=[], tail=[], serial=[])
    if S > FIN_THREADS:
        out['serial'] = [(0, j) for j in range(nnz)]
        return out
    G = FIN_THREADS // S
    for g in range(G):
        j = g
        if pf:
            for u in range(PF_NC):
                if j < nnz:
                    out['c16'].append((g, j))
                    j += G
        while j + 15 * G < nnz:
            out['x16'] += [(g, j + u * G) for u in range(16)]
            j += 16 * G
        while j + 3 * G < nnz:
            out['x4'] += [(g, j + u * G) for u in range(4)]
            j += 4 * G
        while j < nnz:
            out['tail'].append((g, j))
            j += G
    return out


def loop_of(S, nnz, pf, entry):
    for name, lst in xw_walk(S, nnz, pf).items():
        if any(j == entry for _, j in lst):
            return name
    return None


def xw_model(S, w, cols, G=None, drop=None):
    """xw as a block of FIN_THREADS threads in groups of S builds it: group g = thread // S walks the entries g, g + G, ...;
    a thread beyond the block does not exist.  G = None: the kernel's 512 / S.  (A mutant G = ceil(512 / S) leaves the last
    group short of threads.)  drop: a list entry left out."""
    nnz = cols.shape[0]
    if S > FIN_THREADS:
        keep = np.arange(nnz) != (-1 if drop is None else drop)
        return (w[keep, None] * cols[keep]).sum(axis=0)
    G = FIN_THREADS // S if G is None else G
    xw = np.zeros(S, dtype=cols.dtype)
    for g in range(G):
        js = np.arange(g, nnz, G)
        js = js[js != (-1 if drop is None else drop)]
        live = max(0, min(S, FIN_THREADS - g * S))
        xw[:live] += (w[js, None] * cols[js, :live]).sum(axis=0)
    return xw


def form_of(S, nnz0, label, redo=False):
    """the finish kernel that serves a step from a list of nnz0 entries in the form `label` names.  redo: the pre-filter's
    candidate lists overflowed in this step (its counter says so) and the step was redone through the exact sweep, whose
    record a kernel without the rescoring reads"""
    if S > FIN_THREADS or 'NOPF' in label or nnz0 + 1 > PF_MAXNNZ:
        return PLAIN
    if 'BC_PREFILTER=0' in label or 'NOFUSE' in label or redo:
        return ONE_ROUND
    return ONE_ROUND_BB if 'BC_I8_BB' in label else ONE_ROUND_RESCORE


# ------------------------------------------------------------------ case lists
S_ONE_ROUND = (3, 7, 63, 64, 65, 100, 170, 171, 256, 257, 511, 512)
S_PLAIN = (513, 1024, 1025)
S_FW_ONLY = (2,)
S_FULL = (7, 65, 100, 171, 257, 512, 513)      # every list length; the other S keep the edges (edge_lengths)
HANDOVER = (1022, 1023, 1024, 1025)


def all_lengths(S):
    G = groups(S)
    return sorted(set((0, 1, G - 1, G, G + 1, 16 * G - 1, 16 * G, 16 * G + 1, 20 * G - 1, 20 * G, 32 * G - 1, 32 * G, 32 * G + 1,
                       36 * G + 3) + HANDOVER))


def edge_lengths(S):
    """kept at every S: an empty list, the last entry served from xf and the first read back from cols (16 G), every loop
    non-empty (36 G + 3), and both sides of the hand-over to the plain kernel"""
    G = groups(S)
    return sorted(set((0, 16 * G - 1, 16 * G, 16 * G + 1, 36 * G + 3, 1023, 1024)))


def S_of(alg):
    return (S_FW_ONLY if alg == 'fw' else ()) + S_ONE_ROUND + S_PLAIN


def cases(S, alg):
    """[(nnz, kind)] at this S: 'fresh' at every length, the other kinds at 36 G + 3 (every loop non-empty, slots on both sides
    of 16 G), 'zeros' at 16 G + 1 too"""
    G = groups(S)
    out = [(L, 'fresh') for L in (all_lengths(S) if S in S_FULL else edge_lengths(S))]
    out += [(36 * G + 3, k) for k in KINDS[1:]] + [(16 * G + 1, 'zeros')]
    return out


def colinear_lengths(S):
    return (1, 16 * groups(S) + 1)
