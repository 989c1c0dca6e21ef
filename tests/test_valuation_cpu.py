"""valuation.tmc_shapley without a GPU: stand-in HMC engine and scorer, against a plain-loop restatement of
group_selection.py:145-164 written here -- the draw order, the group cap, v[0] = 0.5, zero occurrences giving 0, the refusals, and
batching that changes no value."""
import numpy as np
import pytest

from beta_cores_amd import samplers, valuation


class ToyEngine:
    """logistic_hmc's engine protocol on a toy 'posterior': every chain sits at the mean of the problem's rows (shrunk by the row
    count) plus a tenth of the iteration's normals, and accepts where log_u < -0.5.  Deterministic in (rows, draws): enough to tell
    one problem, and one draw, from another."""

    def __init__(self, Z, wts):
        self.centre = np.asarray(Z).sum(axis=0) / (1. + Z.shape[0])

    def begin(self, start, inv_mass, n_leapfrog, n_iter):
        self.th = start.copy()

    def auto_chunk(self, c, d):
        return 5

    def chunk(self, normals, log_u, step):
        s = self.centre + 0.1 * normals + 0.01 * step
        return s, s.sum(axis=2), (log_u < -0.5).astype(np.int32)

    def end(self):
        return None


class ToyHeld:
    def __init__(self, Xt, Yt):
        self.Xt, self.Yt, self.shape = Xt, Yt, Xt.shape

    def accuracy(self, correct):
        correct = np.asarray(correct)
        return float(correct.sum()) / (correct.size * self.shape[0])


def numpy_scorer(held, thetas):
    s = (held.Yt[:, None] * held.Xt).dot(np.asarray(thetas).T)
    y = held.Yt[:, None]
    cor = (((y > 0) & (s >= 0)) | ((y < 0) & (s > 0))).sum(axis=0)
    return cor, -np.logaddexp(0., -s).sum(axis=0)


def make(seed=3, G=6, d=3):
    rng = np.random.RandomState(seed)
    sizes = [3, 8, 5, 4, 7, 6][:G]
    N = sum(sizes)
    X = np.hstack((rng.randn(N, d - 1), np.ones((N, 1))))
    Y = np.where(X[:, 0] + 0.3 * rng.randn(N) > 0, 1., -1.)
    bounds = np.concatenate(([0], np.cumsum(sizes)))
    order = rng.permutation(N)
    groups = [order[bounds[g]:bounds[g + 1]].tolist() for g in range(G)]
    Xt = np.hstack((rng.randn(40, d - 1), np.ones((40, 1))))
    Yt = np.where(Xt[:, 0] > 0, 1., -1.)
    return Y[:, None] * X, groups, ToyHeld(Xt, Yt)


KW = dict(n_samples=7, n_chains=2, warmup=4, adapt_every=2, step_size=0.2)


def restated(Z, groups, held, n_perms, max_groups, cap, seed):
    """group_selection.py:145-164 as a plain loop, one problem at a time, on the documented draw order."""
    rng = np.random.RandomState(seed)
    hseed = rng.randint(2 ** 31 - 1)
    G = len(groups)
    phi, occ = np.zeros(G), np.zeros(G)
    values, perms = [], []
    for _ in range(n_perms):
        idcs = rng.permutation(G)
        v = [0.5]
        for j in range(max_groups):
            rows = []
            for idx in idcs[:j + 1]:
                g = np.asarray(groups[idx])
                rows.append(g if cap is None or len(g) < cap else rng.choice(g, cap, replace=False))
            r = samplers.logistic_hmc_many([(Z[np.concatenate(rows)], None)], rng=np.random.RandomState(hseed), start=np.zeros((2, Z.shape[1])),
                                           engine=ToyEngine, **KW)[0]
            cor, _ = numpy_scorer(held, r.pooled())
            v.append(cor.sum() / (cor.size * held.shape[0]))
            phi[idcs[j]] += v[j + 1] - v[j]
            occ[idcs[j]] += 1
        values.append(v)
        perms.append(idcs)
    return np.divide(phi, occ, out=np.zeros_like(phi), where=occ != 0), occ, np.array(values), np.array(perms)


@pytest.mark.parametrize('cap', [None, 5])
def test_against_the_plain_loop(cap):
    Z, groups, held = make()
    got = valuation.tmc_shapley(Z, groups, held, 5, 3, group_cap=cap, rng=np.random.RandomState(11), engine=ToyEngine, scorer=numpy_scorer, **KW)
    phi, occ, values, perms = restated(Z, groups, held, 5, 3, cap, 11)
    assert np.array_equal(got.perms, perms) and np.array_equal(got.occurrences, occ)
    assert np.array_equal(got.values, values) and np.array_equal(got.phi, phi)
    assert np.all(got.values[:, 0] == 0.5) and got.values.shape == (5, 4) and got.n_fallback == 0
    assert len(np.unique(got.values[:, 1:])) > 5                      # the toy problems are told apart


def test_the_cap_is_redrawn_for_every_prefix():
    """With a cap the same group contributes different rows to different prefixes: the values differ from the uncapped ones, and a
    cap above every group size draws nothing (the stream, and so every value, is the uncapped one's)."""
    Z, groups, held = make()
    run = lambda cap: valuation.tmc_shapley(Z, groups, held, 4, 3, group_cap=cap, rng=np.random.RandomState(5), engine=ToyEngine,
                                            scorer=numpy_scorer, **KW)
    free, capped, loose = run(None), run(4), run(9)
    assert np.array_equal(free.values, loose.values) and np.array_equal(free.perms, loose.perms)
    assert not np.array_equal(free.values, capped.values)


def test_zero_occurrences_give_zero():
    Z, groups, held = make()
    got = valuation.tmc_shapley(Z, groups, held, 1, 2, rng=np.random.RandomState(2), engine=ToyEngine, scorer=numpy_scorer, **KW)
    never = np.setdiff1d(np.arange(6), got.perms[0, :2])
    assert got.occurrences.sum() == 2 and np.all(got.occurrences[never] == 0) and np.all(got.phi[never] == 0.)
    assert np.all(got.occurrences[got.perms[0, :2]] == 1)


def test_batching_changes_no_value():
    Z, groups, held = make()
    run = lambda ppb: valuation.tmc_shapley(Z, groups, held, 5, 3, group_cap=5, rng=np.random.RandomState(7), perms_per_batch=ppb,
                                            engine=ToyEngine, scorer=numpy_scorer, **KW)
    one, two, all_ = run(1), run(2), run(5)
    for other in (two, all_):
        assert np.array_equal(one.values, other.values) and np.array_equal(one.phi, other.phi) and np.array_equal(one.perms, other.perms)
    assert valuation.default_perms_per_batch(groups, 3, 3) >= 1
    big = [list(range(50))] * 50
    per_perm = 8 * 9 * sum(50 * (j + 1) for j in range(20))
    assert valuation.default_perms_per_batch(big, 9, 20, 50) == (256 << 20) // per_perm


def test_refusals():
    Z, groups, held = make()
    kw = dict(rng=np.random.RandomState(1), engine=ToyEngine, scorer=numpy_scorer)
    with pytest.raises(ValueError, match='max_groups'):
        valuation.tmc_shapley(Z, groups, held, 2, 7, **kw)
    with pytest.raises(ValueError, match='max_groups'):
        valuation.tmc_shapley(Z, groups, held, 2, 0, **kw)
    with pytest.raises(ValueError, match='n_perms'):
        valuation.tmc_shapley(Z, groups, held, 0, 2, **kw)
    with pytest.raises(ValueError, match='outside Z'):
        valuation.tmc_shapley(Z, groups[:-1] + [[10 ** 6]], held, 1, 2, **kw)
    with pytest.raises(ValueError, match='set by tmc_shapley'):
        valuation.tmc_shapley(Z, groups, held, 1, 2, keep_samples=True, **kw)
