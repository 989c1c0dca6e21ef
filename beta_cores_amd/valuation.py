"""Data valuation of GROUPS of rows by truncated Monte-Carlo Shapley values: the `DShapley` baseline of the reference's group
selection experiment (examples/zellner_logreg/group_selection.py:145-174), whose value of a set of groups is the held-out
accuracy of the logistic posterior of their rows.

One permutation asks for `max_groups` small posteriors -- the rows of the first 1, 2, ... groups -- each sampled and reduced to
ONE number.  That is the shape of samplers.logistic_hmc_many: the posteriors of a batch of permutations are sampled in one
batched run (one thread block per problem and group of chains, rows in LDS), every kept position is scored against the held-out
rows on the device where it lies (score=held), and no sample is copied to the host (keep_samples=False).
"""
import numpy as np

from . import samplers

PACKED_BYTES = 256 << 20      # the default batch keeps its packed rows under this


class ShapleyResult:
    """What tmc_shapley returns.  phi: G values (sum of marginals / occurrences; 0 for a group that never occurred);
    occurrences: G counts; values: T x (max_groups + 1), values[t, 0] = 0.5 and values[t, j + 1] the held-out accuracy of the
    first j + 1 groups of permutation t; perms: T x G; n_fallback: how many of the T * max_groups problems did not fit one
    block's LDS and took logistic_hmc_many's 'single' route.  From tmc_shapley(summary=True) also max_rhat and min_ess, both
    T x max_groups: the worst split-R-hat and the smallest effective sample size over the coordinates of the posterior behind
    values[t, j + 1] (samplers.chain_summary has the definitions); None otherwise."""

    max_rhat = min_ess = None

    def __init__(self, phi, occurrences, values, perms, n_fallback):
        self.phi, self.occurrences, self.values, self.perms, self.n_fallback = phi, occurrences, values, perms, n_fallback


def default_perms_per_batch(groups, d, max_groups, group_cap=None):
    """The most permutations whose packed rows (an upper bound: every prefix made of the largest groups) stay under 256 MB."""
    sizes = sorted((len(g) if group_cap is None or len(g) < group_cap else group_cap for g in groups), reverse=True)[:max_groups]
    rows = sum(sum(sizes[:j + 1]) for j in range(max_groups))
    return max(1, int(PACKED_BYTES // max(1, 8 * d * rows)))


def tmc_shapley(Z, groups, held, n_perms, max_groups, group_cap=None, rng=None, n_samples=64, n_chains=16, warmup=100, start=None,
                perms_per_batch=None, engine=None, scorer=None, summary=False, summarizer=None, **hmc_kwargs):
    """Truncated Monte-Carlo Shapley values of the G groups `groups` (sequences of row indices into Z) for the held-out accuracy
    of the logistic posterior (group_selection.py:145-164 -- `update_per_t` and `dshapley` -- not the slice of tmcshapley.py:84,
    which scores the wrong prefix).

    Z: N x D host rows y * [x, 1], the intercept as a column (as logistic_hmc's docstring states); every problem has weight 1.
    held: a samplers.HeldOut of the test rows [xt, 1] and labels.
    Per permutation t:  idcs = permutation(G); v[0] = 0.5 (the prior's accuracy); for j = 0 .. max_groups - 1 the problem is the
      rows of the groups idcs[:j + 1] and v[j + 1] its held-out accuracy (compute_accuracy over all kept positions of all chains);
      phi[idcs[j]] += v[j + 1] - v[j], occ[idcs[j]] += 1.  At the end phi = sum phi / sum occ where occ != 0, else 0.
    group_cap: a group with len >= group_cap contributes choice(members, group_cap, replace=False), re-drawn for EVERY prefix
      it is part of (the reference's comprehension, :151); None = no cap.
    Draws.  The reference mixes Python's `random` and NumPy's global stream; here everything comes from the one NumPy stream
      `rng` (None = the global one), in this order: first ONE integer randint(2 ** 31 - 1), the seed of the sampler's draws; then
      per permutation t = 0 .. n_perms - 1: permutation(G), then for j = 0 .. max_groups - 1, for idx in idcs[:j + 1] in order,
      choice(groups[idx], group_cap, replace=False) where the cap applies.  Every batch samples with
      logistic_hmc_many(rng=RandomState(seed), draws='shared'): ALL problems of all batches read the same normals and
      log-uniforms, so every marginal v[j + 1] - v[j] is a difference on common random numbers and batching changes no value.
    Batching: `perms_per_batch` permutations (max_groups problems each) per logistic_hmc_many call; None keeps a batch's packed
      rows under 256 MB (default_perms_per_batch).
    start: C x D for all problems, None = zeros.  n_samples, n_chains, warmup and **hmc_kwargs (step_size, n_leapfrog, inv_mass,
      adapt_every, chunk, ctx, ...) go to logistic_hmc_many.
    summary=True: every posterior's chains are summarised on the device where they lie (logistic_hmc_many(summary=True): still
      no sample is copied) and the result carries max_rhat and min_ess; no value of phi changes with it.
    engine, scorer, summarizer: stand-ins for the HMC engine, the device scorer and the device summary, as logistic_hmc_many takes
      them (CPU tests).
    Returns a ShapleyResult."""
    Z = np.ascontiguousarray(np.asarray(Z, dtype=np.float64))
    if Z.ndim != 2:
        raise ValueError('Z must be N x D, got shape %r' % (Z.shape,))
    groups = [np.asarray(g, dtype=np.int64).ravel() for g in groups]
    G = len(groups)
    if G < 1 or any(g.size < 1 for g in groups):
        raise ValueError('needs at least one group, and every group at least one row')
    if any(g.min() < 0 or g.max() >= Z.shape[0] for g in groups):
        raise ValueError('a group names a row outside Z (%d rows)' % Z.shape[0])
    n_perms, max_groups = int(n_perms), int(max_groups)
    if n_perms < 1:
        raise ValueError('n_perms must be >= 1')
    if not 1 <= max_groups <= G:
        raise ValueError('max_groups must be 1 .. G = %d, got %d' % (G, max_groups))
    if group_cap is not None and int(group_cap) < 1:
        raise ValueError('group_cap must be >= 1 or None')
    for k in ('score', 'keep_samples', 'draws', 'rng'):
        if k in hmc_kwargs:
            raise ValueError('%s is set by tmc_shapley' % k)
    d, c = Z.shape[1], int(n_chains)
    start = np.zeros((c, d)) if start is None else start
    if perms_per_batch is None:
        perms_per_batch = default_perms_per_batch(groups, d, max_groups, group_cap)
    perms_per_batch = int(perms_per_batch)
    if perms_per_batch < 1:
        raise ValueError('perms_per_batch must be >= 1')
    rs = np.random if rng is None else rng
    seed = int(rs.randint(2 ** 31 - 1))
    phi, occ = np.zeros(G), np.zeros(G, dtype=np.int64)
    values = np.zeros((n_perms, max_groups + 1))
    values[:, 0] = 0.5
    perms = np.zeros((n_perms, G), dtype=np.int64)
    n_fallback = 0
    max_rhat, min_ess = (np.full((n_perms, max_groups), np.nan), np.full((n_perms, max_groups), np.nan)) if summary else (None, None)
    extra = dict(summary=True, summarizer=summarizer) if summary else {}
    for t0 in range(0, n_perms, perms_per_batch):
        t1 = min(n_perms, t0 + perms_per_batch)
        problems = []
        for t in range(t0, t1):
            idcs = rs.permutation(G)
            perms[t] = idcs
            for j in range(max_groups):
                rows = [groups[i] if group_cap is None or groups[i].size < group_cap else rs.choice(groups[i], int(group_cap), replace=False)
                        for i in idcs[:j + 1]]
                problems.append((Z[np.concatenate(rows)], None))
        res = samplers.logistic_hmc_many(problems, n_samples=n_samples, n_chains=c, warmup=warmup, start=start,
                                         rng=np.random.RandomState(seed), draws='shared', score=held, keep_samples=False, engine=engine,
                                         scorer=scorer, **extra, **hmc_kwargs)
        n_fallback += len(res.fallback)
        values[t0:t1, 1:] = np.array([r.accuracy for r in res]).reshape(t1 - t0, max_groups)
        if summary:
            max_rhat[t0:t1] = np.array([r.summary.worst_rhat() for r in res]).reshape(t1 - t0, max_groups)
            min_ess[t0:t1] = np.array([r.summary.least_ess() for r in res]).reshape(t1 - t0, max_groups)
    for t in range(n_perms):
        for j in range(max_groups):
            phi[perms[t, j]] += values[t, j + 1] - values[t, j]
            occ[perms[t, j]] += 1
    phi = np.divide(phi, occ, out=np.zeros_like(phi), where=occ != 0)
    out = ShapleyResult(phi, occ, values, perms, n_fallback)
    out.max_rhat, out.min_ess = max_rhat, min_ess
    return out
