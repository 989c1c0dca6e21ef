"""The cases of K4's GPU tests (tests/gram_cases.py), on the CPU: run_gram takes its row splits from csrc/bc_gram_plan.h, the
header compiled for the host gives what the case file's restatement gives, the lists stay inside the host route's limits and
reach every class of split the kernels treat differently (a class that goes missing is named), and the derived bound is
neither loose nor wrong: NumPy's own float64 result lies inside it on every host case, four wrong Grams lie outside it."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import gram_cases as GC                                                          # noqa: E402
from oracle import models_ref as M                                               # noqa: E402

CSRC = os.path.join(ROOT, 'beta_cores_amd', 'csrc')


def header_plans(tmp_path, rows):
    """bc_gram_plan for every (n_rows, ntri, n_cu, slots, waves, kr) of `rows`, from the header compiled for the host"""
    exe = str(tmp_path / 'gram_plan_harness')
    cmd = ['gcc', '-std=c99', '-O1', '-Wall', '-Werror', '-pedantic-errors', '-I', CSRC, os.path.join(ROOT, 'tests', 'gram_plan_harness.c'),
           '-o', exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    res = subprocess.run([exe], input=''.join('%d %d %d %d %d %d\n' % r for r in rows), capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr
    got = [tuple(int(x) for x in line.split()) for line in res.stdout.splitlines()]
    assert len(got) == len(rows)
    return got


def test_run_gram_and_the_harness_share_the_header():
    src = open(os.path.join(CSRC, 'bc_gram.hip')).read()
    assert '#include "bc_gram_plan.h"' in src
    assert len(re.findall(r'\bbc_gram_plan\(data->n_rows, ntri, ctx->n_cu, slots, waves, KR, &rps, &splits, &nruns\)', src)) == 1
    # ... and no longer spells the arithmetic itself
    assert 'want_splits' not in src and 'max_splits' not in src and '2 * KR' not in src
    assert not re.search(r'#\s*define\s+BC_GRAM_SEG', src)
    assert not re.search(r'\b(rps|splits|nruns) = [^0;]', src.replace('a.splits = splits;', '')), 'bc_gram.hip computes a split quantity itself'
    hdr = open(os.path.join(CSRC, 'bc_gram_plan.h')).read()
    assert int(re.search(r'#define BC_GRAM_SEG (\d+)', hdr).group(1)) == GC.SEG
    assert int(re.search(r'#define BC_GRAM_SMALL_ROWS (\d+)', src).group(1)) == GC.SMALL_ROWS
    assert 'data->n_rows >= %d' % GC.DMA_MIN_ROWS in src


def test_restated_plan_is_what_the_header_computes(tmp_path):
    rows = []
    for n in list(range(1, 300)) + [511, 512, 513, 4095, 4096, 4097, 20000, 200_000, 262_145, 10_000_000, 2 ** 31 + 5, 2 ** 33]:
        for ntri in (1, 3, 6, 10, 153):
            for n_cu in (1, 64, 256, 304):
                for slots, kr in ((3, 32), (2, 16), (4, 16)):
                    for waves in (1, 8, 0):
                        rows.append((n, ntri, n_cu, slots, waves, kr))
    for n, d in GC.SPLIT_EDGES + GC.RESIDENT_FEW + [(n, dz - 1) for n, dz in GC.HOST_BIG]:
        for weighted in (True, False):
            r = GC.route(n, d, weighted)
            rows.append((n, r['ntri'], 256, r['slots'], r['waves'], r['kr']))
    have = header_plans(tmp_path, rows)
    wrong = [(r, h, GC.plan(*r)) for r, h in zip(rows, have) if h != GC.plan(*r)]
    assert not wrong, '(inputs, header, restatement) ' + repr(wrong[:5])


def test_lists_respect_the_host_route_limits():
    assert len(set(GC.SMALL)) == len(GC.SMALL) == 93 and len(set(GC.HOST_BIG)) == len(GC.HOST_BIG) == 10
    for n, dz in GC.SMALL + GC.HOST_BIG:
        assert dz >= 2 and n * (dz + 1) <= GC.HOST_DOUBLES and dz * dz <= GC.HOST_DOUBLES, (n, dz)
    assert all(1 <= n <= GC.SMALL_ROWS for n, _ in GC.SMALL) and all(n > GC.SMALL_ROWS for n, _ in GC.HOST_BIG)
    # k_gram_small: row counts on both sides of every 128-row trip it can take; block pairs ta < tb with x * x entries; sampler shapes
    assert {127, 128, 129, 255, 256, 257, 511, 512} <= set(n for n, _ in GC.SMALL)
    assert {17, 18, 33, 65, 101, 116, 243, 244} <= set(dz for _, dz in GC.SMALL)
    # past 512 rows: both tile sizes, and (20000, 2) sits exactly on the limit
    assert any(dz - 1 <= 64 for _, dz in GC.HOST_BIG) and any(dz - 1 > 64 for _, dz in GC.HOST_BIG)
    assert max(n * (dz + 1) for n, dz in GC.HOST_BIG) == GC.HOST_DOUBLES
    # none of the resident lists reaches the LDS-DMA kernel (it has its own cases) and every plan is limited by the rows, not by
    # the device: the same on any device with at least 128 CUs
    for n, d in GC.SPLIT_EDGES + GC.RESIDENT_FEW:
        for weighted in (True, False):
            assert not GC.route(n, d, weighted)['dma']
            assert GC.route(n, d, weighted, n_cu=128) == GC.route(n, d, weighted) == GC.route(n, d, weighted, n_cu=304), (n, d)


def test_every_class_of_split_has_a_case():
    lost = []
    for bt in (64, 128):
        rs = [(n, GC.route(n, d, True)) for n, d in GC.SPLIT_EDGES + GC.RESIDENT_FEW]
        rs = [(n, r) for n, r in rs if r['bt'] == bt]
        classes = {
            'fewer rows than a slab': lambda n, r: n < r['kr'],
            'a last split of exactly one row': lambda n, r: r['splits'] >= 2 and r['last'] == 1,
            'a last split of exactly one full slab': lambda n, r: r['splits'] >= 2 and r['last'] == r['kr'],
            'n a multiple of rows_per_split': lambda n, r: r['splits'] >= 2 and n % r['rps'] == 0,
            'more than eight runs of splits': lambda n, r: r['nruns'] > 8,
        }
        for s in GC.SPLIT_COUNTS:
            classes['%d splits' % s] = lambda n, r, s=s: r['splits'] == s
        for name, has in classes.items():
            if not any(has(n, r) for n, r in rs):
                lost.append('BT = %d: %s' % (bt, name))
    assert not lost, 'classes without a GPU case: ' + '; '.join(lost)
    # each split count comes with its n + 1, whose last split holds one row
    for bt, d in GC.SPLIT_D.items():
        for s in GC.SPLIT_COUNTS:
            full = [n for n, dd in GC.SPLIT_EDGES if dd == d and GC.route(n, d, True)['splits'] == s and n % GC.route(n, d, True)['rps'] == 0]
            assert full and (full[0] + 1, d) in GC.SPLIT_EDGES, (bt, s)
            r1 = GC.route(full[0] + 1, d, True)
            assert r1['splits'] == s + 1 and r1['last'] == 1 and r1['bt'] == bt
    # the weights do not move the plan of these shapes (no case reaches the DMA kernel)
    assert all(GC.route(n, d, True) == GC.route(n, d, False) for n, d in GC.SPLIT_EDGES + GC.RESIDENT_FEW)


def test_inputs_are_what_the_docstring_says():
    for n, dz in ((1, 2), (2, 3), (129, 18), (512, 116)):
        for kind in GC.KINDS:
            Z, w = GC.inputs(n, dz, kind)
            Z2, w2 = GC.inputs(n, dz, kind)
            assert np.array_equal(Z, Z2) and np.array_equal(w, w2) and Z.shape == (n, dz) and w.shape == (n,)
            assert (w >= 0).all() and (w < 2).all() and w[-1] > 0 and (w == 0).sum() == (n // 4 if n > 1 else 0)
            assert np.isfinite(Z).all() and np.abs(Z).min() > 0
    Z, _ = GC.inputs(512, 116, 'wide')
    assert np.abs(Z).max() / np.abs(Z).min() > 1e12


def need_longdouble():
    if not GC.LONGDOUBLE_OK:
        pytest.skip(GC.LONGDOUBLE_WHY)


MUTANTS = {
    'one positively weighted row dropped': lambda Z, w: (np.delete(Z, np.flatnonzero(w > 0)[0], axis=0), np.delete(w, np.flatnonzero(w > 0)[0])),
    'two columns swapped': lambda Z, w: (Z[:, [1, 0] + list(range(2, Z.shape[1]))], w),
    'the last row counted twice': lambda Z, w: (np.vstack((Z, Z[-1:])), np.append(w, w[-1])),
    'y taken from column D - 1': lambda Z, w: (np.hstack((Z[:, :-1], Z[:, -2:-1])), w),
}


def test_numpy_float64_lies_inside_the_bound_and_four_mutants_outside():
    """The bound is not wrong (NumPy's float64 Gram of every host case lies inside it, and uses a good part of it somewhere)
    and not loose (on the plain weighted cases with two rows or more, four wrong Grams each leave it in some element)."""
    need_longdouble()
    worst, mutated = (0., None), dict.fromkeys(MUTANTS, 0)
    for n, dz in GC.SMALL + GC.HOST_BIG:
        for kind in GC.KINDS:
            for weighted in (True, False):
                Z, w, ref = GC.case(n, dz, kind, weighted)
                G, v = M.linreg_xtwx(Z, w if weighted else np.ones(n))
                r = GC.ratio(G, v, n, ref)
                worst = max(worst, (r, (n, dz, kind, weighted)))
                assert r <= 1., (n, dz, kind, weighted, r)
                if kind != 'plain' or not weighted or n < 2:
                    continue
                for name, mutate in MUTANTS.items():
                    if name == 'two columns swapped' and dz < 3:                 # (one x column: nothing to swap it with)
                        continue
                    Gm, vm = M.linreg_xtwx(*mutate(Z, w))
                    assert GC.ratio(Gm, vm, n, ref) > 1., (name, n, dz)
                    mutated[name] += 1
    print('worst error / bound of NumPy float64: %.3f at %r' % worst)
    assert worst[0] > 0.05
    assert min(mutated.values()) >= 80, mutated


def test_ratio_sees_a_nan_where_the_reference_is_finite():
    need_longdouble()
    Z, w, ref = GC.case(129, 18, 'plain', True)
    G, v = M.linreg_xtwx(Z, w)
    assert GC.ratio(G, v, 129, ref) <= 1.
    G[3, 4] = np.nan
    assert GC.ratio(G, v, 129, ref) == float('inf')
