"""The pre-filter's control block (beta_cores_amd/csrc/bc_pref_ctrl.h), compiled for the host by tests/pref_ctrl_harness.c: the
names keep the word positions the kernels have always used, u64 fields are 8-byte aligned, no two fields share a word, and
the block is the 64 ints that include/beta_cores_prefdiag.h documents for the "ctrl" buffer."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# field -> (word index, width in words): the layout every sweep and rescoring kernel, and tests/test_gpu_pref_counters.py, rely on
LAYOUT = {
    'BC_PCTL_OVERFLOWED': (1, 1),     # last launch overflowed
    'BC_PCTL_OVERFLOWS': (3, 1),      # overflows so far
    'BC_PCTL_SWEEPS': (4, 2),         # sweeps
    'BC_PCTL_RESCORED': (6, 2),       # rows rescored
    'BC_PCTL_RING_POS': (9, 1),       # ring position
    'BC_PCTL_L1_PASSED': (12, 2),     # rows passed on by level 1
    'BC_PCTL_SPILL_N': (14, 1),       # pairs in the spill list
    'BC_PCTL_BB_THETA': (16, 2),      # branch-and-bound shared bound
}


@pytest.fixture(scope='module')
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('pref_ctrl') / 'pref_ctrl_harness')
    cmd = ['cc', '-O2', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'beta_cores_amd', 'csrc'),
           os.path.join(ROOT, 'tests', 'pref_ctrl_harness.c'), '-o', exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    res = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout + res.stderr
    block, fields = None, {}
    for line in res.stdout.splitlines():
        w = line.split()
        if w[0] == 'block':
            block = (int(w[1]), int(w[2]))
        else:
            assert w[0] == 'field' and w[1] not in fields, line
            fields[w[1]] = (int(w[2]), int(w[3]))
    assert block is not None
    return block, fields


def test_fields_are_where_the_kernels_have_them(table):
    block, fields = table
    assert block == (256, 64)
    assert fields == LAYOUT


def test_u64_fields_are_even_aligned(table):
    _, fields = table
    wide = {n: f for n, f in fields.items() if f[1] == 2}
    assert len(wide) == 4
    assert all(idx % 2 == 0 for idx, _ in wide.values()), wide


def test_fields_are_disjoint_and_inside(table):
    (_, ints), fields = table
    words = [w for idx, width in fields.values() for w in range(idx, idx + width)]
    assert len(words) == len(set(words)), sorted(words)
    assert min(words) >= 0 and max(words) < ints


def test_int_count_is_the_documented_one(table):
    (nbytes, ints), _ = table
    with open(os.path.join(ROOT, 'include', 'beta_cores_prefdiag.h')) as f:
        m = re.findall(r'"ctrl" \((\d+) ints\)', f.read())
    assert m == [str(ints)], m
    assert nbytes == 4 * ints
