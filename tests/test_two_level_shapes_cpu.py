"""The shape classes of the two-level sweep, on the CPU: the table tests/two_level_shapes.py keeps (U, batches per tile, lines
per int8 record for S = 1 .. 256) is what csrc/bc_layout.h computes, and the S list of tests/test_gpu_two_level.py has a case
in every class.  A change of the candidate batch sizes (bc_lay_i4_batch) or of the record size fails here and names the class
that is left without a GPU case."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from two_level_shapes import CLASSES, S_LIST, class_of, rounds            # noqa: E402


def header_classes(tmp_path):
    exe = str(tmp_path / 'i4_classes_harness')
    cmd = ['gcc', '-O2', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'beta_cores_amd', 'csrc'),
           os.path.join(ROOT, 'tests', 'i4_classes_harness.c'), '-o', exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    res = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout + res.stderr
    rows = [tuple(int(x) for x in line.split()) for line in res.stdout.splitlines()]
    assert [r[0] for r in rows] == list(range(1, 257))
    return {s: (u, b, l) for s, u, b, l in rows}


def test_table_is_what_the_header_computes(tmp_path):
    have = header_classes(tmp_path)
    # the ranges of the table are disjoint and cover 1 .. 256 (so class_of is a function on it)
    covered = sorted(s for lo, hi in CLASSES.values() for s in range(lo, hi + 1))
    assert covered == list(range(1, 257))
    wrong = {s: (have[s], class_of(s)) for s in range(1, 257) if have[s] != class_of(s)}
    assert not wrong, 'S: (header, table) ' + repr(wrong)
    assert set(have.values()) == set(CLASSES)


def test_gpu_list_has_a_case_in_every_class(tmp_path):
    have = header_classes(tmp_path)
    assert all(1 <= s <= 256 for s in S_LIST) and len(set(S_LIST)) == len(S_LIST)
    hit = set(have[s] for s in S_LIST)
    lost = sorted(set(have.values()) - hit)
    assert not lost, 'classes (U, batches, lines) without a GPU case: %r' % (lost,)
    # the edges: a record grows by a line at 125 and 253; 256 is the largest S; 65 and 80 are the ends of a class that pads
    assert {124, 125, 252, 253, 256, 65, 80} <= set(S_LIST)
    assert have[124][2] + 1 == have[125][2] and have[252][2] + 1 == have[253][2]
    assert have[65] == have[80] and have[64] != have[65] and have[80] != have[81]


def test_rounds_arithmetic():
    # one tile per wave up to n_cu * waves * 256 rows, then two; the long-walk tests' n = 256 R n_cu - 100
    assert rounds(1, 256, 8) == 1 and rounds(524_288, 256, 8) == 1 and rounds(524_289, 256, 8) == 2
    for n_cu in (256, 304, 64):
        for r in (1, 3, 5, 7):
            assert rounds(256 * r * n_cu - 100, n_cu, 1) == r
