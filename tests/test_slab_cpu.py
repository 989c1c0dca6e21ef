"""The slab cursor of csrc/bc_slab.h, which lays out every slab of the chunked device runs, on the CPU: tests/slab_harness.cpp
built as a program of its own with AddressSanitizer and UBSan and run directly."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def even(n):
    return (n + 1) & ~1


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('slab') / 'slab_harness')
    cmd = ['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
           os.path.join(ROOT, 'tests', 'slab_harness.cpp'), '-o', exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def run(exe, *args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stderr == '', (args, out.returncode, out.stderr[-2000:])
    return [int(v) for v in out.stdout.split()]


# zero-sized pieces, one double, odd and even sizes, a lone piece, and a last piece of two doubles that holds ints
@pytest.mark.parametrize('sizes', [(0,), (1,), (2,), (0, 0, 1), (1, 1, 1), (3, 0, 5, 2), (7, 8, 9, 1, 0, 2), (15, 3, 18, 33, 2), (1001, 0, 77, 2)])
@pytest.mark.parametrize('ints', [False, True])
def test_pieces_are_aligned_disjoint_and_fill_the_total(harness, sizes, ints):
    got = run(harness, 'pieces', *(sizes + (('ints',) if ints else ())))
    offs, o = [], 0
    for n in sizes:
        offs.append(o)
        o += even(n)
    assert got == [o] + offs


@pytest.mark.parametrize('c,d', [(1, 1), (3, 5), (64, 256)])
def test_hmc_state_layout_has_the_closed_form(harness, c, d):
    """bc_hmc's state slab, piece by piece, against 5 even(cd) + 3 even(c) + even(c (1 + d)) + even(d) + 2."""
    total, closed = run(harness, 'hmc_state', c, d)
    assert total == closed == 5 * even(c * d) + 3 * even(c) + even(c * (1 + d)) + even(d) + 2
