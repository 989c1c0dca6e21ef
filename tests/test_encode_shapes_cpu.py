"""The launch shapes of the feature encoder, on the CPU: what tests/encode_shapes.py restates (rows per tile, LDS bytes, the grid
of the persistent kernel) is what csrc/bc_encode_tile.h computes, LONG_NETS has a network in every launch class (rows per tile,
blocks per CU) the chooser can produce, and every long-walk n makes exactly three trips.  A change of the tile chooser or of
the grid arithmetic fails here and names the class that is left without a long-walk GPU case."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import encode_shapes as ES            # noqa: E402

CUS = (64, 256, 304)
# the table of the long-walk tests: widths -> (rows per tile, blocks per CU, LDS bytes, long-walk n on 256 CUs)
TABLE = {
    (13, 20, 20): (64, 4, 20480, 163857), (32, 512): (64, 4, 18432, 163857), (13, 100, 100): (64, 2, 61440, 81937),
    (33, 130, 4, 9): (32, 3, 43008, 61457), (64, 256, 64): (16, 3, 41984, 30737), (512, 512, 512): (16, 1, 132096, 10257),
    (40, 50, 8): (64, 3, 49152, 122897), (100, 200, 30): (32, 2, 77824, 40977), (300, 200, 300): (16, 2, 64512, 20497),
    (13, 21, 30, 40, 7): (64, 4, 40960, 163857),
}


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('encode_shapes') / 'encode_shapes_harness')
    cmd = ['gcc', '-O2', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'beta_cores_amd', 'csrc'),
           os.path.join(ROOT, 'tests', 'encode_shapes_harness.c'), '-o', exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr

    def run(*args):
        res = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=60)
        assert res.returncode == 0, res.stdout + res.stderr
        return [tuple(int(x) for x in line.split()) for line in res.stdout.splitlines()]
    return run


def _networks():
    rng = np.random.RandomState(21)
    nets = list(ES.LONG_NETS) + [(1, 1), (3, 5, 7), (20, 20, 20, 20, 20), (512, 1), (1, 512), (512, 512, 512, 512, 512)]
    for _ in range(200):
        nets.append(tuple(int(w) for w in rng.randint(1, 513, size=rng.randint(2, 6))))
    return nets


def test_restatement_is_what_the_header_computes(harness):
    cases = []
    for w in _networks():
        for cu in CUS:
            for n in (1, 17, 1000, 65536, ES.long_walk_n(w, cu), 2000000):
                cases.append((cu, n, w))
    have = harness('nets', *['%d:%d:%s' % (cu, n, ','.join(map(str, w))) for cu, n, w in cases])
    assert len(have) == len(cases)
    wrong = [(c, h) for c, h in zip(cases, have)
             if h != (ES.tile_rows(c[2]), ES.lds_bytes(c[2], ES.tile_rows(c[2])), ES.blocks(c[1], c[2], c[0]))]
    assert not wrong, '(n_cu, n, widths), header: ' + repr(wrong[:5])


def test_table_of_the_long_nets():
    assert set(TABLE) == set(ES.LONG_NETS) and len(set(ES.LONG_NETS)) == len(ES.LONG_NETS)
    for w, (rows, per_cu, lds, n256) in TABLE.items():
        assert ES.launch_class(w) == (rows, per_cu) and ES.lds_bytes(w, rows) == lds and ES.long_walk_n(w, 256) == n256, w
    assert ES.panel_pitch((32, 512), 1) == 0                      # the one-layer network has no second panel
    assert ES.kpad(13) == 16 and ES.pitch(13) == 20 and ES.pitch(20) == 20 and ES.pitch(512) == 516
    assert ES.tile_rows((13, 513)) == 0 and ES.tile_rows((3,) * 6) == 0


def test_long_nets_have_a_case_in_every_launch_class(harness):
    have = set(harness('classes'))
    assert have == ES.CLASSES
    hit = set(ES.launch_class(w) for w in ES.LONG_NETS)
    lost = sorted(have - hit)
    assert not lost, 'launch classes (rows per tile, blocks per CU) without a long-walk GPU case: %r' % (lost,)
    # both sides of the 48 KB of dynamic LDS that need no attribute, and the one network that fits one block per CU only
    lds = sorted(ES.lds_bytes(w, ES.tile_rows(w)) for w in ES.LONG_NETS)
    assert 48 * 1024 in lds and lds[0] < 48 * 1024 < lds[-1] and lds[-1] > ES.LDS_BUDGET
    assert any(len(w) == 2 for w in ES.LONG_NETS) and any(len(w) == 4 for w in ES.LONG_NETS)
    # one network in which later layers of a tile overwrite the padded slots of BOTH panels (d[2] > d[0], d[3] > d[1], neither
    # d[0] nor d[1] a multiple of 4): only there can a tile inherit anything but zeros in its padding
    assert any(len(w) == 5 and w[0] % 4 and w[1] % 4 and ES.kpad(w[0]) <= w[2] and ES.kpad(w[1]) <= w[3] for w in ES.LONG_NETS)


def test_every_long_walk_makes_three_trips():
    for w in ES.LONG_NETS:
        for cu in CUS:
            n, r, b = ES.long_walk_n(w, cu), ES.tile_rows(w), cu * ES.per_cu(w)
            assert ES.blocks(n, w, cu) == b and ES.trips(n, w, cu) == 3, (w, cu)
            assert ES.trips(2 * r * b, w, cu) == 2 and ES.trips(2 * r * b + 1, w, cu) == 3
            # the 17 rows past the full tiles: one short tile of 17 rows (R = 64, 32), or a full tile and one of 1 row (R = 16)
            tail = (17 + r - 1) // r
            assert ES.ntiles(n, w) == 2 * b + b // 2 + tail and n - r * (ES.ntiles(n, w) - 1) == (17 if r > 16 else 1)
            # the short last tile is the third of its block
            assert (ES.ntiles(n, w) - 1) % b == b // 2 + tail - 1 and (ES.ntiles(n, w) - 1) // b == 2
    # the sizes the existing GPU tests use make one trip everywhere
    for w in ES.LONG_NETS:
        assert ES.trips(1000, w, 64) == 1
