"""Shapes for the long-walk GPU tests of the feature encoder (tests/test_gpu_encode.py); no test in here.

k_encode_mlp (beta_cores_amd/csrc/bc_encode.hip) is a persistent kernel: bc_data_encode launches min(ntiles, n_cu * per_cu)
blocks and block b walks the tiles b, b + blocks, ... through the same two LDS panels.  What a block meets from its second
tile on (panels that hold an earlier tile, a last tile that is partly past n) depends on the rows per tile R, on which panels
exist and on the grid, so this module restates the shape arithmetic of csrc/bc_encode_tile.h -- kpad, pitch, panel_pitch,
lds_bytes, tile_rows, per_cu, blocks -- and from it the smallest n at which blocks make a third trip.
tests/test_encode_shapes_cpu.py holds the restatement against the header (compiled for the host) and LONG_NETS against the
launch classes (R, per_cu) that occur, so that a change of the tile chooser names the class that lost its GPU case."""

MAX_LAYERS = 4
MAX_WIDTH = 512
LDS_DEVICE = 160 * 1024
LDS_BUDGET = LDS_DEVICE // 2
MAX_ROWS = 64

# One network per launch class (rows per tile R, blocks per CU), and the workloads' own.
LONG_NETS = [
    (13, 20, 20),         # R = 64, per_cu 4: the neural-linear driver's network
    (32, 512),            # R = 64, per_cu 4, one layer: the random-feature workload's network; panel 1 does not exist
    (13, 100, 100),       # R = 64, per_cu 2: 61 440 B of LDS, launched through the attribute that lifts the 48 KB limit
    (33, 130, 4, 9),      # R = 32, per_cu 3: three layers, both panels re-used inside a tile with different widths
    (64, 256, 64),        # R = 16, per_cu 3
    (512, 512, 512),      # R = 16, per_cu 1: 132 096 B of LDS
    (40, 50, 8),          # R = 64, per_cu 3: 49 152 B of LDS, the most that is launched without the attribute
    (100, 200, 30),       # R = 32, per_cu 2
    (300, 200, 300),      # R = 16, per_cu 2
    # R = 64, per_cu 4, four layers.  The one network of the list in which a tile dirties the padded slots of its own panels:
    # layer 1 writes 30 outputs over the input's slots 13 .. 15 of panel 0, layer 2 writes 40 over slots 21 .. 23 of panel 1,
    # so the zeros there are those of the NEXT tile's load stage and of its layer 0.  (In the networks above no later layer
    # reaches a padded slot: zeros written on a block's first trip would survive a missing fill on its second.)
    (13, 21, 30, 40, 7),
]

# the classes the chooser can produce for widths 1 .. 512 (held against the header by test_encode_shapes_cpu.py)
CLASSES = {(64, 4), (64, 3), (64, 2), (32, 3), (32, 2), (16, 3), (16, 2), (16, 1)}


def kpad(d):
    return (d + 3) & ~3


def pitch(d):
    k = kpad(d)
    return k if (k & 7) == 4 else k + 4


def panel_pitch(widths, p):
    """Row pitch (doubles) of panel p: the widest input d[l] of the layers l = p, p + 2, ..; 0 if there is none."""
    n_layers = len(widths) - 1
    w = max([widths[l] for l in range(p, n_layers, 2)] or [0])
    return pitch(w) if w > 0 else 0


def lds_bytes(widths, rows):
    return rows * 8 * (panel_pitch(widths, 0) + panel_pitch(widths, 1))


def tile_rows(widths):
    n_layers = len(widths) - 1
    if not 1 <= n_layers <= MAX_LAYERS or not all(1 <= w <= MAX_WIDTH for w in widths):
        return 0
    r = MAX_ROWS
    while r > 16:
        if lds_bytes(widths, r) <= LDS_BUDGET:
            return r
        r >>= 1
    return 16 if lds_bytes(widths, 16) <= LDS_DEVICE else 0


def per_cu(widths):
    return min(4, max(1, LDS_DEVICE // lds_bytes(widths, tile_rows(widths))))


def launch_class(widths):
    return tile_rows(widths), per_cu(widths)


def ntiles(n, widths):
    r = tile_rows(widths)
    return (n + r - 1) // r


def blocks(n, widths, n_cu):
    return min(ntiles(n, widths), n_cu * per_cu(widths))


def trips(n, widths, n_cu):
    """Tiles the busiest block of the launch walks."""
    b = blocks(n, widths, n_cu)
    return (ntiles(n, widths) + b - 1) // b


def long_walk_n(widths, n_cu):
    """2 B + B // 2 full tiles and 17 rows more, B = n_cu * per_cu the full grid: half of the blocks make three trips, the rest
    two, and the short last tile (17 rows; with R = 16 a full tile and one of 1 row) falls to a block that has filled its
    panels twice before."""
    r, b = tile_rows(widths), n_cu * per_cu(widths)
    return 2 * r * b + r * (b // 2) + 17
