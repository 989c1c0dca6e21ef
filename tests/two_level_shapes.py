"""Shapes for the GPU tests of the two-level sweep (tests/test_gpu_two_level.py); no test in here.

k_sweep_i4<MODE, U> (beta_cores_amd/csrc/bc_prefilter_i4.h) takes a different path through its code for every
(U, batches per 256-row tile, cache lines per int8 record): U is the template instance, the number of batches decides how the
two register buffers alternate along a tile and across its end, the number of lines how many chunks bc_r8_interval reads.
bc_lay_i4_batch, bc_lay_i4_sp8 and bc_lay_r8_bytes (csrc/bc_layout.h) sort S = 1 .. 256 into the 21 classes of CLASSES;
tests/test_two_level_shapes_cpu.py holds this table against the header (compiled for the host) and S_LIST against the table, so
that a change of the candidate batch sizes names the class that lost its GPU case."""

# (U, batches per tile, lines per record) -> first and last S of the class (each class is one run of consecutive S)
CLASSES = {
    (5, 1, 1): (1, 40), (5, 2, 1): (65, 80), (5, 3, 1): (113, 120), (5, 4, 2): (145, 160), (5, 5, 2): (193, 200),
    (6, 1, 1): (41, 48), (6, 2, 1): (81, 96), (6, 3, 2): (129, 144), (6, 5, 2): (225, 240),
    (7, 1, 1): (49, 56), (7, 2, 1): (105, 112), (7, 3, 2): (161, 168), (7, 4, 2): (209, 224),
    (8, 1, 1): (57, 64), (8, 2, 1): (121, 124), (8, 2, 2): (125, 128), (8, 3, 2): (169, 192), (8, 4, 2): (241, 252),
    (8, 4, 3): (253, 256),
    (13, 1, 1): (97, 104), (13, 2, 2): (201, 208),
}

# One S per class and the edges: 124 | 125 and 252 | 253 (a record grows by a line), 256 (the largest S the form takes), 65 and
# 80 (first and last S of a class whose tiles carry padding k-groups: 9 or 10 groups of 8 stored as 10).  Mostly odd S, so
# that the last k-group of 8 and the last int8 dword of 4 are partly padding as well.
S_LIST = [37, 65, 80, 115, 150, 197, 45, 90, 131, 233, 53, 107, 165, 217, 61, 124, 125, 180, 252, 253, 256, 99, 203]


def class_of(s):
    """The class of S by the table above (None: S outside 1 .. 256)."""
    for c, (lo, hi) in CLASSES.items():
        if lo <= s <= hi:
            return c
    return None


def rounds(n_rows, n_cu, waves_per_cu):
    """Tiles a wave of the int8 / two-level sweep walks: the grid arithmetic of bc_pref_create (csrc/bc_prefilter.hip), restated.
    (The grid's cap of 1024 blocks, 4096 waves, does not bind while n_cu * waves_per_cu <= 4096.)"""
    ptiles = max(1, (n_rows + 255) // 256)
    wmax = n_cu * waves_per_cu
    assert wmax <= 4096
    return (ptiles + wmax - 1) // wmax
