"""The cases of the sparse-convolution tests (tests/test_spconv_cpu.py, tests/test_spconv_gpu.py): a few hundred voxels
at most, each built for one edge of the plans or of the kernels."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

Case = namedtuple("Case", "name coords shape batch_size c_in c_out bias scale")

LAYERS = ("subm", "down", "inverse")
WAVE_TILE, WG_TILE, CIN_CHUNK, MIN_CHUNK_ROWS = 16, 64, 32, 256   # csrc/spconv.hip, GAPRO_SPCONV_*
SCAN_BLOCK = 1024                                                  # csrc/scan.h kScanBlock


def _random(seed, V, shape, B=1, samples=None):
    """V distinct rows of a B x shape grid in SHUFFLED order: row order is not coordinate order."""
    rng = np.random.default_rng(seed)
    samples = list(range(B)) if samples is None else samples
    cells = int(np.prod(shape))
    pick = rng.choice(len(samples) * cells, size=V, replace=False)
    b = np.array(samples)[pick // cells]
    z, y, x = np.unravel_index(pick % cells, shape)
    return np.stack([b, z, y, x], axis=1).astype(np.int64)


def _full(shape, B=1, lo=(0, 0, 0)):
    g = np.stack(np.meshgrid(np.arange(B), *[np.arange(lo[a], lo[a] + shape[a]) for a in range(3)], indexing="ij"), -1)
    return g.reshape(-1, 4).astype(np.int64)


def _late_first_child(seed, V, shape):
    """V distinct shuffled rows of one sample whose LAST row is alone in its coarse voxel: the first child of that
    coarse row is input row V - 1, so its number is the scan's value at the last row."""
    lone = np.array([0, 4, 4, 4], dtype=np.int64)
    cells = _full(shape)
    others = cells[((cells[:, 1:] >> 1) != (lone[1:] >> 1)).any(1)]
    pick = np.random.default_rng(seed).permutation(len(others))[:V - 1]
    return np.concatenate([others[pick], lone[None]])


def _cases():
    out = []

    def add(name, coords, shape, B=1, c_in=6, c_out=16, bias=False, scale=1.0):
        out.append(Case(name, coords, tuple(shape), B, c_in, c_out, bias, scale))

    # rows: one, and the wave (16) and workgroup (64) tile edges
    for V in (1, 15, 16, 17, 63, 64, 65):
        add("rows_%d" % V, _random(V, V, (6, 7, 5)), (6, 7, 5))
    # the smallest V that spans three chunks of the weight-gradient reduction (chunks of 256 rows at C = 16)
    add("three_chunks", _random(3, 2 * MIN_CHUNK_ROWS + 1, (10, 9, 11)), (10, 9, 11), c_in=16, c_out=16)
    # geometry
    add("isolated", np.array([[0, 2, 2, 2], [0, 5, 5, 5]], dtype=np.int64), (7, 7, 7))
    add("full_block", _full((3, 3, 3), lo=(1, 2, 1)), (6, 6, 6))
    add("faces", _full((3, 4, 5)), (3, 4, 5))   # every voxel of the grid: a probe at -1 or D must miss, not wrap
    same = _random(5, 40, (4, 5, 4))
    add("twin_samples", np.concatenate([same, same + np.array([1, 0, 0, 0])])[np.random.default_rng(6).permutation(80)],
        (4, 5, 4), B=2)
    add("empty_middle", _random(7, 70, (4, 4, 5), samples=[0, 2]), (4, 4, 5), B=3)
    add("odd_dz", _full((5, 4, 4))[np.random.default_rng(8).permutation(80)], (5, 4, 4))  # z = 4: the dropped slice
    add("odd_all", _random(9, 90, (5, 7, 3), B=2), (5, 7, 3), B=2)
    add("extent_1", _random(10, 12, (1, 4, 5)), (1, 4, 5))   # D_out = 0: the strided layer has no output row
    add("extent_1x", _random(11, 20, (4, 6, 1)), (4, 6, 1))
    # channels: 1, 6, 32, 40, just past the 32-channel chunk (33: the scalar loads; 36: the float4 loads); 1, 16, 48, 224
    add("c_1_1", _random(12, 50, (5, 5, 5)), (5, 5, 5), c_in=1, c_out=1)
    add("c_32_48", _random(13, 70, (5, 5, 5)), (5, 5, 5), c_in=32, c_out=48)
    add("c_40_224", _random(14, 40, (4, 5, 4)), (4, 5, 4), c_in=40, c_out=224)
    add("c_33_16", _random(15, 66, (5, 5, 5)), (5, 5, 5), c_in=CIN_CHUNK + 1, c_out=16)
    add("c_36_48", _random(16, 66, (5, 5, 5)), (5, 5, 5), c_in=CIN_CHUNK + 4, c_out=48)
    add("c_224_40", _random(17, 40, (4, 5, 4)), (4, 5, 4), c_in=224, c_out=40)
    # values
    add("large_values", _random(18, 80, (5, 6, 5), B=2), (5, 6, 5), B=2, scale=1e4)
    add("bias", _random(19, 80, (5, 6, 5), B=2), (5, 6, 5), B=2, bias=True)
    add("bias_odd", _random(20, 45, (5, 3, 5)), (5, 3, 5), c_in=8, c_out=24, bias=True)
    add("sorted_rows", _full((4, 4, 4), B=2), (4, 4, 4), B=2)   # row order = coordinate order, for once
    # one row past the 1024 rows of a block of the down plan's scan (csrc/scan.h): the second block starts from a carry
    # (last in the list: tensors() seeds a case by its place)
    add("rows_1025", _late_first_child(21, SCAN_BLOCK + 1, (11, 10, 11)), (11, 10, 11))
    return out


CASES = _cases()
NAMES = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}


@lru_cache(maxsize=None)
def tensors(name, layer):
    """(x, weight, bias, grad_out) of a case's layer, float32 NumPy, seeded by the names.  The inverse layer maps the
    coarse rows' C_in channels to C_out on the fine rows."""
    import spconv_ref as ref

    c = BY_NAME[name]
    rng = np.random.default_rng(1000 * NAMES.index(name) + LAYERS.index(layer))
    n_coarse = len(ref.down_tables(c.coords, c.shape)[0])
    V = len(c.coords)
    rows_in, rows_out = {"subm": (V, V), "down": (V, n_coarse), "inverse": (n_coarse, V)}[layer]
    k = 3 if layer == "subm" else 2
    x = (c.scale * rng.standard_normal((rows_in, c.c_in))).astype(np.float32)
    w = (c.scale * rng.standard_normal((c.c_out, k, k, k, c.c_in)) / np.sqrt(k ** 3 * c.c_in)).astype(np.float32)
    b = rng.standard_normal(c.c_out).astype(np.float32) if c.bias else None
    g = rng.standard_normal((rows_out, c.c_out)).astype(np.float32)
    return x, w, b, g

