"""The cases of the voxelisation tests (tests/test_voxelize_cpu.py, tests/test_voxelize_gpu.py): small inputs at the
sizes where the kernels take another path -- a wave (64), a workgroup (256), a scan block (1024), the rows ranked by 8
lanes / a wave / a workgroup (8 | 9, 64 | 65), the cap of GAPRO_VOXELIZE_MAX_ACTIVE -- and the conventions a wrong
implementation gets wrong.  Every case is a dict ``coords`` (int64 [N, 3 | 4]), ``mode``; the expected outcome is what
tests/voxelize_ref.py makes of it.
"""
import functools

import numpy as np

import voxelize_ref as ref

SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1025)


def _rng(seed):
    return np.random.default_rng(seed)


def _with_batch(xyz, batch):
    xyz = np.asarray(xyz, np.int64)
    return np.concatenate([np.full((len(xyz), 1), batch, np.int64), xyz], axis=1)


def _voxels_of(sizes, seed, cols=4):
    """Voxels of the given numbers of points, the points of all of them interleaved by a fixed permutation."""
    rng = _rng(seed)
    keys = np.stack([np.array([v % 3, 7 * v, -v, v * v % 11][4 - cols:], np.int64) for v in range(len(sizes))])
    rows = np.repeat(np.arange(len(sizes)), sizes)
    return keys[rng.permutation(rows)]


@functools.lru_cache(maxsize=None)  # computed once and left unchanged
def index_cases():
    c = {}
    for n in SIZES:
        # all distinct, first appearances in descending key order: sorted numbering reverses them
        c["distinct_%d" % n] = dict(coords=_with_batch(np.stack([np.arange(n, 0, -1)] * 3, axis=1), 0), mode=4)
        c["one_voxel_%d" % n] = dict(coords=np.tile(np.array([[1, -2, 3, 4]], np.int64), (n, 1)), mode=4)
    c["max_active_at_cap"] = dict(coords=_voxels_of([ref.MAX_ACTIVE, 3, 1], 1), mode=4)
    c["max_active_beyond_cap"] = dict(coords=_voxels_of([ref.MAX_ACTIVE + 1, 2], 2), mode=4)
    c["max_active_beyond_cap_mode1"] = dict(coords=_voxels_of([ref.MAX_ACTIVE + 1, 2], 2), mode=1)  # width 2: served
    c["rows_8_9"] = dict(coords=_voxels_of([8, 9, 1, 2, 7], 3), mode=4)
    c["rows_63_64_65"] = dict(coords=_voxels_of([63, 64, 65, 1, 5], 4), mode=3)
    c["rows_255_256_257"] = dict(coords=_voxels_of([255, 256, 257, 2], 5), mode=4)
    c["descending_keys"] = dict(coords=_with_batch([[9, 9, 9], [5, 5, 5], [9, 9, 9], [1, 1, 1], [5, 5, 5]], 0), mode=4)
    c["interleaved"] = dict(coords=_voxels_of([5, 4, 3, 6], 6), mode=4)
    xyz = _rng(7).integers(-3, 4, size=(300, 3))
    c["equal_xyz_other_batch"] = dict(coords=np.concatenate([_with_batch(xyz, 1), _with_batch(xyz, 0),
                                                             _with_batch(xyz[::-1], 1)]), mode=4)
    c["three_columns"] = dict(coords=_rng(8).integers(0, 5, size=(500, 3)).astype(np.int64), mode=4)
    c["three_columns_negative_first"] = dict(coords=_rng(9).integers(-4, 2, size=(200, 3)).astype(np.int64), mode=3)
    c["negative_xyz"] = dict(coords=_with_batch(_rng(10).integers(-2 ** 40, -2 ** 40 + 4, size=(400, 3)), 2), mode=4)
    high = np.array([[0, 1, 2, 3], [0, 1 + 2 ** 32, 2, 3], [0, 1, 2 + 2 ** 33, 3], [0, 1, 2, 3 - 2 ** 63],
                     [2 ** 32, 1, 2, 3], [0, 1, 2, 3 + 2 ** 62]], np.int64)
    c["above_bit_32"] = dict(coords=high[_rng(11).integers(0, len(high), size=130)], mode=4)
    bad = _with_batch(_rng(12).integers(0, 3, size=(70, 3)), 0)
    bad[66, 0] = -1
    c["negative_batch"] = dict(coords=bad, mode=4)
    dup = _voxels_of([3, 1, 2, 1, 4], 13)
    for mode in range(5):
        c["mode_%d_duplicates" % mode] = dict(coords=dup, mode=mode)  # mode 0: refused
        c["mode_%d_distinct" % mode] = dict(coords=_with_batch(_rng(14).permutation(300).reshape(100, 3), 1), mode=mode)
    c["empty_4"] = dict(coords=np.zeros((0, 4), np.int64), mode=4)
    c["empty_3"] = dict(coords=np.zeros((0, 3), np.int64), mode=1)
    c["random_1025"] = dict(coords=_with_batch(_rng(15).integers(0, 6, size=(1025, 3)), 0), mode=4)
    return c


INDEX_NAMES = sorted(index_cases())


def collision_case(slots_of, hash_of, n=1025, seed=16):
    """Many distinct keys that start their probes in the same few slots of the device table, each listed a few times:
    ``slots_of(n)`` and ``hash_of(rows)`` are the library's (gapro_voxelize_plan, gapro_voxelize_hash)."""
    rng = _rng(seed)
    pool = np.unique(_with_batch(rng.integers(-2 ** 20, 2 ** 20, size=(40000, 3)), 0), axis=0)
    start = hash_of(pool) & np.uint64(slots_of(n) - 1)
    keys = pool[start < np.uint64(8)]  # about 40000 * 8 / 4096 keys in one cluster of the table
    assert 40 <= len(keys) <= n
    return dict(coords=keys[rng.integers(0, len(keys), size=n)], mode=4)


# ---- pooling ----------------------------------------------------------------------------------------------------------
def _table(rows, width):
    t = np.zeros((len(rows), width), np.int32)
    for v, r in enumerate(rows):
        t[v, 0] = len(r)
        t[v, 1:1 + len(r)] = r
    return t


def _feats(n, C, seed):
    rng = _rng(seed)
    return (rng.standard_normal((n, C)) * np.exp(rng.uniform(-6, 6, size=(n, C)))).astype(np.float32)


def three_way_row():
    """Seven float32 values, found by search, whose mean the unfused, the fused and the sum-then-divide convention round
    to three different float32s."""
    rng = _rng(17)
    table = _table([list(range(7))], 8)
    for _ in range(2000):
        x = (rng.standard_normal((7, 1)) * np.exp(rng.uniform(-2, 2, size=(7, 1)))).astype(np.float32)
        got = {k: ref.pool_forward_ref(x, table, 4, convention=k)[0, 0] for k in ("unfused", "fused", "divide")}
        if len({v.tobytes() for v in got.values()}) == 3:
            return x, table
    raise AssertionError("no such row found")


@functools.lru_cache(maxsize=None)
def pool_cases():
    c = {}
    rng = _rng(18)
    perm = rng.permutation(200)
    rows, at = [], 0
    for n in (0, 1, 2, 3, 7, 64, 0, 5, 9, 8, 4, 65):  # the counts; zero padding follows every shorter row
        rows.append([int(p) for p in perm[at:at + n]])
        at += n
    table = _table(rows, 66)
    for C in (1, 3, 6, 9, 33):
        c["rows_C%d" % C] = dict(feats=_feats(200, C, 19 + C), map_rule=table, mode=4)
    c["mode_3"] = dict(feats=_feats(200, 3, 30), map_rule=table, mode=3)
    c["mode_1_sums_rows_as_given"] = dict(feats=_feats(200, 6, 31), map_rule=table, mode=1)
    neg = np.array([[-0.0, 1.0], [-0.0, -0.0], [2.0, -0.0]], np.float32)
    c["negative_zero"] = dict(feats=neg, map_rule=_table([[0], [1], [1, 0], [2, 1]], 4), mode=4)
    x, t = three_way_row()
    c["three_way"] = dict(feats=x, map_rule=t, mode=4)
    # many voxels: more than one workgroup and a last partial one, C no divisor of 256
    coords = _rng(32).integers(0, 9, size=(3001, 3)).astype(np.int64)
    c["many_voxels"] = dict(feats=_feats(3001, 9, 33), map_rule=ref.voxelize_idx_ref(coords, 4)[2], mode=4)
    # garbage behind the count is never read as a point
    padded = table.copy()
    padded[0, 1:] = 10 ** 9
    padded[3, 4:] = -7
    c["garbage_padding"] = dict(feats=_feats(200, 3, 34), map_rule=padded, mode=4)
    bad_count = table.copy()
    bad_count[2, 0] = 66
    bad_count[4, 0] = -1
    c["bad_counts"] = dict(feats=_feats(200, 3, 35), map_rule=bad_count, mode=4)
    bad_index = table.copy()
    bad_index[5, 3] = 200
    bad_index[11, 1] = -1
    c["bad_indices"] = dict(feats=_feats(200, 3, 36), map_rule=bad_index, mode=4)
    twice = table.copy()
    twice[8, 2] = twice[3, 1]
    c["listed_twice"] = dict(feats=_feats(200, 3, 37), map_rule=twice, mode=4)
    return c


POOL_NAMES = sorted(pool_cases())
