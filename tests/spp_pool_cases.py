"""The cases of the superpoint pooling tests: seeded and small.  A case is a dict of ``index`` (int64 ``[N]``), ``S``,
``src`` (float32 ``[R, C]`` or ``[R]``), and optionally ``point_map`` / ``R``, ``batch_offsets`` and ``i32`` (the index
tensors go to the device as int32).  Nothing here needs a device."""
import functools

import numpy as np

import spp_pool_ref as ref

F32 = np.float32
TILE = 4096  # GAPRO_SPP_SORT_TILE: the points of a workgroup of the sort
CHANNELS = (1, 3, 6, 32, 33)
LENGTHS = (0, 1, 2, 3, 7, 64, 65, 4097)


def _feats(n, c, seed):
    """Values whose float32 sums round: a wide range of magnitudes and both signs."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, c)) * 10.0 ** rng.integers(-3, 4, size=(n, c))
    return x.astype(F32)


def _case(index, S, C, seed, **kw):
    index = np.asarray(index, dtype=np.int64)
    rows = kw.get("R", len(index))
    case = dict(index=index, S=int(S), src=_feats(rows, C, seed) if C else _feats(rows, 1, seed)[:, 0])
    case.update(kw)
    return case


def three_way_segment():
    """A segment on which ascending order, descending order, a pairwise tree and ``sum * (1 / n)`` give four different
    float32 results: found by a seeded search."""
    for seed in range(1000):
        x = _feats(7, 1, 5000 + seed)
        index = np.zeros(7, dtype=np.int64)
        got = [ref.pool_forward_ref(x, index, 1, convention=c)[0].tobytes()
               for c in (None, "reversed", "tree", "reciprocal")]
        if len(set(got)) == 4:
            return x, index
    raise AssertionError("no such segment among 1000 seeds")


def shared_row_case():
    """A mapped backward in which ascending point order and segment-by-segment order differ in float32: rows read by
    points of different segments, the lower points in the higher segments; found by a seeded search."""
    for seed in range(1000):
        rng = np.random.default_rng(7000 + seed)
        N, S, R = 24, 4, 3
        index = (S - 1 - np.arange(N) * S // N).astype(np.int64)  # descending ids
        rng.shuffle(index[4:20])
        pm = rng.integers(0, R, N).astype(np.int64)
        g = _feats(S, 2, 7000 + seed)
        a = ref.pool_backward_ref(g, index, S, point_map=pm, R=R)
        b = ref.pool_backward_ref(g, index, S, point_map=pm, R=R, convention="by_segment")
        if a.tobytes() != b.tobytes():
            return dict(index=index, S=S, src=_feats(R, 2, seed), point_map=pm, R=R, g=g)
    raise AssertionError("no such case among 1000 seeds")


@functools.lru_cache(maxsize=None)
def pool_cases():
    rng = np.random.default_rng(2024)
    cases = {}
    # sizes at the wave, workgroup and tile edges; the channel counts go round
    for k, n in enumerate((1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1)):
        cases["n%d" % n] = _case(rng.integers(0, 7, n), 7, CHANNELS[k % 5], 100 + n, i32=bool(k & 1))
    cases["one_segment"] = _case(np.zeros(300), 1, 3, 1)
    cases["all_distinct"] = _case(rng.permutation(300), 300, 6, 2)
    cases["descending_ids"] = _case(np.arange(299, -1, -1) // 3, 100, 33, 3)
    cases["flat_1d"] = _case(rng.integers(0, 9, 200), 9, 0, 4)
    cases["second_byte"] = _case(rng.choice([3, 259, 515], 700), 516, 3, 5)  # equal low bytes: stability between passes
    cases["third_pass"] = _case(rng.choice([3, 65536, 65537, 70000, 131075], 600), 131076, 1, 6)
    cases["empty_segments"] = _case(rng.choice([0, 2, 5], 150), 9, 32, 7)  # empty in the middle and at the end
    lengths = np.repeat(np.arange(len(LENGTHS)), LENGTHS)
    cases["segment_lengths"] = _case(rng.permutation(lengths), len(LENGTHS), 6, 8)
    long_ids = np.concatenate([np.full(70000, 1), rng.integers(0, 4, 500)])
    cases["segment_70000"] = _case(rng.permutation(long_ids), 4, 3, 9)
    x, index = three_way_segment()
    cases["three_way"] = dict(index=index, S=1, src=x)
    cases["negative_zero"] = dict(index=np.array([0, 1, 1, 3], dtype=np.int64), S=4,
                                  src=np.array([-0.0, -0.0, -0.0, 1.0], dtype=F32))
    # max: ties at the first and the last point, +0 against -0 both ways, NaN first / in the middle / alone, an empty one
    nan = np.nan
    vals = [(0, 5.0), (0, 1.0), (0, 5.0), (1, 1.0), (1, 2.0), (1, 2.0), (2, 0.0), (2, -0.0), (3, -0.0), (3, 0.0),
            (4, nan), (4, 7.0), (5, 1.0), (5, nan), (5, 0.5), (6, nan), (8, -3.0)]
    cases["max_edges"] = dict(index=np.array([v[0] for v in vals], dtype=np.int64), S=9,
                              src=np.array([[v[1], -v[1] if v[1] == v[1] else nan] for v in vals], dtype=F32))
    # point maps
    n = 500
    ids = rng.integers(0, 11, n)
    cases["map_identity"] = _case(ids, 11, 3, 20, point_map=np.arange(n, dtype=np.int64), R=n)
    cases["map_repeats"] = _case(ids, 11, 32, 21, point_map=np.sort(rng.integers(0, 120, n)).astype(np.int64), R=120,
                                 i32=True)
    cases["map_unread_rows"] = _case(ids, 11, 6, 22, point_map=(rng.integers(0, 60, n) * 2).astype(np.int64), R=130)
    cases["map_shared_rows"] = _case(ids, 11, 33, 23, point_map=rng.integers(0, 40, n).astype(np.int64), R=40)
    cases["map_tile"] = _case(rng.integers(0, 300, TILE + 37), 300, 1, 24,
                              point_map=rng.integers(0, 70000, TILE + 37).astype(np.int64), R=70000)
    shared = shared_row_case()
    cases["map_order"] = {k: v for k, v in shared.items() if k != "g"}
    # batches: ids are not shared between samples; an empty sample; one sample
    ids = np.concatenate([rng.integers(0, 5, 90), rng.integers(5, 6, 40), rng.integers(8, 13, 70)])
    cases["batch_empty_sample"] = _case(ids, 14, 3, 30, batch_offsets=np.array([0, 90, 90, 130, 200], dtype=np.int64))
    cases["batch_one_sample"] = _case(rng.integers(0, 6, 77), 6, 6, 31, batch_offsets=np.array([0, 77], dtype=np.int64),
                                      i32=True)
    return cases


POOL_NAMES = tuple(pool_cases())


@functools.lru_cache(maxsize=None)
def bad_cases():
    rng = np.random.default_rng(77)
    ids = rng.integers(0, 6, 140)
    cases = {}
    for name, where, value in (("index_minus_one", 17, -1), ("index_at_n_spps", 101, 6)):
        bad = ids.copy()
        bad[where] = value
        cases[name] = _case(bad, 6, 3, 40)
    pm = rng.integers(0, 50, 140).astype(np.int64)
    pm[66] = 50
    cases["map_at_n_rows"] = _case(ids, 6, 6, 41, point_map=pm, R=50)
    return cases


BAD_NAMES = tuple(bad_cases())


def upstream(case, seed=99):
    """The upstream gradient of a case's pooled output."""
    src = case["src"]
    return _feats(case["S"], src.shape[1], seed) if src.ndim == 2 else _feats(case["S"], 1, seed)[:, 0]
