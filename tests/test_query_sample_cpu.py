"""The NumPy restatement of the query sampling (tests/query_sample_ref.py) on the cases of tests/query_sample_cases.py
against answers one can check by hand, the two deliberately wrong variants on the cases that target them, and
gapro_fps_plan.  No GPU: tests/test_query_sample_gpu.py compares the device with the restatement bit for bit.
"""
import numpy as np
import pytest

import query_sample_cases as cases
import query_sample_ref as ref

from gapro_amd import consumer_ops as ops

_, XYZ_CAPACITY, CAPACITY = ops.fps_plan(0)
FPS = cases.fps_cases(XYZ_CAPACITY, CAPACITY)
BALL = cases.ball_cases()
SMALL = sorted(k for k, c in FPS.items() if c["form"] == "fps" and len(c["xyz"]) <= 6000)


def _fps(c, **kw):
    return ref.fps_ref(c["xyz"], c["offset"], c["new_offset"], **kw)


def test_plan_is_monotone_and_its_paths_meet_at_the_capacities():
    assert 1024 <= XYZ_CAPACITY < CAPACITY
    order = ("resident", "streamed", "global")
    last = 0
    for n in (0, 1, 1024, XYZ_CAPACITY - 1, XYZ_CAPACITY, XYZ_CAPACITY + 1, CAPACITY - 1, CAPACITY, CAPACITY + 1,
              10 * CAPACITY, 2 ** 31 - 1):
        path, a, b = ops.fps_plan(n)
        assert (a, b) == (XYZ_CAPACITY, CAPACITY)
        assert order.index(path) >= last
        last = order.index(path)
    assert ops.fps_plan(XYZ_CAPACITY)[0] == "resident" and ops.fps_plan(XYZ_CAPACITY + 1)[0] == "streamed"
    assert ops.fps_plan(CAPACITY)[0] == "streamed" and ops.fps_plan(CAPACITY + 1)[0] == "global"
    with pytest.raises(ValueError):
        ops.fps_plan(-1)
    with pytest.raises(ValueError):
        ops.fps_plan(2 ** 31)


@pytest.mark.parametrize("name", [k for k in SMALL if k.startswith("size_")])
def test_a_sample_is_visited_once_and_then_its_first_point_repeats(name):
    c = FPS[name]
    idx, _, flags = _fps(c)
    assert flags == 0
    n = int(c["offset"][0])
    lo, m_lo = 0, 0
    for b in range(4):  # m = 1, 2, n, n + 3
        hi, m_hi = int(c["offset"][b]), int(c["new_offset"][b])
        got = idx[m_lo:m_hi]
        assert got[0] == lo and ((got >= lo) & (got < hi)).all()
        assert len(set(got[:n].tolist())) == min(n, len(got))  # distinct random points: no index twice
        assert (got[n:] == lo).all()                           # every minimum is 0: the first point wins
        lo, m_lo = hi, m_hi


def test_lattice_corners_and_the_tie_rule():
    c = FPS["lattice"]
    idx, minima, _ = _fps(c)
    assert idx[0] == 0 and idx[1] == 215  # the origin, then the opposite corner: the only point at distance^2 4.6875
    d = np.minimum(((c["xyz"] - c["xyz"][0]) ** 2).sum(1), ((c["xyz"] - c["xyz"][215]) ** 2).sum(1))
    tied = np.nonzero(d == d.max())[0]
    assert len(tied) > 1 and idx[2] == tied.min()  # several points tie for the third place: the lowest index
    for block in (8, 64, 256):  # the reference's order depends on its block size, and is another one
        other = _fps(c, pick=ref.tournament(block))[0]
        assert (other[:2] == idx[:2]).all() and other[2] != idx[2] and other[2] in tied, block
    # the arithmetic is exact on the lattice: contraction cannot matter
    fused = _fps(c, dist=ref.sqdist_fused)
    assert (fused[0] == idx).all() and fused[1].tobytes() == minima.tobytes()
    shuffled = _fps(FPS["lattice_shuffled"])[0]
    for block in (8, 64, 256):  # in another order of the points the two rules part as well (not always at the third)
        assert (_fps(FPS["lattice_shuffled"], pick=ref.tournament(block))[0] != shuffled).any(), block


def test_without_ties_the_tournament_is_the_restatement():
    c = FPS["random_5000"]
    idx, minima, _ = _fps(c)
    assert len(np.unique(idx)) == len(idx)
    for block in (8, 64, 512):
        other = _fps(c, pick=ref.tournament(block))
        assert (other[0] == idx).all() and other[1].tobytes() == minima.tobytes(), block


def test_a_fused_distance_changes_the_bits_of_the_minima():
    c = FPS["random_5000"]
    _, minima, _ = _fps(c)
    _, fused, _ = _fps(c, dist=ref.sqdist_fused)
    differ = np.mean(minima.view(np.uint32) != fused.view(np.uint32))
    print("minima whose bits differ between unfused and fused evaluation: %.1f %%" % (100 * differ))
    assert 0.05 < differ < 0.5  # about a fifth
    assert np.abs(minima - fused).max() <= 4e-7  # and by a last bit of numbers below 1


def test_batches_follow_one_offset_rule():
    plain, lead, wide = (_fps(FPS[k]) for k in ("batch3", "batch3_leading_zero", "batch3_int64"))
    assert (plain[0] == lead[0]).all() and (plain[0] == wide[0]).all() and plain[1].tobytes() == lead[1].tobytes()
    assert plain[0][0] == 0 and plain[0][10] == 100 and plain[0][22] == 230  # each sample starts at its first point
    c = FPS["batch3"]
    for b, (lo, hi) in enumerate(((0, 100), (100, 230), (230, 300))):  # a sample alone gives the same indices
        m0, m1 = (int(c["new_offset"][b - 1]) if b else 0), int(c["new_offset"][b])
        alone = ref.fps_ref(c["xyz"][lo:hi], [hi - lo], [m1 - m0])[0]
        assert (alone + lo == plain[0][m0:m1]).all()
    idx, _, flags = _fps(FPS["empty_middle"])
    assert flags == 0 and len(idx) == 19 and idx[10] == 100
    idx, _, flags = _fps(FPS["no_points"])
    assert flags == ref.FLAG_EMPTY and (idx[10:13] == -1).all() and idx[13] == 100
    assert ref.status_of(flags) == ref.ERR_BAD_ARG
    for name in ("nan_coordinate", "inf_first_point"):
        idx, _, flags = _fps(FPS[name])
        assert flags == ref.FLAG_NOT_FINITE and ref.status_of(flags) == ref.ERR_NOT_FINITE
        assert (idx[:10] < 100).all() and ((idx[10:22] >= 100) & (idx[10:22] < 230)).all() and (idx[22:] >= 230).all()
    for name in ("offsets_decrease", "offsets_beyond"):
        assert _fps(FPS[name])[2] == ref.FLAG_OFFSETS


def test_near_origin_skip():
    c = FPS["skip_origin"]
    B, N, _ = c["xyz"].shape
    off, new = np.arange(1, B + 1) * N, np.arange(1, B + 1) * c["npoint"]
    idx, minima, flags = ref.fps_ref(c["xyz"], off, new, skip_origin=True, local_index=True)
    assert flags == 0
    a = idx[:c["npoint"]]
    assert a[0] == 0 and not set(a[1:].tolist()) & {0, 3, 7}  # inside and on the ball: never candidates
    assert 5 in ref.fps_ref(c["xyz"][0], [N], [N], skip_origin=True)[0]  # just outside: one
    assert (minima[[0, 3, 7]] == ref.FAR).all()  # and never updated
    assert (idx[c["npoint"]:] == 0).all() and (minima[N:] == ref.FAR).all()  # no candidate: index 0
    plain = ref.fps_ref(c["xyz"], off, new, local_index=True)[0]
    assert (plain != idx).any()


def test_ball_query_by_hand():
    for ns in (1, 32, 64):
        for extra in (-1, 0, 1):
            c = BALL["ns%d_hits%+d" % (ns, extra)]
            idx, counts, flags = ref.ball_ref(c["radius"], ns, c["xyz"], c["new_xyz"], c["offset"], c["new_offset"])
            hits = np.nonzero(c["xyz"][:, 0] < 1)[0]
            assert flags == 0 and counts[0] == min(ns, len(hits)) == min(ns, ns + extra)
            assert (idx[0, :counts[0]] == hits[:ns]).all()
            assert (idx[0, counts[0]:] == (hits[0] if len(hits) else 0)).all()
    c = BALL["hits_at_63_and_64"]
    idx, counts, _ = ref.ball_ref(0.5, 4, c["xyz"], c["new_xyz"], c["offset"], c["new_offset"])
    assert idx.tolist() == [[63, 64, 63, 63]] and counts.tolist() == [2]
    c = BALL["early_stop_in_first_chunk"]
    assert ref.ball_ref(0.5, 3, c["xyz"], c["new_xyz"], c["offset"], c["new_offset"])[0].tolist() == [[2, 9, 40]]
    c = BALL["radius_zero"]
    idx, counts, _ = ref.ball_ref(0.0, 8, c["xyz"], c["new_xyz"], c["offset"], c["new_offset"])
    assert not idx.any() and not counts.any()  # d2 = 0 < 0 is false: rows of zeros, index 0 of the table
    c = BALL["lattice_exactly_r"]
    idx, counts, _ = ref.ball_ref(0.5, 32, c["xyz"], c["new_xyz"], c["offset"], c["new_offset"])
    assert counts[62] == 27  # the centre: its 3 x 3 x 3 block; the six points at exactly 0.5 are not hits
    assert not set(idx[62].tolist()) & {12, 52, 60, 64, 72, 112}


def test_ball_query_keeps_to_the_querys_sample():
    c = BALL["no_leak"]
    idx, counts, flags = ref.ball_ref(c["radius"], c["nsample"], c["xyz"], c["new_xyz"], c["offset"], c["new_offset"])
    assert flags == 0 and counts.min() >= 1  # every query finds itself
    assert (idx[:80] < 80).all() and (idx[80:] >= 80).all()
    d = np.linalg.norm(c["xyz"][79] - c["xyz"][80])
    assert d < c["radius"]  # the boundary points would be hits of each other
    lead = BALL["no_leak_leading_zero_int64"]
    assert (ref.ball_ref(lead["radius"], lead["nsample"], lead["xyz"], lead["new_xyz"], lead["offset"],
                         lead["new_offset"])[0] == idx).all()
    c = BALL["sample_of_one_point"]
    idx, counts, _ = ref.ball_ref(c["radius"], 4, c["xyz"], c["new_xyz"], c["offset"], c["new_offset"])
    assert (idx[1:] == 80).all() and counts.tolist()[1:] == [1, 1]
    c = BALL["empty_sample_of_queries"]
    idx, counts, flags = ref.ball_ref(c["radius"], 4, c["xyz"], c["new_xyz"], c["offset"], c["new_offset"])
    assert flags == 0 and counts.tolist() == [4, 4, 0, 0, 4, 4] and not idx[2:4].any() and (idx[4:] >= 80).all()
    for name in ("offsets_decrease", "queries_beyond_the_offsets"):
        c = BALL[name]
        assert ref.ball_ref(c["radius"], 4, c["xyz"], c["new_xyz"], c["offset"], c["new_offset"])[2] == ref.FLAG_OFFSETS
    c = BALL["batched"]
    B, N, _ = c["xyz"].shape
    M = c["new_xyz"].shape[1]
    idx = ref.ball_ref(c["radius"], c["nsample"], c["xyz"], c["new_xyz"], np.arange(1, B + 1) * N,
                       np.arange(1, B + 1) * M, local_index=True)[0]
    assert idx.max() < N and idx.reshape(B, M, -1)[1, 0, 0] == 0  # local indices: a query finds itself at 0


def test_argument_refusals_need_no_device():
    import torch

    xyz = torch.zeros((10, 3))
    off = torch.tensor([10], dtype=torch.int32)
    with pytest.raises(ValueError, match="one of new_offset and n_sample"):
        ops.furthestsampling_batchflat(xyz, off)
    with pytest.raises(ValueError, match="xyz must be a float32"):
        ops.furthestsampling_batchflat(xyz.to(torch.float64), off, n_sample=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.furthestsampling_batchflat(xyz, off, n_sample=2)
    with pytest.raises(ValueError, match="nsample must be a positive int"):
        ops.ballquery_batchflat(0.2, 0, xyz, xyz, off, off)
    with pytest.raises(ValueError, match="radius must be a finite number"):
        ops.ball_query(float("nan"), 4, xyz.view(1, 10, 3), xyz.view(1, 10, 3))
    with pytest.raises(ValueError, match="no points"):
        ops.furthest_point_sample(torch.zeros((2, 0, 3)), 4)
    with pytest.raises(ValueError, match="batch offsets for batch_size"):
        ops.sample_queries(xyz, [0, 10], 2, 4, 0.2, 8, 8)
