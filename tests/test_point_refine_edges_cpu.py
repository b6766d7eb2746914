"""The inputs of tests/test_point_refine_edges_gpu.py are what they were built to be, and their references can tell the
mistakes they are there for: no GPU is needed.  Every constant of tests/point_refine_cases.py is read back from
csrc/point_refine.hip; every case straddles the cap, gap or table edge its name speaks of and passes the library's host
checks (check_blocks restated in NumPy); every vectorised reference agrees with a per-row loop on a small instance; and
for every grid cap the reference of a kernel that did not wrap (truncated at the cap) differs from the full one."""
import os
import re

import numpy as np
import pytest

import point_refine_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _src(*path):
    with open(os.path.join(ROOT, "gapro_amd", *path)) as f:
        return f.read()


def _same(a, b):
    return all(np.array_equal(pc.bits(x), pc.bits(y)) for sa, sb in zip(a, b) for x, y in zip(sa, sb))


# ---------------------------------------------------------------------------------------------- the constants
def test_the_constants_are_the_numbers_in_the_source():
    text = _src("csrc", "point_refine.hip")

    def one(pattern, count=1):
        got = re.findall(pattern, text)
        assert len(got) == count and len(set(got)) == 1, (pattern, got)
        return got[0]

    assert int(one(r"constexpr int kThreads = (\d+);")) == pc.THREADS
    assert "256LL * per_thread" in _src("csrc", "launch_util.h")  # grid_for counts in workgroups of kThreads
    # the gather and the mu / var pass share one rule
    many, cap_many, cap_few = one(r"grid_for\(n_max, 1, n_scenes >= (\d+) \? (\d+) : (\d+)\)", 2)
    assert (int(many), int(cap_many), int(cap_few)) == (pc.MANY_SCENES, pc.GATHER_CAP_MANY, pc.GATHER_CAP_FEW)
    many, cap_many, cap_few = one(r"grid_for\(t_max, 1, n_models >= (\d+) \? (\d+) : (\d+)\)")
    assert (int(many), int(cap_many), int(cap_few)) == (pc.MANY_MODELS, pc.APPLY_CAP_MANY, pc.APPLY_CAP_FEW)
    assert int(one(r"constexpr int kMaxGridY = (\d+);")) == pc.GRID_Y
    assert "lo += kMaxGridY" in text and "d_models + lo" in text and "d_model_status + lo" in text
    assert int(one(r"grid_for\(n_rows, 1, (\d+)\)", 2)) == pc.ROW_CAP  # expand and compete
    assert int(one(r"constexpr int kVoteMaxSeg = (\d+);")) == pc.VOTE_MAX_SEG
    assert 1 << int(one(r"std::min\(n_blocks, 1 << (\d+)\)")) == pc.VOTE_GRID
    assert pc.BLOCK_DT.itemsize == 24 and pc.SEGMENT_DT.itemsize == 16 and pc.MODEL_DT.itemsize == 32


# ---------------------------------------------------------------------------------------------- gather
def _gather_cases():
    return ([pc.gather_width_case(d) for d in pc.GATHER_WIDTHS] + [pc.gather_length_case(n) for n in pc.GATHER_LENGTHS]
            + [pc.gather_big_case(), pc.gather_many_case(), pc.gather_short_case(), pc.gather_guard_case()])


def test_the_gather_cases_are_what_their_names_say():
    assert pc.GATHER_WIDTHS == (1, 6, 7, 32, 33) and pc.GATHER_LENGTHS == (1, 255, 256, 257)
    assert {n % pc.THREADS for n in pc.GATHER_LENGTHS} == {0, 1, 255}
    for c in _gather_cases():
        assert c["R"] > 0 and c["R"] < 2 ** 31
        for sc in c["scenes"]:  # what the entry point asks of a scene, and what k_refine_gather indexes with
            assert sc["n"] > 0 and sc["S"] > 0 and len(sc["inv"]) == sc["n"] and sc["feats"].shape == (sc["n"], c["d"])
            assert len(sc["sp_row"]) == sc["S"] and (sc["sp_row"] < c["R"]).all()
            if c["name"] != "guard":
                assert ((sc["inv"] >= 0) & (sc["inv"] < sc["S"])).all()
        # the blocks are disjoint and cover [0, R)
        ref = pc.gather_reference(c)
        assert (ref["scene"] >= 0).all() and (ref["canon"] != pc.SENT).all()
    for d in pc.GATHER_WIDTHS:
        c = pc.gather_width_case(d)
        assert c["d"] == d and [sc["n"] for sc in c["scenes"]] == [1000] and len(c["scenes"][0]["refined"]) == 4
    big = pc.gather_big_case()
    sc = big["scenes"][0]
    assert sc["n"] == pc.GATHER_CAP_FEW * pc.THREADS + 300 and big["d"] == 1
    assert sc["inv"][0] == 198 and sc["count"][198] == 1 and sc["inv"][-1] == 199
    assert sc["count"][7] == pc.BIG_SPP == 70000 and {198, 199, 7} <= set(sc["refined"])
    assert (np.nonzero(sc["inv"] == 199)[0] >= pc.GATHER_CAP_FEW * pc.THREADS).all()  # only wrapped workgroups see them
    run = np.nonzero(sc["inv"] == 7)[0]
    assert (np.diff(run) == 1).sum() >= pc.BIG_SPP // 2 - 1  # a run in which every lane of every wave hits one cursor
    many = pc.gather_many_case()
    assert len(many["scenes"]) == pc.MANY_SCENES == 8
    assert tuple(sc["n"] for sc in many["scenes"]) == (1, 255, 256, 257, 1000, 3, pc.GATHER_CAP_MANY * pc.THREADS + 257,
                                                       2000)
    assert len({sc["S"] for sc in many["scenes"]}) == 8
    assert [si for si, sc in enumerate(many["scenes"]) if not sc["refined"]] == [0, 5]
    long = many["scenes"][6]
    assert long["sp_row"][long["inv"][-1]] >= 0  # a refined point that only a wrapped workgroup reaches
    assert sum(sc["n"] < pc.THREADS for sc in many["scenes"]) >= 3  # workgroups that fall through the loop
    short = pc.gather_short_case()
    assert short["n_rows"] == short["R"] - 1
    last = short["scenes"][-1]
    sp = int(np.argmax(last["sp_row"]))
    assert last["sp_row"][sp] + last["count"][sp] == short["R"] and last["count"][sp] > 1
    guard = pc.gather_guard_case()["scenes"][0]
    assert (guard["inv"] == -1).sum() == 5 and (guard["inv"] == guard["S"]).sum() == 3
    assert guard["inv"].min() == -1 and guard["inv"].max() == guard["S"]  # nothing the kernel's guard does not skip


@pytest.mark.parametrize("which", ["width 7", "length 1", "length 257", "short", "guard", "many small"])
def test_the_gather_reference_agrees_with_a_loop_over_the_points(which):
    if which == "many small":  # the eight scenes without the long one's middle: the same plan code, loop-sized
        rng = np.random.default_rng(0)
        scenes = []
        for si, (n, s) in enumerate(zip((1, 255, 256, 257, 1000, 3, 700, 2000), pc.GATHER_MANY_SPPS)):
            inv = rng.integers(0, s, size=n)
            inv[0], inv[-1] = 0, s - 1
            scenes.append(pc._gather_scene(rng, n, s, 7, () if si in (0, 5) else sorted({0, s // 2, s - 1}), inv))
        c = pc._gather_case("many small", 7, scenes)
    else:
        c = {x["name"]: x for x in _gather_cases()}[which]
    for seed in (0, 1):  # two orders of the atomics: the check does not depend on it
        rp, rf, cur = pc.gather_loop(c, seed)
        n = pc.check_gather(c, rp, rf, cur)
        assert n == min(c["R"], c["n_rows"])
    # and the check can fail: a point in the wrong block, a point twice, a wrong feature bit, a row too many
    rp, rf, cur = pc.gather_loop(c, 0)
    if c["n_rows"] > 1:
        for spoil in ("swap", "twice", "bit", "extra"):
            a, b = rp.copy(), rf.copy()
            ref = pc.gather_reference(c)
            r0 = 0
            other = np.nonzero(ref["spp"][:c["n_rows"]] != ref["spp"][0])[0]
            if spoil == "swap":
                if not len(other):
                    continue
                a[[r0, other[0]]], b[[r0, other[0]]] = a[[other[0], r0]], b[[other[0], r0]]
            elif spoil == "twice":
                a[1], b[1] = a[0], b[0]
                if ref["spp"][1] != ref["spp"][0]:
                    continue
            elif spoil == "bit":
                b[0, -1] = np.nextafter(b[0, -1], np.float32(9))
            else:
                a[c["R"]] = 0
            with pytest.raises(AssertionError):
                pc.check_gather(c, a, b, cur)


def test_a_gather_that_did_not_wrap_is_told_apart():
    for c, cap in ((pc.gather_big_case(), pc.GATHER_CAP_FEW), (pc.gather_many_case(), pc.GATHER_CAP_MANY)):
        full, cut = pc.gather_reference(c), pc.gather_reference(c, limit=cap * pc.THREADS)
        assert max(sc["n"] for sc in c["scenes"]) > cap * pc.THREADS
        assert not np.array_equal(full["canon"], cut["canon"]) and (cut["canon"] == pc.SENT).any()
    # with the cap of the other branch the eight-scene call would not wrap at all
    assert max(sc["n"] for sc in pc.gather_many_case()["scenes"]) < pc.GATHER_CAP_FEW * pc.THREADS


# ---------------------------------------------------------------------------------------------- apply
def _apply_cases():
    return [pc.apply_many_case(), pc.apply_few_case(), pc.apply_grid_y_case(), pc.apply_no_rows_case(), pc.mu_var_case(),
            pc.mu_var_case(True)]


def test_the_apply_cases_are_what_their_names_say():
    for c in _apply_cases():
        for si in range(c["n_scenes"]):  # k_refine_mu_var indexes with spp_inv unguarded
            assert len(c["inv"][si]) == c["n_pts"][si] > 0 and c["spps"][si] > 0
            assert c["inv"][si].min() >= 0 and c["inv"][si].max() < c["spps"][si]
        # gapro_point_refine_apply's own model check, and rows of distinct models do not overlap
        assert ((c["t"] >= 0) & (c["off"] >= 0) & (c["off"] + c["t"] <= c["n_rows"])).all()
        assert ((c["scene_of"] >= 0) & (c["scene_of"] < c["n_scenes"])).all()
        assert (c["off"][1:] >= (c["off"] + c["t"])[:-1]).all() and c["n_rows"] < 2 ** 31
        # no two live rows share a point: the result does not depend on an order
        r = np.repeat(c["off"], c["t"]) + pc._ramp(c["t"])
        key = c["scene_of"][np.repeat(np.arange(len(c["t"])), c["t"])] * 2 ** 32 + c["row_point"][r]
        inside = (c["row_point"][r] >= 0) & (c["row_point"][r] < np.asarray(c["n_pts"])[key >> 32])
        assert len(np.unique(key[inside])) == inside.sum() and (~inside).sum() == len(c["bad_rows"])
    many = pc.apply_many_case()
    assert many["n_scenes"] == 3 and len(many["t"]) == 70 >= pc.MANY_MODELS
    assert many["t"].max() == pc.APPLY_CAP_MANY * pc.THREADS + 70
    assert set(many["t"]) == {0, 1, 255, 256, 257, many["t"].max()}
    assert (many["scene_of"] == np.arange(70) % 3).all()
    assert (many["status"] != 0).sum() == 5 and (many["t"][many["status"] != 0] > 0).sum() >= 4
    bad = many["row_point"][list(many["bad_rows"])]
    assert bad.tolist() == [-1, many["n_pts"][0], 2 ** 31 - 1] and many["scene_of"][33] == 0
    assert set(np.unique(many["lab"])) == {0, 1, 255}
    few = pc.apply_few_case()
    assert len(few["t"]) == 5 < pc.MANY_MODELS and few["t"].max() == pc.APPLY_CAP_FEW * pc.THREADS + 5
    gy = pc.apply_grid_y_case()
    assert len(gy["t"]) == pc.GRID_Y + 3 and gy["t"].min() == 1 and gy["t"].max() == 3
    assert gy["status"][pc.GRID_Y + 1] != 0 and gy["status"][2] != 0 and (gy["status"] != 0).sum() == 2
    none = pc.apply_no_rows_case()
    assert len(none["t"]) == 4 and none["t"].max() == 0
    mv = pc.mu_var_case()
    assert mv["n_pts"] == [1, pc.GATHER_CAP_FEW * pc.THREADS + 300] and len(mv["t"]) == 0
    assert tuple(pc.mu_var_case(True)["n_pts"]) == pc.GATHER_MANY_LENGTHS


def test_the_apply_reference_agrees_with_a_loop_over_the_rows():
    ts = [3, 0, 17, 1, 40, 2]
    c = pc._apply_case("small", 9, ts, [0, 1, 2, 0, 1, 2], failed=(2, 5), bad_rows=(0, 30, 31))
    assert len(c["bad_rows"]) == 3
    for use in (True, False):
        assert _same(pc.apply_reference(c, use), pc.apply_loop(c, use))
    assert not _same(pc.apply_reference(c, True), pc.apply_reference(c, False))
    c = pc.apply_no_rows_case()
    assert _same(pc.apply_reference(c), pc.apply_loop(c))


def test_an_apply_that_did_not_wrap_or_offset_is_told_apart():
    many, few, gy = pc.apply_many_case(), pc.apply_few_case(), pc.apply_grid_y_case()
    assert not _same(pc.apply_reference(many), pc.apply_reference(many, k_limit=pc.APPLY_CAP_MANY * pc.THREADS))
    assert not _same(pc.apply_reference(few), pc.apply_reference(few, k_limit=pc.APPLY_CAP_FEW * pc.THREADS))
    assert _same(pc.apply_reference(many), pc.apply_reference(many, k_limit=pc.APPLY_CAP_FEW * pc.THREADS))  # the other cap
    assert not _same(pc.apply_reference(gy), pc.apply_reference(gy, model_limit=pc.GRID_Y))
    # the status: ignoring it, and reading the second launch's status without the offset, both show
    assert not _same(pc.apply_reference(many), pc.apply_reference(many, use_status=False))
    shifted = dict(gy, status=np.r_[gy["status"][:pc.GRID_Y], gy["status"][:3]])
    assert not _same(pc.apply_reference(gy), pc.apply_reference(shifted))
    for c, cap in ((pc.mu_var_case(), pc.GATHER_CAP_FEW), (pc.mu_var_case(True), pc.GATHER_CAP_MANY)):
        assert not _same(pc.apply_reference(c), pc.apply_reference(c, point_limit=cap * pc.THREADS))
    # a failed model's rows keep the start values and the superpoint's mu / var
    out = pc.apply_reference(many)
    k = 9
    assert many["status"][k] != 0 and many["t"][k] > 0
    pts = many["row_point"][many["off"][k]:many["off"][k] + many["t"][k]]
    si = many["scene_of"][k]
    assert np.array_equal(out[si][2][pts], many["start"][si][2][pts])
    assert np.array_equal(out[si][3][pts], many["mu_spp"][si][many["inv"][si][pts]])


# ---------------------------------------------------------------------------------------------- blocks
def _block_cases():
    return [pc.compete_edge_case(), pc.compete_single_case(), pc.compete_small_case()]


def test_check_blocks_restated():
    c = pc.compete_small_case()
    ok = (c["blocks"], c["segs"], c["R"], c["R2"], 2, 8)
    assert pc.check_blocks(*ok) is None and pc.check_blocks(c["blocks"], c["segs"], c["R"], c["R2"]) is None

    def with_(what, k, col, v, *tail):
        b, g = c["blocks"].copy(), c["segs"].copy()
        (b if what == "b" else g)[k, col] = v
        return pc.check_blocks(b, g, *(tail or ok[2:]))

    rows = "a block outside the rows or out of order"
    assert with_("b", 1, 0, c["blocks"][0, 0]) == rows  # overlaps the block before it
    assert with_("b", 2, 1, 0) == rows and with_("b", 0, 0, -1) == rows
    assert pc.check_blocks(c["blocks"], c["segs"], c["R"] - pc.EDGE_TAIL - 1, c["R2"], 2, 8) == rows
    assert pc.check_blocks(c["blocks"], c["segs"], c["R"] - pc.EDGE_TAIL, c["R2"], 2, 8) is None
    segs = "a block's segments outside the segments"
    assert with_("b", 4, 4, 4) == segs and with_("b", 1, 3, -1) == segs and with_("b", 0, 4, -1) == segs
    assert with_("b", 3, 2, 2) == "a block of no scene" and with_("b", 3, 2, 2, c["R"], c["R2"], -1, 8) is None
    out = "a segment outside the expanded rows"
    assert with_("g", 0, 0, -1) == out
    assert pc.check_blocks(c["blocks"], c["segs"], c["R"], c["R2"] - pc.EDGE_HOLE - 1, 2, 8) == out  # the last segment
    assert pc.check_blocks(c["blocks"], c["segs"], c["R"], c["R2"] - pc.EDGE_HOLE, 2, 8) is None
    assert with_("g", 3, 1, 8) == "a segment of no model" and with_("g", 3, 1, 8, c["R"], c["R2"], 2, -1) is None
    # the first block that fails speaks, and inside a block the row complaint comes first
    b = c["blocks"].copy()
    b[3, 2], b[1, 1] = 5, 0
    assert pc.check_blocks(b, c["segs"], *ok[2:]) == rows


def test_the_block_cases_are_what_their_names_say():
    for c in _block_cases():
        nm = len(c["status"])
        assert pc.check_blocks(c["blocks"], c["segs"], c["R"], c["R2"], len(c["n_pts"]), nm) is None
        assert (c["model_scene"][c["segs"][:, 1]] == np.repeat(c["blocks"][:, 2], c["blocks"][:, 4])).all()
        of = pc.block_of_rows(c["blocks"], c["R"])
        inside = of >= 0
        assert inside.sum() == c["blocks"][:, 1].sum()
        for si, n in enumerate(c["n_pts"]):  # distinct points inside a scene: no order reaches the result
            p = c["row_point"][inside & (c["blocks"][np.maximum(of, 0), 2] == si)]
            assert len(np.unique(p)) == len(p) and p.min() >= 0 and p.max() < n
        # the expanded rows: every segment inside, no two overlap, holes between them
        n_of = np.repeat(c["blocks"][:, 1], c["blocks"][:, 4])
        order = np.argsort(c["segs"][:, 0])
        ends = (c["segs"][:, 0] + n_of)[order]
        assert (c["segs"][order, 0][1:] == ends[:-1] + pc.EDGE_HOLE).all() and c["R2"] == ends[-1] + pc.EDGE_HOLE
        assert (c["status"] != 0).any() and (c["status"][c["segs"][:, 1]] != 0).any()
    c = pc.compete_edge_case()
    b = c["blocks"]
    assert c["R"] == pc.ROW_CAP * pc.THREADS + 1000 == pc.EDGE_R
    assert b[0, 0] == 5 and c["R"] - (b[-1, 0] + b[-1, 1]) == 40
    gaps = b[1:, 0] - (b[:-1, 0] + b[:-1, 1])
    assert set(gaps) == {1, 300}
    assert {1, 255, 256, 257} <= set(b[:, 1]) and (b[:, 4] == 0).sum() == 1 and set(b[b[:, 4] > 0, 4]) == {2, 3}
    assert b[-1, 0] < pc.ROW_CAP * pc.THREADS < b[-1, 0] + b[-1, 1]  # the large block lies across the cap
    of = pc.block_of_rows(b, c["R"])
    assert (of[:5] == -1).all() and of[5] == 0 and (of[-40:] == -1).all() and of[-41] == len(b) - 1
    assert of[b[1, 0] - 1] == -1 and of[b[1, 0] - 2] == 0  # a gap of one row
    k = int(np.nonzero(gaps == 300)[0][0])
    assert (of[b[k, 0] + b[k, 1]:b[k + 1, 0]] == -1).all() and b[k + 1, 0] - b[k, 0] - b[k, 1] == 300
    one = pc.compete_single_case()
    assert len(one["blocks"]) == 1 and one["blocks"][0, 0] == 300 and one["R"] == 1000
    assert (pc.block_of_rows(one["blocks"], 1000) >= 0).sum() == 500


def test_block_of_rows_is_the_bisection():
    def bisect(blocks, r):  # block_of_row, statement by statement
        lo, hi = 0, len(blocks)
        while hi - lo > 1:
            mid = lo + ((hi - lo) >> 1)
            if blocks[mid][0] <= r:
                lo = mid
            else:
                hi = mid
        first = blocks[lo][0]
        return lo if (r >= first and r - first < blocks[lo][1]) else -1

    for c in (pc.compete_small_case(), pc.compete_single_case()):
        of = pc.block_of_rows(c["blocks"], c["R"])
        assert [bisect(c["blocks"], r) for r in range(c["R"])] == of.tolist()
        assert (of == -1).any() and of[0] == -1 and of[-1] == -1


def test_the_contract_reference_agrees_with_a_loop_over_the_rows():
    for c in (pc.compete_small_case(), pc.compete_single_case()):
        start = pc.compete_start(c)
        rows_a, outs_a, model_a = pc.contract_reference(c, start)
        rows_b, outs_b, model_b = pc.contract_loop(c, start)
        assert np.array_equal(rows_a, rows_b) and np.array_equal(model_a, model_b) and _same(outs_a, outs_b)
        assert (rows_a == pc.SENT).sum() == pc.EDGE_HOLE * len(c["segs"])  # the holes
        of = pc.block_of_rows(c["blocks"], c["R"])
        assert (model_a[of < 0] == -1).all() and (model_a >= 0).any()
        assert (model_a[(of >= 0) & (c["blocks"][np.maximum(of, 0), 4] == 0)] == -1).all()
        # ties are there and the first of them takes: the status matters, and so does the strictness
        no_status = dict(c, status=np.zeros_like(c["status"]))
        assert not np.array_equal(pc.contract_reference(no_status, start)[2], model_a)
    p = np.float32([[0.5, np.nan, 0.25, 0.0], [0.5, 0.75, np.nan, -1.0], [0.75, 0.75, 0.25, np.nan]])
    assert pc.first_maximum(p).tolist() == [2, 1, 0, -1]
    assert pc.first_maximum(np.float32([0.25, 0.5, 0.5])).tolist() == [1]


def test_an_expand_or_compete_that_did_not_wrap_is_told_apart():
    c = pc.compete_edge_case()
    start = pc.compete_start(c)
    rows, outs, model = pc.contract_reference(c, start)
    rows_c, outs_c, model_c = pc.contract_reference(c, start, row_limit=pc.ROW_CAP * pc.THREADS)
    assert not np.array_equal(rows, rows_c) and not np.array_equal(model, model_c) and not _same(outs, outs_c)
    assert (rows == pc.SENT).sum() == pc.EDGE_HOLE * len(c["segs"])


# ---------------------------------------------------------------------------------------------- vote
def _votes_by_candidate(c, k):
    """(candidate -> rows it took) of block k, from the per-row rule."""
    r0, n, _, s0, ns = c["blocks"][k]
    sg = c["segs"][s0:s0 + ns]
    took = pc.first_maximum(np.stack([c["pn"][o:o + n] for o, _ in sg]))
    lab = np.array([c["lab"][sg[s][0] + j] != 0 for j, s in enumerate(took)])
    return np.bincount(2 * took + lab, minlength=2 * ns), sg


def test_the_vote_cases_are_what_their_names_say():
    c = pc.vote_edge_case()
    b = c["blocks"]
    assert tuple(b[:, 4]) == pc.VOTE_SEGS == (0, 1, 127, 128, 129, 300, pc.VOTE_MAX_SEG) and (b[:, 1] == 300).all()
    assert pc.check_blocks(b, c["segs"], c["R"], c["R2"], 2, pc.VOTE_MODELS) is None
    assert (c["boxes"] >= 0).all() and (c["boxes"][:, 0] != c["boxes"][:, 1]).all() and not c["status"].any()
    for si in range(2):
        sp = c["block_spp"][b[:, 2] == si]
        assert len(np.unique(sp)) == len(sp) and sp.min() >= 0 and sp.max() < c["n_spps"][si]
    assert len(np.unique(c["segs"][:, 1])) >= 36
    tabs, out = pc.vote_reference(c, pc.vote_start(c))
    assert out[0].tolist() == [-1, -1, 0]
    for k, ns in enumerate(pc.VOTE_SEGS):
        if ns < 129:
            continue
        cnt, sg = _votes_by_candidate(c, k)
        box = np.array([c["boxes"][m][lb] for _, m in sg for lb in (0, 1)])
        votes = {int(x): int(cnt[box == x].sum()) for x in np.unique(box[cnt > 0])}
        assert cnt.sum() == 300 and (cnt[256:] > 0).any() and (cnt[:256] > 0).any()
        # a box argued by several voting candidates, one of them beyond index 256
        if ns > 129:  # (in the 129 block only candidates 256 and 257 lie behind the edge, and box 20 is theirs alone)
            assert any((cnt[box == x] > 0).sum() > 1 and (np.nonzero((box == x) & (cnt > 0))[0] >= 256).any() for x in votes)
        if ns in (129, 300):
            assert out[k].tolist() == [36, 20, 101] and votes[20] == 101 and votes[23] == 100
            assert np.nonzero((box == 20) & (cnt > 0))[0].min() >= 256  # the winner's candidates: all in the tail
            assert np.nonzero((box == 23) & (cnt > 0))[0].max() < 256 and max(v for x, v in votes.items() if x < 20) <= 99
    cnt, sg = _votes_by_candidate(c, 5)
    box = np.array([c["boxes"][m][lb] for _, m in sg for lb in (0, 1)])
    assert np.nonzero((box == 20) & (cnt > 0))[0].tolist() == [400, 501] and cnt[[400, 501]].tolist() == [60, 41]
    big = pc.vote_big_case()
    assert big["blocks"].tolist() == [[0, 70000, 0, 0, 3]]
    assert pc.check_blocks(big["blocks"], big["segs"], big["R"], big["R2"], 1, pc.VOTE_MODELS) is None
    mag = np.abs(big["mu"])
    assert mag.min() < 1e-29 and mag.max() > 1e5 and (big["mu"] < 0).any() and (big["mu"] > 0).any()
    grid = pc.vote_grid_case()
    nb = len(grid["blocks"])
    assert nb == pc.VOTE_GRID + 3 == grid["n_spps"][0] and (grid["blocks"][:, [1, 4]] == 1).all()
    assert pc.check_blocks(grid["blocks"], grid["segs"], grid["R"], grid["R2"], 1, pc.VOTE_MODELS) is None
    assert (grid["segs"][-3:, 1] == 36).all() and (grid["segs"][:-3, 1] < 4).all()
    assert len(np.unique(grid["block_spp"])) == nb and len(np.unique(grid["segs"][:, 0])) == nb


def test_the_vote_refusal_is_built_from_valid_tables():
    """One segment too many: block 0 (no segment) is given the first VOTE_MAX_SEG + 1 segments; every one of them lies
    inside the expanded rows because all blocks have 300 rows, so only the segment bound can refuse it."""
    c = pc.vote_edge_case()
    b = c["blocks"].copy()
    b[0, 3], b[0, 4] = 0, pc.VOTE_MAX_SEG + 1
    assert len(c["segs"]) >= pc.VOTE_MAX_SEG + 1
    assert pc.check_blocks(b, c["segs"], c["R"], c["R2"], 2, pc.VOTE_MODELS) is None
    b[0, 4] = pc.VOTE_MAX_SEG
    assert b[:, 4].max() == pc.VOTE_MAX_SEG


def test_a_vote_that_missed_its_tails_is_told_apart():
    c = pc.vote_edge_case()
    start = pc.vote_start(c)
    tabs, out = pc.vote_reference(c, start)
    tabs_c, out_c = pc.vote_reference(c, start, seg_limit=pc.THREADS // 2)  # candidates 0 .. 255 only
    for k, ns in enumerate(pc.VOTE_SEGS):
        if ns <= 128:
            assert out[k].tolist() == out_c[k].tolist()
        else:
            assert out[k, 1] != out_c[k, 1] or out[k, 2] != out_c[k, 2], ns
        if ns in (129, 300):
            assert (out[k, 1], out_c[k, 1]) == (20, 23)  # X itself changes
    assert not _same(tabs, tabs_c)
    grid = pc.vote_grid_case()
    start = pc.vote_start(grid)
    tabs, out = pc.vote_grid_reference(grid, start)
    tabs_c, out_c = pc.vote_grid_reference(grid, start, block_limit=pc.VOTE_GRID)
    assert (out[-3:, 0] == 36).all() and (out_c[-3:] == pc.SENT).all() and np.array_equal(out[:-3], out_c[:-3])
    assert not _same(tabs, tabs_c)
    assert (out[:, 2] == 0).sum() > 1000 and (out[:, 2] == 1).sum() > 200000  # the NaN pattern votes for nobody


def test_the_grid_reference_is_the_block_loop():
    small = pc.vote_grid_case(403)
    start = pc.vote_start(small)
    a, out_a = pc.vote_grid_reference(small, start)
    b, out_b = pc.vote_reference(small, start)
    assert np.array_equal(out_a, out_b) and _same(a, b)
    assert len(np.unique(small["segs"][:, 1] * 16 + small["pattern"])) > 50
