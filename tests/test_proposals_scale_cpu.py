"""The cases of tests/proposals_cases.py at workload size, without a device: every one is built around one loop or cap of
csrc/proposals.hip, and each must tell the definition from the kernel that runs that loop's first trip only.

``first_pass`` of tests/proposals_ref.py (and the two switches of ``rle_chunked_ref``) restate those wrong kernels.  A
switch must change the result of the case built for it and must not change the case just below the threshold.
"""
import numpy as np
import pytest

import proposals_cases as cases
import proposals_ref as ref

SMALL = dict(cases.cases())


def _same(a, b):
    return (a["status"] == b["status"] and a["stages"] == b["stages"] and np.array_equal(a["label_id"], b["label_id"])
            and np.array_equal(a["query"], b["query"]) and a["conf"].tobytes() == b["conf"].tobytes()
            and np.array_equal(a["masks"], b["masks"]))


def test_the_mirrored_constants_agree_with_the_header_and_with_each_other():
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "gapro_hip.h")).read()
    value = dict(re.findall(r"#define GAPRO_PROPOSALS_(GRID_CAP|MAX_PRE_TOPK|MAX_SEM2INS) (\d+)", text))
    value = {k: int(v) for k, v in value.items()}
    assert cases.PACK_PASS_WAVES == value["GRID_CAP"] * 4 and cases.GRID_PASS_ITEMS == value["GRID_CAP"] * 256
    assert (cases.MAX_TOPK, cases.MAX_SEM) == (value["MAX_PRE_TOPK"], value["MAX_SEM2INS"])
    assert cases.chunking(65535) == (64, 1024) and cases.chunking(65536) == (65, 1009)
    assert cases.chunking(1048575) == (1024, 1024) and cases.chunking(1048576) == (1024, 1025)
    assert cases.chunking(1300001) == (1024, 1270)


@pytest.mark.parametrize("name", cases.SCALE_NAMES)
def test_counts_decode_back_and_the_chunked_algorithm_gives_the_same_counts(name):
    out = cases.scale_reference(name)
    assert out["status"] == ref.OK and len(out["conf"]) > 0
    n = len(cases.scale_case(name)["v2p_map"])
    for mask, counts in zip(out["masks"], out["counts"]):
        assert counts.dtype == np.int64 and len(counts) % 2 == 0
        if len(counts) <= 4096:
            assert np.array_equal(ref.rle_decode_ref(n, counts), mask.astype(np.uint8))
        step = np.zeros(n + 1, np.int64)  # the same rule without a loop over a million runs
        step[counts[0::2] - 1] += 1
        step[counts[0::2] - 1 + counts[1::2]] -= 1
        assert np.array_equal(np.cumsum(step)[:n], mask.astype(np.int64)) and (counts[1::2] > 0).all()
        assert np.array_equal(ref.rle_chunked_ref(mask), counts)


@pytest.mark.parametrize("name", [n for n in cases.SCALE_NAMES if cases.scale_case(n).get("voxel_spps") is not None])
def test_both_mask_forms_agree_in_the_restatement(name):
    c = cases.scale_case(name)
    wide = dict(c, mask_logits=np.ascontiguousarray(c["mask_logits"][:, c["voxel_spps"]]), voxel_spps=None)
    assert _same(cases.scale_reference(name), ref.get_instance_ref(**wide))


def _case(name):
    return SMALL[name] if name in SMALL else cases.scale_case(name)


def _definition(name):
    return ref.get_instance_ref(**SMALL[name]) if name in SMALL else cases.scale_reference(name)


# switch -> (the cases it must change, the cases just below its threshold it must leave alone)
FIRST_PASS = {
    "pack_run": (("pack_v2049", "pack_v4097"), ("pack_v2048",)),
    "pack_grid": (("pack_grid_q8200",), ("pack_grid_q8192",)),
    "inter": (("pack_v4097",), ("pack_v2048", "pack_v2049")),
    "score_grid": (("scores_at_the_cap",), ("tie_across_65536",)),
    "points_grid": (("points_1048575", "points_1048576", "points_1300001"), ("points_65536", "points_65537")),
    "tally": (("points_65537", "points_1048575", "points_1048576", "points_1300001"), ("points_65535", "points_65536")),
    "index16": (("tie_across_65536", "scores_at_the_cap"), ("tie_across_256", "scores_1025")),
    "index8": (("tie_across_256", "tie_across_65536", "scores_at_the_cap"), ("tie_across_cut", "tie_inside")),
    "nms256": (("nms_victims_257_behind",), ("nms_victims_256_behind", "p1024_standard_all")),
    "finish_rows": (("p1024_standard_all", "p1024_matrix_topk"), ("p1024_matrix_none", "scores_1024")),
}


def test_every_switch_of_the_restatement_has_its_cases():
    assert set(FIRST_PASS) == set(ref.FIRST_PASS)


@pytest.mark.parametrize("switch", sorted(FIRST_PASS))
def test_a_first_pass_only_kernel_would_show_and_the_case_below_does_not_reach_it(switch):
    bites, below = FIRST_PASS[switch]
    for name in bites:
        assert not _same(_definition(name), ref.get_instance_ref(**_case(name), first_pass=switch)), name
    for name in below:
        assert _same(_definition(name), ref.get_instance_ref(**_case(name), first_pass=switch)), name


def _rle_rows(n_points):
    return cases.scale_reference("points_%d" % n_points)["masks"]


@pytest.mark.parametrize("switch, bites, below", (
    ("drop_carry", (65536, 1048575, 1048576, 1300001), (65535,)),
    ("hold_chunk_len", (1048576, 1300001), (65535, 65536, 1048575))))
def test_a_scan_without_its_carry_and_a_chunk_that_does_not_grow_would_show(switch, bites, below):
    for n in bites:  # at 1 048 576 points only the position N is beyond the chunks: the row of all ones closes there
        rows = _rle_rows(n)
        assert not np.array_equal(ref.rle_chunked_ref(rows[0], **{switch: True}), ref.rle_ref(rows[0])), n
    for n in below:
        for mask in _rle_rows(n):
            assert np.array_equal(ref.rle_chunked_ref(mask, **{switch: True}), ref.rle_ref(mask)), n


@pytest.mark.parametrize("n_points", (65535, 65536, 65537, 1048575, 1048576, 1300001))
def test_the_rows_of_a_large_scene_meet_every_chunk_boundary(n_points):
    c, out = cases.scale_case("points_%d" % n_points), cases.scale_reference("points_%d" % n_points)
    assert list(out["query"]) == [0, 1, 2, 3] and len(c["v2p_map"]) == n_points
    assert list(out["counts"][0]) == [1, n_points]                             # all ones
    assert np.array_equal(out["masks"][1], np.arange(n_points) % 2 == 0)       # alternates every point
    m = np.concatenate([[0], out["masks"][3].astype(np.int8), [0]])
    trans = set(np.nonzero(m[1:] != m[:-1])[0].tolist())
    nchunks, chunk = cases.chunking(n_points)
    three = set(np.nonzero(c["spps"] == 16)[0].tolist())  # the superpoint of three points is no part of row 3
    for b in [chunk * i for i in range(1, nchunks + 1)]:
        for p in (b - 1, b, b + 1):
            assert p >= n_points or p in trans or p in three or p - 1 in three, (b, p)
    assert nchunks > cases.SCAN_CHUNKS or n_points == 65535
    # the points beyond one pass of `tally` decide superpoints of row 2, those beyond one pass of `points` others
    part = ref.refine_ref(ref.bits_ref(c["mask_logits"], 0.0)[2:3], c["v2p_map"], c["spps"], c["n_spps"],
                          c_from=cases.TALLY_PASS_POINTS)
    assert (part[0][cases.TALLY_PASS_POINTS:] != out["masks"][2][cases.TALLY_PASS_POINTS:]).any() == (n_points > 65536)


def test_a_tie_is_cut_at_the_lowest_indices_of_its_block():
    for name, lo, hi, higher, n in (("tie_across_65536", 65300, 65800, 100, 66000),
                                    ("tie_across_256", 100, 1300, 100, 2000),
                                    ("scores_at_the_cap", 0xC0000 - 300, 0xC0000 + 300, 200, 1 << 20)):
        c, out = cases.scale_case(name), cases.scale_reference(name)
        s = ref.scores_ref(c["cls_logits"], c["conf_logits"]).reshape(-1)
        assert len(s) == n and len(set(s[lo:hi].tobytes()[i:i + 4] for i in range(0, 4 * (hi - lo), 4))) == 1
        assert s[:lo].max() < s[lo] and s[hi:n - higher].max() < s[lo] < s[n - higher:].min()
        taken = c["pre_topk"] - higher
        want = np.r_[np.arange(n - higher, n)[np.argsort(-s[n - higher:], kind="stable")], np.arange(lo, lo + taken)]
        assert np.array_equal(out["query"], want) and 0 < taken < hi - lo
    assert 65300 + 300 > 65536 and 100 + 924 > 256 and 0xC0000 - 300 + 312 > 0xC0000  # the cut lies beyond the carry


def test_pre_topk_1024_takes_all_of_1024_scores_and_drops_the_least_of_1025():
    a, b = cases.scale_reference("scores_1024"), cases.scale_reference("scores_1025")
    assert a["stages"] == (1024, 1024, 1024, 1024) and b["stages"] == (1024, 1024, 1024, 1024)
    c = cases.scale_case("scores_1025")
    s = ref.scores_ref(c["cls_logits"], c["conf_logits"]).reshape(-1)
    flat = b["query"].astype(np.int64) * 5 + b["label_id"] - 1
    assert len(s) == 1025 and sorted(set(range(1025)) - set(flat.tolist())) == [int(np.argmin(s))]
    assert (np.diff(a["conf"].astype(np.float64)) < 0).all()


def test_the_1024_candidate_cases_fill_the_sorts_and_reach_1032_rows():
    for name, rows in (("p1024_standard_all", 1032), ("p1024_matrix_topk", 1032)):
        out = cases.scale_reference(name)
        assert out["stages"] == (1024, 1024, 1024, 1024) and len(out["conf"]) == rows
        assert list(out["query"][:8]) == [-1] * 8 and list(out["label_id"][:8]) == list(range(1, 9))
    out = cases.scale_reference("p1024_matrix_none")
    assert out["stages"][:2] == (1024, 1024) and 256 < out["stages"][2] < 1024
    assert (out["conf"] >= np.float32(0.1)).all()
    for name in ("nms_victims_256_behind", "nms_victims_257_behind"):
        out = cases.scale_reference(name)
        assert out["stages"][1] == 1024 and not np.isin(out["query"], np.arange(200) + int(name.split("_")[2])).any()


def test_mask_nms_at_1024_proposals_tells_the_first_trips_apart():
    bits, cat, score, _ = cases.nms_1024_inputs()
    order = ref.order_ref(score, len(score))
    b, k, s = bits[order], cat[order], score[order]
    cases.guard_values("mask_nms_1024", s)
    _, new = ref.nms_ref(b, k, s, "matrix", len(s))  # every updated score, in descending order
    cases.guard_values("mask_nms_1024", new, 0.1)
    assert 256 < int((new >= np.float32(0.1)).sum()) < 1024
    _, cut = ref.nms_ref(b, k, s, "matrix", len(s), first_pass=("inter",))  # the 65th word is part of the IoU
    assert cut.tobytes() != new.tobytes()
    keep, _ = ref.nms_ref(b, k, s, "standard", -1, 0.2)
    blind, _ = ref.nms_ref(b, k, s, "standard", -1, 0.2, first_pass=("nms256",))
    assert 32 < len(keep) < 1024 and not np.array_equal(blind, keep)  # victims more than 256 places behind a pivot
