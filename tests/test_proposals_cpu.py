"""The predicted-instance chain without a device: the NumPy restatement tests/proposals_ref.py against what the real
reference returned (tests/golden/proposals_*.npz, written by tests/golden/make_golden_proposals.py), and the edge cases
of tests/proposals_cases.py against the wrong conventions they are built to catch.

Labels and run lengths agree with the reference exactly, under the order-free comparison (the reference's order is not
defined).  ``conf``: the restatement evaluates in float64 and rounds once, the reference runs a float32 chain of
softmax, product, square root, two exp and a quotient.  The largest relative deviation measured over the fixtures is
2.18e-7 (make_golden_proposals.py prints it); the test allows four times that, 8.72e-7, which is below the 2e-6 beyond
which something other than rounding would differ.
"""
import ctypes as C

import numpy as np
import pytest

import proposals_cases as cases
import proposals_ref as ref

MEASURED_CONF_DEVIATION = 2.18e-7
CONF_TOL = 4 * MEASURED_CONF_DEVIATION
CASES = dict(cases.cases())


def test_the_tolerance_is_four_times_the_measured_deviation_and_within_rounding():
    assert CONF_TOL == 4 * MEASURED_CONF_DEVIATION and CONF_TOL <= 2e-6


@pytest.mark.parametrize("name", ref.FIXTURES)
def test_restatement_equals_the_reference(name):
    kw, (label, conf, counts) = ref.load_fixture(name)
    ours = ref.get_instance_ref(**kw)
    dev = ref.compare_with_reference(ours, label, conf, counts)
    print("%s: largest relative conf deviation %.3g" % (name, dev))
    assert dev <= CONF_TOL
    assert len(label) > 0


def test_the_fixtures_cover_both_nms_types_and_sem2ins():
    kinds = {ref.load_fixture(n)[0]["type_nms"] for n in ref.FIXTURES}
    assert kinds == {"matrix", "standard"}
    kw, (label, conf, _) = ref.load_fixture("s3dis")
    assert kw["sem2ins_classes"] == (0, 1) and list(label[:2]) == [1, 2] and list(conf[:2]) == [1.0, 1.0]
    assert kw["label_shift"] == 3 and label[2:].min() >= 3


@pytest.mark.parametrize("name", sorted(CASES))
def test_counts_decode_back_to_the_masks(name):
    out = ref.get_instance_ref(**CASES[name])
    assert out["status"] == ref.OK
    n = len(CASES[name]["v2p_map"])
    for mask, counts in zip(out["masks"], out["counts"]):
        assert counts.dtype == np.int64 and len(counts) % 2 == 0
        assert np.array_equal(ref.rle_decode_ref(n, counts), mask.astype(np.uint8))
        assert (counts[1::2] > 0).all() and (np.diff(counts[0::2]) > 0).all()


def _same(a, b):
    return (a["status"] == b["status"] and np.array_equal(a["label_id"], b["label_id"])
            and np.array_equal(a["query"], b["query"]) and a["conf"].tobytes() == b["conf"].tobytes()
            and np.array_equal(a["masks"], b["masks"]))


@pytest.mark.parametrize("V", (63, 65, 129))
def test_tail_bits_kept_would_show(V):
    c = CASES["tail_v%d" % V]
    assert not _same(ref.get_instance_ref(**c), ref.get_instance_ref(**c, wrong_tail=True))


def test_a_whole_last_word_has_no_tail():
    c = CASES["tail_v64"]
    assert _same(ref.get_instance_ref(**c), ref.get_instance_ref(**c, wrong_tail=True))


def test_ties_go_to_the_lower_flat_index():
    c = CASES["tie_across_cut"]
    s = ref.scores_ref(c["cls_logits"], c["conf_logits"]).reshape(-1)
    assert s[2].tobytes() == s[3].tobytes()  # bit-identical across the cut
    out, wrong = ref.get_instance_ref(**c), ref.get_instance_ref(**c, tie_desc_index=True)
    assert list(out["query"]) == [0, 1, 2] and list(wrong["query"]) == [0, 1, 3]
    c = CASES["tie_inside"]
    out, wrong = ref.get_instance_ref(**c), ref.get_instance_ref(**c, tie_desc_index=True)
    assert not _same(out, wrong)
    # q2 comes first and decays q3, not the reverse
    i2, i3 = list(out["query"]).index(2), list(out["query"]).index(3)
    assert out["conf"][i2] > out["conf"][i3]


def test_pre_topk_below_equal_and_above_the_number_of_scores():
    stages = {n: ref.get_instance_ref(**CASES[n])["stages"] for n in ("qc_below", "qc_equal", "qc_above")}
    assert stages["qc_below"][0] == 144 and stages["qc_equal"][0] == 144 and stages["qc_above"][0] == 100


def test_npoint_threshold_is_inclusive():
    out = ref.get_instance_ref(**CASES["npoint_at_and_below"])
    assert list(out["query"]) == [1] and out["stages"] == (4, 1, 1, 1)
    out = ref.get_instance_ref(**CASES["all_below_npoint"])
    assert out["status"] == ref.OK and len(out["conf"]) == 0 and out["counts"] == [] and out["masks"].shape == (0, 64)


def test_suppression_stays_inside_a_class():
    c = CASES["same_query_two_classes"]
    out, wrong = ref.get_instance_ref(**c), ref.get_instance_ref(**c, cross_class=True)
    assert list(out["query"]) == [0, 0, 1, 1] and list(out["label_id"]) == [1, 2, 1, 2]
    assert list(wrong["query"]) == [0, 1]
    out = ref.get_instance_ref(**CASES["identical_masks_one_class"])
    assert list(out["query"]) == [0, 2]
    out = ref.get_instance_ref(**CASES["identical_masks_matrix"])
    s = ref.scores_ref(CASES["identical_masks_matrix"]["cls_logits"], np.ones(3, np.float32)).reshape(-1)
    assert list(out["query"]) == [0, 2]  # q1 decays by exp(-2) to 0.054 and falls below final_score_thresh
    assert np.float32(np.float64(s[1]) * np.exp(-2.0)) < np.float32(0.1)


def test_an_iou_equal_to_the_threshold_does_not_suppress():
    c = CASES["iou_equals_threshold"]
    bits = ref.bits_ref(c["mask_logits"], 0.0)
    assert ref.iou_ref(bits)[0, 1] == np.float32(0.25) and c["nms_threshold"] == 0.25
    assert list(ref.get_instance_ref(**c)["query"]) == [0, 1]
    lower = dict(c, nms_threshold=0.2499)
    assert list(ref.get_instance_ref(**lower)["query"]) == [0]


@pytest.mark.parametrize("name, rows", (("rows_68", 68), ("rows_132", 132)))
def test_more_rows_than_one_and_two_instance_words(name, rows):
    out = ref.get_instance_ref(**CASES[name])
    assert out["stages"][2] == rows and out["stages"][3] > 64


def test_topk_beyond_the_survivors_none_and_cutting():
    a, b, c = (ref.get_instance_ref(**CASES[n]) for n in ("topk_beyond", "topk_none", "topk_cuts"))
    assert a["stages"][1] < 100 and a["stages"][2] == a["stages"][1]
    assert b["stages"][2] == int((a["conf"] >= np.float32(0.1)).sum()) < a["stages"][2]
    assert c["stages"][2] == 5 and np.array_equal(c["query"], a["query"][:5])
    for out in (a, b, c):
        assert (np.diff(out["conf"].astype(np.float64)) <= 0).all()


def test_half_is_inclusive_and_the_other_superpoint_rules():
    c = CASES["spp_rules"]
    out, strict = ref.get_instance_ref(**c), ref.get_instance_ref(**c, half_strict=True)
    spps = np.asarray(c["spps"])
    m = out["masks"][0]
    assert m[spps == 0].all() and not strict["masks"][0][spps == 0].any()  # 2 c == n
    assert not m[spps == 1].any()                                          # c == 0
    assert m[spps == 2].all() and not (spps == 3).any() and c["n_spps"] == 7
    assert not m[spps == 4].any() and m[spps == 5].all()                   # 1 of 3, 2 of 3
    assert not _same(out, strict)
    assert not np.isin([10, 11], c["v2p_map"]).any() and (np.diff(spps) < 0).any()


def test_a_row_can_lose_and_gain_points_in_the_refinement():
    c = CASES["lose_and_gain"]
    out = ref.get_instance_ref(**c)
    raw = ref.bits_ref(c["mask_logits"], 0.0)[:, c["v2p_map"]].sum(axis=1)
    assert list(raw) == [6, 5] and out["stages"] == (2, 2, 2, 1)
    assert list(out["query"]) == [1] and int(out["masks"][0].sum()) == 8


def test_run_shapes():
    out = ref.get_instance_ref(**CASES["run_shapes"])
    counts = {int(q): list(c) for q, c in zip(out["query"], out["counts"])}
    assert counts[0] == [1, 5] and counts[1] == [191, 10] and counts[2] == [1, 200]
    assert counts[3] == [v for i in range(100) for v in (2 * i + 1, 1)]
    assert counts[4][:2] == [2, 1] and counts[4][-2:] == [200, 1]
    assert counts[5] == [61, 10, 121, 10, 192, 2] and counts[6] == [1, 1, 64, 2, 128, 2, 200, 1]


def test_sem2ins_rows_come_first_with_and_without_ordinary_rows():
    a, b = ref.get_instance_ref(**CASES["sem2ins_with_rows"]), ref.get_instance_ref(**CASES["sem2ins_alone"])
    for out in (a, b):
        assert list(out["label_id"][:2]) == [1, 3] and list(out["query"][:2]) == [-1, -1]
        assert list(out["conf"][:2]) == [1.0, 1.0] and not out["box"][:2].any()
    assert len(a["conf"]) > 2 and len(b["conf"]) == 2 and a["label_id"][2:].min() >= 3
    assert np.array_equal(a["masks"][:2], b["masks"][:2])


@pytest.mark.parametrize("name, case, status, flags", list(cases.refusals()), ids=[r[0] for r in cases.refusals()])
def test_refusals_of_the_data(name, case, status, flags):
    out = ref.get_instance_ref(**case)
    assert out["status"] == status and out["flags"] == flags and "conf" not in out


def test_a_non_finite_mask_value_counts_only_in_a_candidate_row():
    bad, fine = cases.mask_refusal()
    out = ref.get_instance_ref(**bad)
    assert out["status"] == ref.ERR_NOT_FINITE and out["flags"] == ref.FLAG_MASK
    assert ref.get_instance_ref(**fine)["status"] == ref.OK


def test_both_mask_forms_agree_in_the_restatement():
    for name in ("topk_beyond", "standard_scene", "sem2ins_with_rows"):
        c = CASES[name]
        wide = dict(c, mask_logits=np.ascontiguousarray(c["mask_logits"][:, c["voxel_spps"]]), voxel_spps=None)
        assert _same(ref.get_instance_ref(**c), ref.get_instance_ref(**wide))


# ---- the library, without a device: what it refuses before anything is launched ------------------------------------
def _sizes(mode=0, Q=384, C_=18, V=100000, N=150000, S=2500, **par):
    from gapro_amd import _lib

    lib = _lib.load()
    i = _lib.ProposalsInputs(n_queries=Q, n_voxels=V, n_points=N, n_spps=S)
    p = dict(mode=mode, instance_classes=C_, pre_topk=300, type_nms=0, topk=100, npoint_thresh=100)
    p.update(par)
    p = _lib.ProposalsParams(**p)
    return (int(lib.gapro_proposals_workspace_bytes(C.byref(i), C.byref(p))),
            int(lib.gapro_proposals_header_bytes(C.byref(i), C.byref(p))))


def test_workspace_and_header_sizes_and_the_refused_sizes():
    from gapro_amd import _lib

    ws, hdr = _sizes()
    assert ws > 0 and ws % 256 == 0 and hdr == C.sizeof(_lib.ProposalsHeader) + 4 * 100 == 40 + 400  # topk rows
    assert _sizes(topk=-1)[1] == 40 + 4 * 300 and _sizes(type_nms=1)[1] == 40 + 4 * 300  # nothing cuts below pre_topk
    assert _sizes(n_sem2ins=2)[1] == 40 + 4 * 102 and _sizes(topk=0)[1] == 40 + 4
    assert _sizes(Q=10, topk=-1)[1] == 40 + 4 * 180  # Q C below pre_topk
    for bad in (dict(npoint_thresh=0), dict(pre_topk=0), dict(pre_topk=1025), dict(Q=(1 << 20) // 18 + 1),
                dict(V=1 << 31), dict(N=1 << 31), dict(type_nms=2), dict(mode=3), dict(topk=-2), dict(n_sem2ins=9),
                dict(Q=0), dict(V=0), dict(N=0), dict(S=0), dict(C_=0), dict(S=(1 << 31) // 100 + 1)):
        assert _sizes(**bad) == (0, 0), bad
    assert _sizes(pre_topk=1024)[0] > ws and _sizes(V=(1 << 31) - 1, Q=1)[0] > 0
    assert _sizes(mode=_lib.PROPOSALS_NMS, Q=1024)[1] == 40 + 4 * 1024 and _sizes(mode=_lib.PROPOSALS_NMS, Q=1025) == (0, 0)
    assert _sizes(mode=_lib.PROPOSALS_RLE, Q=1032)[0] > 0 and _sizes(mode=_lib.PROPOSALS_RLE, Q=1033) == (0, 0)


def test_the_entry_points_are_exported():
    import gapro_amd

    for name in ("get_instance", "mask_nms", "rle_encode_gpu_batch"):
        assert name in gapro_amd.__all__ and callable(getattr(gapro_amd, name))
