"""SPFormer's predicted-instance chain without a device: the NumPy restatement tests/spf_predict_ref.py against what the
real reference returned (tests/golden/spf_predict_*.npz, written by tests/golden/make_golden_spf_predict.py), on
hand-checked tiny cases, and the edge cases of tests/spf_predict_cases.py against the wrong conventions they are built to
catch.

Labels, run lengths and boxes agree with the reference exactly, under the order-free comparison (the reference's order is
not defined).  ``conf``: the restatement evaluates in float64 and rounds once, the reference runs a float32 chain of
softmax, product, sigmoid, sum, quotient and product.  The largest relative deviation measured over the fixtures is
3.49e-7 (make_golden_spf_predict.py prints it); the test allows four times that, 1.4e-6, which is below the 2e-6 beyond
which something other than rounding would differ.
"""
import ctypes as C

import numpy as np
import pytest

import spf_predict_cases as cases
import spf_predict_ref as ref

MEASURED_CONF_DEVIATION = 3.49e-7
CONF_TOL = 4 * MEASURED_CONF_DEVIATION
CASES = dict(cases.cases())


def test_the_tolerance_is_four_times_the_measured_deviation_and_within_rounding():
    assert CONF_TOL == 4 * MEASURED_CONF_DEVIATION and CONF_TOL <= 2e-6


@pytest.mark.parametrize("name", ref.FIXTURES)
def test_restatement_equals_the_reference(name):
    kw, (label, conf, counts, box) = ref.load_fixture(name)
    ours = ref.predict_ref(**kw)
    dev = ref.compare_with_reference(ours, label, conf, counts, box)
    print("%s: largest relative conf deviation %.3g" % (name, dev))
    assert dev <= CONF_TOL
    assert len(label) > 0
    assert all(c.dtype == np.int64 for c in ours["counts"]) and ours["box"].dtype == np.float32


def test_the_fixtures_cover_what_they_are_named_for():
    import os

    stages = {}
    for name in ref.FIXTURES:
        kw, (label, conf, counts, box) = ref.load_fixture(name)
        stages[name] = (ref.predict_ref(**kw)["stages"], kw)
        golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
        assert os.path.getsize(os.path.join(golden, "spf_predict_%s.npz" % name)) <= max(
            os.path.getsize(os.path.join(golden, f)) for f in os.listdir(golden) if f.startswith("proposals_"))
        assert kw["labels"].shape[0] <= 48 and kw["masks"].shape[1] <= 200 and len(kw["superpoints"]) <= 6000
    (k, s, r), kw = stages["plain"]
    assert k == kw["topk_insts"] == 100 and r > 0
    (k, s, r), kw = stages["few_queries"]
    assert k == kw["labels"].shape[0] * kw["num_class"] < kw["topk_insts"]
    (k, s, r), kw = stages["score_thr"]
    assert kw["score_thr"] > 0 and 0 < s < k and r > 0
    (k, s, r), kw = stages["npoint_negative"]
    assert (kw["pred_scores"] < 0).any() and 0 < r < s < k  # negative scores among the candidates; both thresholds cut


@pytest.mark.parametrize("name", sorted(CASES))
def test_counts_decode_back_to_the_masks(name):
    out = ref.predict_ref(**CASES[name])
    assert out["status"] == ref.OK
    n = len(CASES[name]["superpoints"])
    for mask, counts, npoints in zip(out["masks"], out["counts"], out["npoints"]):
        assert counts.dtype == np.int64 and len(counts) % 2 == 0
        back = np.zeros(n, np.uint8)
        for lo, num in zip(counts[0::2], counts[1::2]):
            back[lo - 1:lo - 1 + num] = 1
        assert np.array_equal(back, mask.astype(np.uint8)) and mask.sum() == npoints
        assert (counts[1::2] > 0).all() and (np.diff(counts[0::2]) > 0).all()


def test_the_boxes_are_those_of_the_points():
    for name in ("mixed_sign_coords", "empty_superpoints", "points_1025"):
        c = CASES[name]
        out = ref.predict_ref(**c)
        assert len(out["conf"]) > 0
        for mask, box in zip(out["masks"], out["box"]):
            xyz = c["coords_float"][mask]
            assert np.array_equal(box[:3], xyz.min(axis=0)) and np.array_equal(box[3:], xyz.max(axis=0))


# ---- hand-checked tiny cases -----------------------------------------------------------------------------------------
def _tiny(**kw):
    """One class, two queries, three superpoints over five points."""
    c = dict(labels=np.array([[0.0, 0.0], [np.log(3.0), 0.0]], np.float32), pred_scores=np.array([1.0, 0.5], np.float32),
             masks=np.array([[1.0, -1.0, 0.0], [-2.0, 0.0, 3.0]], np.float32),
             superpoints=np.array([0, 0, 2, 1, 2]), num_class=1, topk_insts=5, score_thr=0.0, npoint_thr=0,
             coords_float=np.array([[0, 1, 2], [3, -1, 2], [5, 5, 5], [9, 9, 9], [-4, 6, 0.5]], np.float32))
    c.update(kw)
    return c


def test_hand_checked_two_queries():
    out = ref.predict_ref(**_tiny())
    # class scores: softmax([0, 0])[0] * 1 = 0.5; softmax([log 3, 0])[0] * 0.5 = 0.375: query 0 first
    assert np.allclose(out["cand_scores"], [0.5, 0.375], rtol=1e-6, atol=0)
    sig1, sig3 = 1 / (1 + np.exp(-1.0)), 1 / (1 + np.exp(-3.0))
    want = np.array([0.5 * sig1 / (1 + 1e-6), 0.375 * sig3 / (1 + 1e-6)], np.float64).astype(np.float32)
    # conf: 0.3655 and 0.3572: the order of the class scores survives
    assert out["conf"].tobytes() == want.tobytes() and list(out["query"]) == [0, 1] and list(out["label_id"]) == [1, 1]
    assert [list(x) for x in out["counts"]] == [[1, 2], [3, 1, 5, 1]] and list(out["npoints"]) == [2, 2]
    assert out["box"].tolist() == [[0, -1, 2, 3, 1, 2], [-4, 5, 0.5, 5, 6, 5]]
    assert out["stages"] == (2, 2, 2)


def test_hand_checked_order_follows_conf_not_the_class_score():
    # query 0 has the larger class score (0.5 against 0.75 * 0.6 = 0.45) but a mask logit of 0.1: sigmoid 0.525
    c = _tiny(pred_scores=np.array([1.0, 0.6], np.float32), masks=np.array([[0.1, -1, -1], [-2, -1, 6]], np.float32))
    out = ref.predict_ref(**c)
    assert np.allclose(out["cand_scores"], [0.5, 0.45]) and list(out["query"]) == [1, 0]
    assert np.allclose(out["conf"], [0.45 / (1 + np.exp(-6.0)), 0.5 / (1 + np.exp(-0.1))], rtol=1e-5)


def test_hand_checked_thresholds():
    out = ref.predict_ref(**_tiny(npoint_thr=2))  # both rows have two points: none has more
    assert out["stages"] == (2, 2, 0) and out["box"].shape == (0, 6) and out["masks"].shape == (0, 5)
    out = ref.predict_ref(**_tiny(score_thr=0.36))
    assert out["stages"] == (2, 1, 1) and list(out["query"]) == [0]
    out = ref.predict_ref(**_tiny(topk_insts=1))
    assert out["stages"] == (1, 1, 1) and list(out["query"]) == [0]


def test_the_order_image_orders_floats_and_comes_back():
    x = np.array([-np.inf, -3.5, -1e-30, -0.0, 0.0, 1e-30, 2.0, np.inf], np.float32)
    u = ref.order_image(x)
    assert (np.diff(u.astype(np.int64)) > 0).all()  # -0.0 strictly below +0.0
    assert ref.order_image_inv(u).tobytes() == x.tobytes()


# ---- the wrong conventions, each shown to fail the case built to catch it ------------------------------------------------
def _same(a, b):
    return (a["status"] == b["status"] and a["stages"] == b["stages"] and np.array_equal(a["label_id"], b["label_id"])
            and np.array_equal(a["query"], b["query"]) and a["conf"].tobytes() == b["conf"].tobytes()
            and np.array_equal(a["masks"], b["masks"]) and a["box"].tobytes() == b["box"].tobytes())


def test_zero_logits_are_not_set():
    c = CASES["zero_logits_not_set"]
    assert (c["masks"] == 0).any() and np.signbit(c["masks"][c["masks"] == 0]).any()
    out, wrong = ref.predict_ref(**c), ref.predict_ref(**c, ge_bits=True)
    assert not _same(out, wrong) and not np.array_equal(out["masks"], wrong["masks"])
    c = CASES["empty_row_score_thr_negative"]  # a row of -0.0 has no bit
    assert ref.predict_ref(**c)["stages"] != ref.predict_ref(**c, ge_bits=True)["stages"]


def test_the_score_threshold_is_strict():
    c = CASES["conf_equals_score_thr"]
    out, wrong = ref.predict_ref(**c), ref.predict_ref(**c, ge_score_thr=True)
    assert wrong["stages"][1] == out["stages"][1] + 1
    assert np.float32(c["score_thr"]) in wrong["conf"] and np.float32(c["score_thr"]) not in out["conf"]
    c = CASES["empty_row_score_thr_zero"]  # conf 0 against the threshold 0
    assert ref.predict_ref(**c)["stages"][1] < ref.predict_ref(**c, ge_score_thr=True)["stages"][1]


def test_the_point_threshold_is_strict():
    c = CASES["npoints_at_the_threshold"]
    out, wrong = ref.predict_ref(**c), ref.predict_ref(**c, ge_npoint_thr=True)
    assert list(out["npoints"]) == [11] * len(out["npoints"]) and len(out["npoints"]) > 0
    assert sorted(set(wrong["npoints"])) == [10, 11]


def test_the_top_k_is_taken_before_the_mask_score():
    c = CASES["topk_before_mask_score"]
    out, wrong = ref.predict_ref(**c), ref.predict_ref(**c, topk_after=True)
    assert list(out["query"]) == [1, 0] and list(wrong["query"]) == [1, 2]


def test_the_softmax_keeps_the_last_column_in_its_sum():
    c = CASES["scores_below_topk"]
    out, wrong = ref.predict_ref(**c), ref.predict_ref(**c, renorm=True)
    assert out["conf"].tobytes() != wrong["conf"].tobytes() and (wrong["conf"].max() > out["conf"].max())


def test_the_flat_index_is_divided_by_the_class_count():
    c = CASES["one_query_two_classes"]
    out, wrong = ref.predict_ref(**c), ref.predict_ref(**c, div_c1=True)
    assert sorted(out["label_id"][out["query"] == 2][:2]) == [1, 3]  # one query under two classes
    assert not np.array_equal(out["query"], wrong["query"])


def test_the_mask_score_has_its_epsilon():
    c = CASES["one_point_instance"]  # masks of one or two superpoints: the epsilon is 1e-6 / 5e-7 of the value
    out, wrong = ref.predict_ref(**c), ref.predict_ref(**c, no_eps=True)
    assert np.array_equal(out["query"], wrong["query"]) and out["conf"].tobytes() != wrong["conf"].tobytes()
    assert (np.abs(out["conf"] / wrong["conf"] - 1) < 2e-6).all()


def test_label_ids_start_at_one():
    c = CASES["scores_below_topk"]
    out, wrong = ref.predict_ref(**c), ref.predict_ref(**c, label_c=True)
    assert np.array_equal(out["label_id"], wrong["label_id"] + 1) and out["label_id"].min() >= 1


def test_ties_go_to_the_lower_flat_index_and_keep_the_candidate_order():
    c = CASES["tie_across_cut"]
    s = ref.class_scores64(c["labels"], c["pred_scores"]).astype(np.float32)
    assert s[1].tobytes() == s[4].tobytes()  # bit-identical rows, one on either side of the cut
    out = ref.predict_ref(**c)
    assert 1 in out["query"] and 4 not in out["query"]
    c = CASES["tie_inside"]
    out = ref.predict_ref(**c)
    conf = out["conf"]
    pairs = [(i, i + 1) for i in range(len(conf) - 1) if conf[i].tobytes() == conf[i + 1].tobytes()]
    assert len(pairs) == 3  # the three classes of queries 1 and 4: identical conf, the lower query first
    assert all((out["query"][i], out["query"][j]) == (1, 4) for i, j in pairs)


def test_a_tie_across_index_65536_is_cut_at_the_lowest_indices_of_its_block():
    c = CASES["tie_across_65536"]
    n, lo, hi, higher, topk = cases.TIE_BLOCK
    s = ref.class_scores64(c["labels"], c["pred_scores"]).reshape(-1).astype(np.float32)
    assert len(s) == n and len(np.unique(s[lo:hi].view(np.uint32))) == 1 and lo < 65536 < lo + topk - higher < hi
    assert s[:lo].max() < s[lo] and s[hi:n - higher].max() < s[lo] < s[n - higher:].min()
    out = ref.predict_ref(**c)
    want = np.r_[np.arange(n - higher, n), np.arange(lo, lo + topk - higher)]
    assert np.array_equal(out["query"], want)
    assert out["conf"][higher].tobytes() == out["conf"][-1].tobytes()
    assert not np.array_equal(out["masks"][-1], out["masks"][-2])
    # a select that compared the low 16 bits of the index would take the block from 65536 on
    low16 = np.lexsort((np.arange(n) & 0xffff, -s.astype(np.float64)))[:topk]
    assert set(low16.tolist()) != set(want.tolist()) and 65536 in low16[higher:higher + 1]


def test_the_large_scene_has_more_chunks_than_a_row_may_have():
    c = CASES["points_1048576"]
    n = len(c["superpoints"])
    assert n == 1048576 > 2048 * 256 and (n + 1 + 1023) // 1024 > 1024  # chunks of 1025; two passes of `points`
    out = ref.predict_ref(**c)
    assert list(out["counts"][0]) == [1, n] or list(out["counts"][1]) == [1, n]
    assert max(len(x) for x in out["counts"]) > 2 * 1024  # a run at most of the chunk boundaries


def test_a_one_point_instance_has_a_flat_box_and_an_empty_superpoint_gives_nothing():
    c = CASES["one_point_instance"]
    out = ref.predict_ref(**c)
    one = [r for r in range(len(out["conf"])) if out["npoints"][r] == 1]
    assert one and all(np.array_equal(out["box"][r, :3], out["box"][r, 3:]) for r in one)
    assert all(list(out["counts"][r]) == [11, 1] for r in one)
    assert 3 not in out["query"]  # query 3 sets a superpoint without points only: conf > 0, no point
    assert (np.asarray(out["npoints"]) > 0).all()


def test_negative_scores_sort_last_and_never_pass_a_zero_threshold():
    c = CASES["negative_scores_kept"]
    out = ref.predict_ref(**c)
    assert (out["conf"] < 0).any() and (np.diff(out["conf"]) <= 0).all()
    assert (ref.predict_ref(**CASES["negative_scores_dropped"])["conf"] > 0).all()
    cut = ref.predict_ref(**CASES["negative_scores_in_the_cut"])
    assert cut["stages"][0] == 20 and (cut["conf"] < 0).any()  # the cut runs through the negative scores


def test_refusals_and_their_precedence():
    seen = set()
    for name, case, status, flags in cases.refusals():
        out = ref.predict_ref(**case)
        assert (out["status"], out["flags"]) == (status, flags) and "conf" not in out, name
        seen.add(flags)
    assert {ref.FLAG_SCORE, ref.FLAG_MASK, ref.FLAG_COORDS, ref.FLAG_SPP} <= seen
    assert ref.status_of(ref.FLAG_SPP) == ref.ERR_SPP_RANGE and ref.status_of(ref.FLAG_SPP | ref.FLAG_COORDS) == -4
    bad, fine = cases.mask_refusal()
    assert ref.predict_ref(**bad)["flags"] == ref.FLAG_MASK and ref.predict_ref(**fine)["status"] == ref.OK


# ---- the ABI ---------------------------------------------------------------------------------------------------------
def test_abi_sizes_of_the_structs():
    from gapro_amd import _lib

    assert C.sizeof(_lib.SpfPredictInputs) == 72 and C.sizeof(_lib.SpfPredictParams) == 16
    assert C.sizeof(_lib.SpfPredictHeader) == 32 and _lib.SpfPredictHeader.total_runs.offset == 24
    assert _lib.SpfPredictInputs.superpoints_i64.offset == 64 and _lib.SpfPredictParams.score_thr.offset == 12


def _sizes(Q=400, C_=18, S=1500, N=200000, topk=100, npoint_thr=100, score_thr=0.0):
    from gapro_amd import _lib

    lib = _lib.load()
    inputs = _lib.SpfPredictInputs(n_queries=Q, n_spps=S, n_points=N)
    params = _lib.SpfPredictParams(num_class=C_, topk_insts=topk, npoint_thr=npoint_thr, score_thr=score_thr)
    return (int(lib.gapro_spf_predict_workspace_bytes(C.byref(inputs), C.byref(params))),
            int(lib.gapro_spf_predict_header_bytes(C.byref(inputs), C.byref(params))))


def test_workspace_and_header_sizes_and_the_refused_sizes():
    ws, hdr = _sizes()
    assert ws > 0 and ws % 256 == 0 and hdr == 32 + 4 * 100
    assert ws < 1 << 20  # nothing of size K x N: the chunk counts are the largest part
    assert _sizes(Q=5, C_=3)[1] == 32 + 4 * 15 and _sizes(topk=1024)[1] == 32 + 4 * 1024  # K = min(topk_insts, Q C)
    for bad in (dict(topk=0), dict(topk=1025), dict(npoint_thr=-1), dict(score_thr=float("nan")),
                dict(score_thr=float("-inf")), dict(Q=(1 << 20) // 18 + 1), dict(S=1 << 31), dict(N=1 << 31),
                dict(Q=0), dict(S=0), dict(N=0), dict(C_=0)):
        assert _sizes(**bad) == (0, 0), bad
    assert _sizes(npoint_thr=0)[0] > 0 and _sizes(S=(1 << 31) - 1, N=(1 << 31) - 1)[0] > 0


def test_the_functions_are_exported():
    import gapro_amd

    assert "spformer_predict" in gapro_amd.__all__ and "spformer_instances" in gapro_amd.__all__
