"""The inputs of test_labeler_edges_gpu.py really are what labeler_cases.py claims (no device): the literal per-point
reference agrees with oracle/labeler_oracle.py -- which the goldens pin to the real reference -- on every case, and every
case decides what it was built to decide.  getInstanceInfo's host forms (NumPy and native) against the oracle's loop."""
import numpy as np
import pytest

import labeler_cases as lc


# ------------------------------------------------------------------------------------------ literal == oracle
@pytest.mark.parametrize("name", lc.LABELER_CASE_NAMES)
def test_literal_reference_agrees_with_the_oracle(name):
    case, lit, ref = lc.labeler_case(name), lc.literal(name), lc.oracle_labels(name)
    for labeler in case.labelers:
        for ds in lc.DATASETS:
            sem, inst = lit.labels(labeler, ds)
            np.testing.assert_array_equal(sem, ref[labeler, ds][0], err_msg="%s %s sem" % (labeler, ds))
            np.testing.assert_array_equal(inst, ref[labeler, ds][1], err_msg="%s %s inst" % (labeler, ds))


# ------------------------------------------------------------------------------------------ each case is what it claims
@pytest.mark.parametrize("n_boxes", lc.MANY_BOXES)
def test_many_box_cases_reach_past_the_first_word_and_tie_on_volume(n_boxes):
    name = "boxes_%d" % n_boxes
    case, lit = lc.labeler_case(name), lc.literal(name)
    assert len(case.box) == n_boxes and (n_boxes + 63) // 64 == {63: 1, 64: 1, 65: 2, 128: 2, 129: 3, 255: 4, 256: 4}[n_boxes]
    vol = np.array(lit.raw("volume"))
    dist = np.array(lit.raw("dist"))
    # equal minimal volumes: the strict '<' decides
    ties = sum(1 for i in lit.multi if sum(1 for b in lit.inside[i] if lit.vol[b] == lit.vol[vol[i]]) > 1)
    assert ties >= 100
    assert all(vol[i] == min(b for b in lit.inside[i] if lit.vol[b] == lit.vol[vol[i]]) for i in lit.multi)
    assert (vol != dist).sum() >= 1000
    last = n_boxes - 1
    assert any(last in boxes for boxes in lit.inside)  # the last bit of the last word is set somewhere
    if n_boxes >= 65:
        assert (vol >= 64).sum() > 0 and (dist >= 64).sum() > 0
        for ds in lc.DATASETS:  # and survive the superpoint vote
            assert (lc.oracle_labels(name)["volume", ds][1] >= 64).any()
            assert (lc.oracle_labels(name)["dist", ds][1] >= 64).any()
    if n_boxes in (129, 256):
        assert (vol >= 64).sum() > 1000 and (dist >= 64).sum() > 1000
    none = np.array(lit.raw("none"))
    if n_boxes == 256:
        assert len(lit.multi) == lit.n and (none == -2).all()
    if n_boxes in (65, 129):  # "none" still labels points
        assert (none >= 0).sum() >= 50
        assert (lc.oracle_labels(name)["none", "other"][1] >= 0).sum() == (none >= 0).sum()


@pytest.mark.parametrize("name", ["rank_scan", "rank_scan_single_head", "rank_scan_n1", "rank_scan_n63",
                                  "rank_scan_n257"])
def test_rank_scan_cases_force_their_indices_and_see_the_indexing_quirk(name):
    case, lit = lc.labeler_case(name), lc.literal(name)
    multi = np.zeros(lit.n, bool)
    multi[lit.multi] = True
    np.testing.assert_array_equal(multi, case.meta["multi"])  # multi-box exactly where the builder chose
    assert case.meta["forced"] and all(multi[i] for i in case.meta["forced"])
    assert any(len(b) == 3 for b in lit.inside) or lit.n < 63
    rank = np.cumsum(multi) - multi  # rank of every multi-box point
    if case.meta["single_head"]:
        assert not multi[:300].any() and not (rank[multi] == np.flatnonzero(multi)).any()
    if lit.n == lc.RANK_N:
        assert lit.n == 2 * lc.LAB_CHUNK + 300
        assert all(multi[c * lc.LAB_CHUNK:(c + 1) * lc.LAB_CHUNK].any() for c in range(3))
        # every lane, wave and sub-block position of the scan holds a multi-box point somewhere
        pos = np.flatnonzero(multi)
        assert len(set(pos % 64)) == 64 and len(set(pos // 64 % 4)) == 4 and len(set(pos // 256 % 8)) == 8
        by_rank, by_own = np.array(lit.raw("dist")), np.array(lit.raw("dist", own_coords=True))
        assert (by_rank != by_own).sum() >= 100
        for ds in lc.DATASETS:  # and the library's answer must be the by-rank one
            own = lit.labels("dist", ds, own_coords=True)[1]
            assert (own != lc.oracle_labels(name)["dist", ds][1]).sum() >= (100 if ds == "other" else 1)


def test_mirrored_centres_tie_in_the_reference_and_not_under_contraction():
    case, lit = lc.labeler_case("mirrored_centres"), lc.literal("mirrored_centres")
    pair_of_point = case.meta["pair_of_point"]
    n = len(pair_of_point)
    assert n == 3 * lc.MIRROR_POINTS and lit.multi[:n] == list(range(n))  # rank k = index k
    dist = lit.raw("dist")
    later = {order: [0, 0, 0] for order in ((1, 0, 2), (0, 1, 2))}  # fma(z, fma(x, RN(y^2))), fma(z, fma(y, RN(x^2)))
    for i in range(n):
        pair = int(pair_of_point[i])
        first, second = 2 * pair, 2 * pair + 1
        assert lit.inside[i] == [first, second]
        p = lit.points[i]
        assert lc.sqdist_reference(p, lit.centre[first]) == lc.sqdist_reference(p, lit.centre[second])
        assert dist[i] == first
        for order in later:
            later[order][pair] += lc.sqdist_fused(p, lit.centre[second], order) < lc.sqdist_fused(p, lit.centre[first], order)
    for order, counts in later.items():
        assert min(counts) >= 10, (order, counts)
    # the emulation is the reference's arithmetic when nothing is fused: exact squares, rounded, then summed
    for i in range(0, n, 7):
        p, c = lit.points[i], lit.centre[0]
        sq = [float(lc.Fraction(p[k] - c[k]) ** 2) for k in range(3)]
        assert (sq[0] + sq[1]) + sq[2] == lc.sqdist_reference(p, c)
    assert case.vol[0] == case.vol[1] and all(lit.raw("volume")[i] == 2 * int(pair_of_point[i]) for i in range(n))


@pytest.mark.parametrize("variant", ["neg", "big"])
def test_mask_case_differs_from_box2mask_exactly_below_the_threshold(variant):
    name = "mask_%s_ids" % variant
    case, lit, ref = lc.labeler_case(name), lc.literal(name), lc.oracle_labels(name)
    ids = case.meta["ids"]
    assert sorted(np.unique(case.spp)) == sorted(ids) and max(ids) - min(ids) < (1 << 20)
    assert (min(ids) < 0) if variant == "neg" else (min(ids) > (1 << 31))
    groups, mask = lit.members(), lit.occupancy_mask()
    for sid, (n, k) in zip(ids, lc.MASK_SPPS):
        assert len(groups[sid]) == n and sum(1 for i in groups[sid] if lit.inside[i] == [2]) == k
        assert sum(1 for i in groups[sid] if lit.inside[i]) == k
        assert mask[sid][2] == (np.float32(k) / np.float32(n) >= np.float32(0.7)) == (10 * k >= 7 * n)
    assert np.float32(7) / np.float32(10) == np.float32(0.7) == np.float32(70) / np.float32(100)  # exactly at it
    below = {sid for sid, (n, k) in zip(ids, lc.MASK_SPPS) if (n, k) in ((10, 6), (100, 69))}
    assert len(below) == 2
    for rule in ("volume", "dist", "none"):
        differ = ref[rule, "scannetv2"][1] != ref["box2mask", "scannetv2"][1]
        assert set(case.spp[differ]) == below and differ.sum() == 110
        np.testing.assert_array_equal(ref[rule, "other"][1], ref["box2mask", "other"][1])


def test_vote_tie_superpoints_have_equal_leading_counts():
    case, lit, ref = lc.labeler_case("vote_ties"), lc.literal("vote_ties"), lc.oracle_labels("vote_ties")
    assert lit.multi[:10] == list(range(10)) and all(lit.inside[i] == [lc.TIE_A, lc.TIE_B] for i in range(10))
    mask = lit.occupancy_mask()
    assert mask[100][lc.TIE_A] and mask[100][lc.TIE_B]
    seen = 0
    for labeler, ties in case.meta["ties"].items():
        counts = lit.label_counts(lit.raw(labeler))
        for sid, (first, second, winner) in ties.items():
            c = counts[sid]
            assert c[first + 1] == c[second + 1] == 5 and sum(c) == 10 and first < second
            got = set(ref[labeler, "scannetv2"][1][case.spp == sid])
            assert got == {winner if winner >= 0 else -100}
            if winner < 0:
                assert set(ref[labeler, "scannetv2"][0][case.spp == sid]) == {18}  # background, not "ignore"
            seen += 1
    assert seen == 4
    assert any(b >= 64 for boxes in lit.inside for b in boxes)  # box 70: a count row in the second word


def test_face_probes_sit_on_the_float32_faces():
    case, lit = lc.labeler_case("faces"), lc.literal("faces")
    kind = case.meta["kind"]
    assert len(kind) == 18
    f64_inside = []
    for i, k in enumerate(kind):
        inside = lc.FACE_BOX in lit.inside[i]
        if k == "on":
            assert inside
        elif k == "beyond":
            assert not inside
        else:
            f64_inside.append(inside)
        assert all(b == lc.FACE_BOX for b in lit.inside[i])
    # the float64 margin would hold every "f64" probe; the float32 margin must drop some and keep some
    assert len(f64_inside) == 6 and any(f64_inside) and not all(f64_inside)
    assert lit.inside[case.meta["inverted_point"]] == [] and not any(0 in b for b in lit.inside)
    plate = [lit.inside[i] for i in case.meta["plate_points"]]
    assert plate == [[1, 4]] * 5 + [[4]] and case.vol[1] == 0 and case.vol[0] < 0
    assert all(lit.raw("volume")[i] == 1 for i in case.meta["plate_points"][:5])
    sem = set(lc.oracle_labels("faces")["volume", "other"][0])
    assert {0, 17, -100, 2 ** 31 - 1} <= sem


def test_grid_stride_case_wraps_every_point_kernel():
    case, lit = lc.labeler_case("grid_stride"), lc.literal("grid_stride")
    assert lit.n == lc.LAB_GRID_POINTS + 300 and len(case.box) == 3 and case.labelers == ("volume", "dist")
    assert 1900 <= len(np.unique(case.spp)) <= 2100
    tail = range(lc.LAB_GRID_POINTS, lit.n)  # the points of the second sweep: every kind among them
    assert {min(len(lit.inside[i]), 2) for i in tail} == {0, 1, 2}
    assert len(lit.multi) > 100000 and (np.array(lit.raw("volume")) != np.array(lit.raw("dist"))).sum() > 10000


# ------------------------------------------------------------------------------------------ getInstanceInfo on the host
def _assert_info_equal(got, ref, corners):
    assert got[0] == ref[0]
    for a, b in zip(got[1:4], ref[1:4]):
        assert np.asarray(a).dtype == np.float64
        np.testing.assert_array_equal(a, b)
    if corners:
        assert got[4].dtype == np.float32
        np.testing.assert_array_equal(got[4], ref[4])
    else:
        assert got[4] is None


@pytest.mark.parametrize("dataset_name", ["scannetv2", "other"])
@pytest.mark.parametrize("name", lc.INSTANCE_CASE_NAMES)
def test_instance_info_host_forms_match_the_oracle(name, dataset_name):
    from gapro_amd.gen_ps_utils import getInstanceInfo, getInstanceInfo_native

    case = lc.instance_case(name)
    ref = lc.oracle_instance_info(name, dataset_name == "scannetv2")
    with np.errstate(over="ignore", under="ignore"):
        host = getInstanceInfo(case.xyz, case.inst, case.sem, dataset_name=dataset_name)
    _assert_info_equal(host, ref, corners=True)
    _assert_info_equal(getInstanceInfo_native(case.xyz, case.inst, case.sem, dataset_name=dataset_name), ref, corners=False)


def test_instance_cases_are_what_they_claim():
    ids = {name: set(np.unique(lc.instance_case(name).inst)) for name in lc.INSTANCE_CASE_NAMES}
    edges = {lc.INST_LDS_IDS - 1, lc.INST_LDS_IDS, lc.INST_FIRST_CAP - 1}
    assert edges <= ids["id_edges"] and max(ids["id_edges"]) == lc.INST_FIRST_CAP - 1 and {-100.0, -1.0} <= ids["id_edges"]
    assert edges | {lc.INST_FIRST_CAP, lc.INST_FIRST_CAP + 1, 3001} <= ids["id_edges_regrow"]
    assert 3002 % 256 != 0 and 2048 % 256 == 0  # the regrown table: finalize's id ranges end unevenly
    assert ids["dense_1101"] == set(map(float, range(1101))) and len(lc.oracle_instance_info("dense_1101", True)[1]) == 1101
    single = lc.instance_case("singletons")
    counts = {i: int((single.inst == i).sum()) for i in ids["singletons"]}
    assert [counts[i] for i in (1.0, 7.0, 600.0)] == [1, 1, 1] and counts[0.0] == 2000 and counts[601.0] == 500
    np.testing.assert_array_equal(lc.oracle_instance_info("singletons", True)[3][[1, 3, 4]], 0.0)
    signs = lc.instance_case("signs")
    assert (signs.xyz[signs.inst == 0] < 0).all()
    mixed = signs.xyz[signs.inst == 1]
    assert (mixed < 0).any(axis=0).all() and (mixed > 0).any(axis=0).all()
    for i in (2, 3):
        z = signs.xyz[signs.inst == i]
        assert ((z == 0) & np.signbit(z)).any(axis=0).all() and ((z == 0) & ~np.signbit(z)).any(axis=0).all()
    mag = np.abs(lc.instance_case("magnitudes").xyz)
    assert np.isfinite(mag).all() and ((mag > 0) & (mag < 2.2250738585072014e-308)).any()
    assert mag.max() <= 1e100 and mag.max() > 1e99 and ((mag >= 1e-300) & (mag < 1e-200)).any()
    assert np.isfinite(lc.oracle_instance_info("magnitudes", True)[3]).all()
    shift = lc.instance_case("class_shift")
    assert shift.sem[np.flatnonzero(shift.inst == 0)[0]] == -100 and shift.sem[np.flatnonzero(shift.inst == 2)[0]] == 2
    on, off = lc.oracle_instance_info("class_shift", True)[1], lc.oracle_instance_info("class_shift", False)[1]
    np.testing.assert_array_equal(on[:3], [-100.0, 0.0, -100.0])
    np.testing.assert_array_equal(off[:3], [-100.0, 2.0, -100.0])
    big = lc.instance_case("corner_grid_stride")
    assert len(big.inst) == lc.CORNER_GRID_POINTS + 77 and len(ids["corner_grid_stride"] - {-100.0}) == 30
    assert (big.inst[lc.CORNER_GRID_POINTS:] >= 0).any() and (big.inst[lc.CORNER_GRID_POINTS:] < 0).any()
