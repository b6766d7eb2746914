"""The two pseudo-label evaluators at their kernel and table edges (gapro_amd/csrc/eval_batch.hip behind evaluate_scenes,
get_miou_scene and get_scene_sem_conf; eval_ap.hip behind ap_tables): every named case of eval_cases.py against its plain
NumPy reference, BIT FOR BIT, dtypes included -- integers and float32 / float64 in a fixed order leave no tolerance.
test_eval_edges_cpu.py proves that each case is what it claims and can tell the mistake it was built for."""
import numpy as np
import pytest

import eval_cases as ec

pytestmark = pytest.mark.gpu

ALL_EVAL = list(ec.IOU_CASES) + list(ec.CONF_CASES)
COMMON_TAUS = (0.8, 0.4, 0.8, 0.5)   # of the invariance batches: unsorted, one of them twice


def _assert_rows(res, i, rows, what):
    assert len(res.ious[i]) == len(rows), what
    for r, row in enumerate(rows):
        got = res.ious[i][r]
        assert got.dtype == np.float32 and got.shape == row.ious.shape, (what, r)
        np.testing.assert_array_equal(got.view(np.uint32), row.ious.view(np.uint32), err_msg="%s row %d" % (what, r))
        assert res.kept[i, r] == row.kept, (what, r)


def _conf_sum(all_rows, C):
    out = np.zeros((len(all_rows[0]), C, C), np.int64)
    for rows in all_rows:
        for r, row in enumerate(rows):
            out[r] += row.conf
    return out


def _run(case, scenes=None, taus=None):
    from gapro_amd.eval_ps_labels import evaluate_scenes

    scenes = case.scenes if scenes is None else scenes
    return evaluate_scenes([ec.writable(sc) for sc in scenes], prob_thresholds=case.thresholds if taus is None else taus,
                           scannet_remap=case.remap, num_classes=case.num_classes)


def _assert_result(res, want, C, what):
    for i, rows in enumerate(want):
        _assert_rows(res, i, rows, "%s scene %d" % (what, i))
    assert res.conf.dtype == np.int64 and res.kept.dtype == np.int64
    np.testing.assert_array_equal(res.conf, _conf_sum(want, C), err_msg=what)


def _same(a, b, i, j):
    """Scene i of result a and scene j of result b, bit for bit."""
    assert len(a.ious[i]) == len(b.ious[j])
    for x, y in zip(a.ious[i], b.ious[j]):
        np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))
    assert np.array_equal(a.kept[i], b.kept[j])


# ------------------------------------------------------------------------------------------ eval_batch
@pytest.mark.parametrize("name", ALL_EVAL)
def test_evaluate_scenes_equals_the_reference(name):
    case = ec.eval_case(name)
    _assert_result(_run(case), ec.eval_expected(name), case.num_classes, name)


@pytest.mark.parametrize("name", ALL_EVAL)
def test_per_scene_functions_equal_the_reference(name):
    """get_miou_scene and get_scene_sem_conf on every row's points, filtered beforehand (one-scene batches without
    thresholds); GT labels of a case without the remap go in as they are, fractions included."""
    import torch
    from gapro_amd.eval_ps_labels import get_miou_scene, get_scene_sem_conf

    case = ec.eval_case(name)
    for sc, rows in zip(case.scenes, ec.eval_expected(name)):
        n = len(sc["semantic_label"])
        masks = [np.ones(n, bool)] + [ec.keep_mask(sc["ps_prob"], t) for t in case.thresholds]
        sem = ec.remap_sem(ec.to_int(sc["semantic_label"])) if case.remap else sc["semantic_label"]
        for m, row in zip(masks, rows):
            args = [np.ascontiguousarray(a[m]) for a in (sem, sc["instance_label"], sc["ps_semantic_label"],
                                                          sc["ps_instance_label"])]
            ious = get_miou_scene(*args)
            conf = get_scene_sem_conf(args[0], args[2], num_classes=case.num_classes)
            assert ious.dtype == torch.float32 and conf.dtype == torch.int64 and ious.is_cuda and conf.is_cuda
            np.testing.assert_array_equal(ious.cpu().numpy().view(np.uint32), row.ious.view(np.uint32))
            np.testing.assert_array_equal(conf.cpu().numpy(), row.conf)


def test_size_ladder_batch_equals_its_single_scenes():
    case = ec.eval_case("size_ladder")
    whole = _run(case)
    conf = np.zeros_like(whole.conf)
    for i, sc in enumerate(case.scenes):
        one = _run(case, [sc])
        _same(one, whole, 0, i)
        conf += one.conf
    np.testing.assert_array_equal(conf, whole.conf)


@pytest.mark.parametrize("a,b", [("pair_8192", "pair_8256"), ("pair_b2_4096", "pair_b2_over"), ("c19_k4", "c19_k5")])
def test_both_sides_of_a_table_switch_agree(a, b):
    """The same points with the tables in LDS and in global memory; c19_k5's first five rows are c19_k4's."""
    ra, rb = _run(ec.eval_case(a)), _run(ec.eval_case(b))
    rows = len(ra.ious[0])
    for r in range(rows):
        np.testing.assert_array_equal(ra.ious[0][r].view(np.uint32), rb.ious[0][r].view(np.uint32))
    np.testing.assert_array_equal(ra.conf, rb.conf[:rows])
    np.testing.assert_array_equal(ra.kept, rb.kept[:, :rows])


def test_equal_thresholds_give_equal_rows():
    res = _run(ec.eval_case("thr_equal"))
    for r in (2, 4):
        np.testing.assert_array_equal(res.ious[0][1].view(np.uint32), res.ious[0][r].view(np.uint32))
        np.testing.assert_array_equal(res.conf[1], res.conf[r])
        assert res.kept[0, 1] == res.kept[0, r]
    assert res.kept[0, 3] > res.kept[0, 1]


def test_threshold_and_class_count_limits_are_refused():
    import torch
    from gapro_amd._lib import GaproError
    from gapro_amd.eval_ps_labels import evaluate_scenes, get_scene_sem_conf

    sc = ec.writable(ec.eval_case("thr_max").scenes[0])
    with pytest.raises(ValueError, match="at most 32"):
        evaluate_scenes([sc], prob_thresholds=ec.THR_MAX_TAUS + (0.99,))
    c128 = ec.eval_case("classes_128").scenes[0]
    with pytest.raises(GaproError, match="gapro_eval_batch: bad argument"):
        get_scene_sem_conf(c128["semantic_label"].copy(), c128["ps_semantic_label"].copy(), num_classes=129)
    torch.cuda.synchronize()
    got = get_scene_sem_conf(c128["semantic_label"].copy(), c128["ps_semantic_label"].copy(), num_classes=128)
    np.testing.assert_array_equal(got.cpu().numpy(), ec.eval_expected("classes_128")[0][0].conf)


def test_eval_batch_composition_does_not_change_a_bit():
    """All scenes of the family that the 19-class remapped confusion is defined on, in one batch, reversed, and alone,
    under thresholds of the batch's own; against the reference too."""
    names = [n for n in ALL_EVAL if ec.eval_case(n).num_classes == 19]
    scenes = [sc for n in names for sc in ec.eval_case(n).scenes]
    assert len(scenes) > 25 and all(ec.conf_in_range(*(ec.scene_ints(sc, 1)[k] for k in (0, 2)), 19) for sc in scenes)
    case = ec.EvalCase("batch", scenes, COMMON_TAUS, True, 19, {})
    want = [ec.rows_reference(sc, COMMON_TAUS) for sc in scenes]
    whole = _run(case)
    _assert_result(whole, want, 19, "batch")
    rev = _run(case, scenes[::-1])
    np.testing.assert_array_equal(rev.conf, whole.conf)
    conf = np.zeros_like(whole.conf)
    for i, sc in enumerate(scenes):
        _same(rev, whole, len(scenes) - 1 - i, i)
        one = _run(case, [sc])
        _same(one, whole, 0, i)
        conf += one.conf
    np.testing.assert_array_equal(conf, whole.conf)


# ------------------------------------------------------------------------------------------ eval_ap
def _tables(scenes, confidence, remap=True):
    from gapro_amd.eval_ap_ps_labels import ap_tables

    return ap_tables([ec.writable(sc) for sc in scenes], confidence, scannet_remap=remap)


def _assert_tables(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        for f in ec.ApRef._fields:
            x, y = np.asarray(getattr(g, f)), np.asarray(getattr(w, f))
            assert x.dtype == y.dtype and x.shape == y.shape, (what, i, f)
            np.testing.assert_array_equal(x, y, err_msg="%s scene %d %s" % (what, i, f))


@pytest.mark.parametrize("name", list(ec.AP_CASES))
def test_ap_tables_equal_the_reference(name):
    case = ec.ap_case(name)
    _assert_tables(_tables(case.scenes, case.confidence, case.remap), ec.ap_expected(name), name)
    other = "one" if case.confidence == "mean_prob" else "mean_prob"
    want = [ec.ap_scene_reference(sc, other, case.remap) for sc in case.scenes]
    _assert_tables(_tables(case.scenes, other, case.remap), want, name + " " + other)


@pytest.mark.parametrize("gt_dt", ec.GT_DTYPES)
@pytest.mark.parametrize("ps_dt", [np.int32, np.int64])
@pytest.mark.parametrize("name", list(ec.AP_DTYPE_CASES))
def test_ap_label_dtypes(name, gt_dt, ps_dt):
    case = ec.ap_case(name, gt_dt)
    scenes = []
    for sc in case.scenes:
        sc = ec.writable(sc)
        sc["ps_semantic_label"] = sc["ps_semantic_label"].astype(ps_dt)
        sc["ps_instance_label"] = sc["ps_instance_label"].astype(ps_dt)
        scenes.append(sc)
    _assert_tables(_tables(scenes, case.confidence, case.remap), ec.ap_expected(name), name)


def test_ap_wide_max_ps_equals_the_default_size():
    case = ec.ap_case("wide_max_ps")
    _assert_tables(_tables(case.scenes, "mean_prob"), _tables(case.meta["default"], "mean_prob"), "wide_max_ps")


def test_ap_prob_grid_confidence_is_exact():
    case = ec.ap_case("prob_grid")
    sc = case.scenes[0]
    t = _tables(case.scenes, "mean_prob")[0]
    for u, c, n in zip(t.pred_id, t.pred_conf, t.pred_n):
        idx = np.flatnonzero(sc["ps_instance_label"] == u)
        s = sum(int(np.rint(float(p) * 2.0 ** 32)) for p in sc["ps_prob"][idx])
        assert n == len(idx) and c == np.float64(s) / (np.float64(len(idx)) * 2.0 ** 32)


@pytest.mark.parametrize("name", list(ec.AP_REFUSALS))
def test_ap_refusals_name_the_scene_and_leave_the_rest_right(name):
    """Range-checked before any table is addressed (eval_ap.hip:62,177,183): the scene is named alone, and the same call
    without it gives the right tables."""
    import torch

    good, bad, good2 = ec.refusal_scenes(name)
    with pytest.raises(ValueError, match=r"scene\(s\) \[1\]"):
        _tables([good, bad, good2], "mean_prob")
    torch.cuda.synchronize()
    want = [ec.ap_scene_reference(sc, "mean_prob", True) for sc in (good, good2)]
    _assert_tables(_tables([good, good2], "mean_prob"), want, name)


def test_ap_batch_composition_does_not_change_a_bit():
    """Every scene of the family in one batch (all four table placements, every ladder size, three GT dtypes), reversed,
    and alone."""
    scenes = [sc for n in ec.AP_CASES for sc in ec.ap_case(n).scenes]
    scenes += [sc for n in ec.AP_DTYPE_CASES for dt in (np.int32, np.int64) for sc in ec.ap_case(n, dt).scenes]
    want = [ec.ap_scene_reference(sc, "mean_prob", True) for sc in scenes]
    whole = _tables(scenes, "mean_prob")
    _assert_tables(whole, want, "batch")
    _assert_tables(_tables(scenes[::-1], "mean_prob")[::-1], want, "reversed")
    for i, sc in enumerate(scenes):
        _assert_tables(_tables([sc], "mean_prob"), [want[i]], "alone %d" % i)
