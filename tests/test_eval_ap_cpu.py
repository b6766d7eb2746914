"""ScanNet instance AP of pseudo-labels, host side (gapro_amd/eval_ap_ps_labels.py): the ABI of the AP table kernels,
and evaluate_matches / compute_averages (ap_from_tables) on tables tallied by the NumPy restatement in ap_tally.py,
against the reference ScanNetEval's numbers in tests/golden/ap_eval.npz.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ap_tally import fixture, fixture_scenes, tally
from gapro_amd import _lib
from gapro_amd import eval_ap_ps_labels as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(c, m) for c in ("golden", "synth") for m in ("one", "mean_prob")]
AVG_KEYS = ("all_ap", "all_ap_50%", "all_ap_25%", "all_rc", "all_rc_50%", "all_rc_25%")
CLASS_KEYS = ("ap", "ap50%", "ap25%", "rc", "rc50%", "rc25%")
NAMES = ("gapro_eval_ap_workspace_bytes", "gapro_eval_ap_keys", "gapro_eval_ap_pair_cells", "gapro_eval_ap_tables")


def test_ap_abi_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "gapro_hip.h")).read()
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name)
    assert "gapro_eval_ap_scene" in text
    assert C.sizeof(_lib.EvalApScene) == 8 + 8 + 4 + 4 + 4 * 8
    assert re.search(r"#define GAPRO_VERSION 200\b", text)


def test_ap_workspace_and_pair_layout():
    lib = _lib.load()
    d = (_lib.EvalApScene * 3)()
    for i, (n, p) in enumerate([(10, 4), (0, 1), (5, 900)]):
        d[i].point_offset, d[i].n_points, d[i].max_ps = 0, n, p
    words = (18 * 1000 + 31) // 32  # inst + 1 in [0, 1000) per class
    sizes = [-(-(words * 8 + p * 8) // 256) * 256 for p in (4, 1, 900)]
    assert lib.gapro_eval_ap_workspace_bytes(d, 3) == sum(sizes)
    assert [x.ws_offset for x in d] == [0, sizes[0], sizes[0] + sizes[1]]
    assert [x.id_offset for x in d] == [0, 4, 5]
    for x, k in zip(d, (3, 0, 17)):
        x.n_keys = k
    assert lib.gapro_eval_ap_pair_cells(d, 3) == 4 * 5 + 1 * 2 + 18 * 901
    assert [x.key_offset for x in d] == [0, 3, 3]
    assert [x.pair_offset for x in d] == [0, 20, 22]
    # bad arguments: 0
    assert lib.gapro_eval_ap_workspace_bytes(d, 0) == 0
    assert lib.gapro_eval_ap_workspace_bytes(None, 3) == 0
    d[2].n_keys = 18 * 1000 + 1
    assert lib.gapro_eval_ap_pair_cells(d, 3) == 0
    d[1].max_ps = 0
    assert lib.gapro_eval_ap_workspace_bytes(d, 3) == 0
    d[1].max_ps, d[1].n_points = 1, -1
    assert lib.gapro_eval_ap_workspace_bytes(d, 3) == 0


def _check(res, z, key):
    np.testing.assert_allclose(res.ap, z[key + "_ap"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(res.rc, z[key + "_rc"], rtol=0, atol=1e-12)
    got = np.array([res.avgs[k] for k in AVG_KEYS])
    np.testing.assert_allclose(got, z[key + "_avg"], rtol=0, atol=1e-12)
    cls = np.array([[res.avgs["classes"][c][k] for k in CLASS_KEYS] for c in A.CLASSES])
    np.testing.assert_allclose(cls, z[key + "_cls"], rtol=0, atol=1e-12)  # NaN where the reference has NaN


@pytest.mark.parametrize("case,conf", CASES)
def test_ap_from_tables_reproduces_the_reference(case, conf):
    z = fixture()
    tables = [tally(*sc, confidence=conf) for sc in fixture_scenes(case)]
    res = A.ap_from_tables(tables)
    _check(res, z, "%s_%s" % (case, conf))
    assert np.isnan(res.ap[res.n_gt == 0]).all() and not np.isnan(res.ap[res.n_gt > 0]).any()
    if case == "golden" and conf == "one":
        assert [round(res.avgs[k], 3) for k in AVG_KEYS[:3]] == [0.736, 0.891, 1.0]


def test_synthetic_fixture_reaches_the_branches():
    """The synthetic case has a class with GT and no prediction (AP 0), classes with neither (NaN), duplicates at
    IoU 0.25 and predictions under and over min_region_size."""
    z = fixture()
    tables = [tally(*sc) for sc in fixture_scenes("synth")]
    res = A.ap_from_tables(tables)
    assert (res.n_gt > 0).any() and ((res.n_gt > 0) & (res.n_pred == 0)).any()
    assert ((res.n_gt == 0) & (res.n_pred == 0)).any()
    assert (res.ap[(res.n_gt > 0) & (res.n_pred == 0)] == 0).all()
    branch = tables[0]
    assert (branch.pred_n < 100).any() and (branch.gt_n < 100).any() and (branch.pred_void > 0).any()
    assert (branch.gt_code % 1000 == 0).any()  # a GT instance id of -1
    assert len(set((branch.gt_code % 1000).tolist())) < len(branch.gt_code)  # one id on two classes
    assert np.isnan(z["synth_one_avg"]).sum() == 0


@pytest.mark.parametrize("case,conf", CASES)
def test_ap_does_not_depend_on_scene_order(case, conf):
    tables = [tally(*sc, confidence=conf) for sc in fixture_scenes(case)]
    ref = A.ap_from_tables(tables)
    rng = np.random.default_rng(7)
    for _ in range(3):
        got = A.ap_from_tables([tables[i] for i in rng.permutation(len(tables))])
        np.testing.assert_array_equal(got.ap, ref.ap)
        np.testing.assert_array_equal(got.rc, ref.rc)
        np.testing.assert_array_equal(got.n_gt, ref.n_gt)


def test_mean_prob_confidence_formula():
    sc = fixture_scenes("synth")[1]
    t = tally(*sc, confidence="mean_prob")
    ps, prob = np.asarray(sc[3]), np.asarray(sc[4])
    for u, c in zip(t.pred_id, t.pred_conf):
        idx = np.flatnonzero(ps == u)
        s = int(sum(int(np.rint(float(p) * 2 ** 32)) for p in prob[idx]))
        assert c == float(s) / (float(len(idx)) * 2.0 ** 32)
        assert abs(c - prob[idx].astype(np.float64).mean()) < 1e-9


def test_min_region_size_and_empty_input():
    tables = [tally(*sc) for sc in fixture_scenes("synth")]
    loose = A.ap_from_tables(tables, min_region_size=1)
    strict = A.ap_from_tables(tables, min_region_size=100)
    assert (loose.n_gt >= strict.n_gt).all() and (loose.n_pred >= strict.n_pred).all()
    assert (loose.n_gt > strict.n_gt).any()
    empty = A.ap_from_tables([])
    assert np.isnan(empty.ap).all() and np.isnan(empty.avgs["all_ap"])


def test_results_table_and_argument_errors():
    tables = [tally(*sc) for sc in fixture_scenes("golden")]
    text = A.format_results(A.ap_from_tables(tables).avgs)
    lines = text.split("\n")
    assert lines[1] == "#" * 64 and lines[2].startswith("what           :      AP  AP_50%")
    assert len(lines) == 1 + 3 + 18 + 1 + 1 + 2
    assert lines[-3].startswith("average        :   0.736   0.891   1.000")
    n = np.zeros(4, dtype=np.int64)
    with pytest.raises(ValueError, match="confidence"):
        A.ap_tables([(n, n, n, n)], confidence="max", device="cuda:0")
    with pytest.raises(ValueError, match="ps_prob"):
        A.ap_tables([(n, n, n, n)], confidence="mean_prob", device="cuda:0")
    with pytest.raises(ValueError, match="length"):
        A.ap_tables([(n, n, n[:3], n[:3])], device="cuda:0")
    with pytest.raises(ValueError, match="no scene"):
        A.ap_tables([], device="cuda:0")
    with pytest.raises(SystemExit):
        A.main(["--confidence", "max"])


def _edge_fixture():
    """tests/golden/ap_eval_edges.npz: two scenes with a value ON every comparison of evaluate_matches, and the reference
    ScanNetEval's numbers on them."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "ap_eval_edges.npz"))
    return z, [[z["edges%d_%s" % (i, k)] for k in ("sem_gt", "inst_gt", "ps_sem", "ps_inst", "prob")]
               for i in range(int(z["n_edges"]))]


@pytest.mark.parametrize("conf", ["one", "mean_prob"])
def test_ap_from_tables_reproduces_the_reference_on_the_threshold_edges(conf):
    """iou > th, prop_ignore <= th and >= min_region_size with values on the comparison: IoUs of exactly 0.5 and 0.25,
    instances of 99 and 100 points, ignored shares of exactly 0.5 and 0.25."""
    z, scenes = _edge_fixture()
    tables = [tally(*sc, confidence=conf) for sc in scenes]
    _check(A.ap_from_tables(tables), z, "edges_%s" % conf)
    for t in tables:  # the fixture holds what it was built for
        iou = t.pair_inter / (t.gt_n[t.pair_gt] + t.pred_n[t.pair_pred] - t.pair_inter)
        assert (iou == 0.5).sum() >= 5 and (iou == 0.25).sum() >= 1 and 100 in t.pred_n[t.pair_pred[iou == 0.25]]
        assert {99, 100} <= set(t.gt_n.tolist()) and {99, 100} <= set(t.pred_n.tolist())
        small = np.bincount(t.pair_pred[t.gt_n[t.pair_gt] < 100], t.pair_inter[t.gt_n[t.pair_gt] < 100], len(t.pred_n))
        share = (t.pred_void + small) / t.pred_n
        assert (share[t.pred_void > 0] == 0.5).any() and (share[t.pred_void > 0] == 0.25).any()
        assert (share[(t.pred_void == 0) & (t.pred_n >= 100)] == 0.5).any()   # ignored through a 60-point GT alone
        assert 18999 in t.gt_code and 18000 in t.gt_code
