"""Probability-threshold rows of the AP evaluator, host side (gapro_amd/eval_ap_ps_labels.py): the step from a row of
the kernels' arrays to its ApTable, the per-row AP, the nesting of the rows, the refusals and the CLI's arguments.  The
reference of a row is ap_tally.tally on the arrays filtered with NumPy's float32 ``prob >= tau``; everything is
integer-exact.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ap_rows_cases import filtered, kept_mask, own_thresholds, random_scene, raw_row
from ap_tally import assert_tables_equal, fixture_scenes, tally
from gapro_amd import _lib
from gapro_amd import eval_ap_ps_labels as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gapro_eval_ap_workspace_bytes_rows", "gapro_eval_ap_tables_rows")


def _equal_results(a, b):
    np.testing.assert_array_equal(a.ap, b.ap)  # NaN == NaN here
    np.testing.assert_array_equal(a.rc, b.rc)
    np.testing.assert_array_equal(a.n_gt, b.n_gt)
    np.testing.assert_array_equal(a.n_pred, b.n_pred)
    for k, v in a.avgs.items():
        if k != "classes":
            np.testing.assert_array_equal(v, b.avgs[k])


def test_rows_abi_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "gapro_hip.h")).read()
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert re.search(r"#define GAPRO_VERSION 200\b", text)
    # the old signatures stand, and the new pass 2 is the old one plus (n_thresholds, h_thresholds) behind d_prob
    old, new = _lib.SIGNATURES["gapro_eval_ap_tables"][1], _lib.SIGNATURES["gapro_eval_ap_tables_rows"][1]
    assert len(old) == 26 and new == old[:15] + [C.c_int32, C.c_void_p] + old[15:]


def test_rows_workspace_is_the_plain_one_plus_first_point_rows():
    lib = _lib.load()
    d = (_lib.EvalApScene * 3)()
    for i, (n, p) in enumerate([(10, 4), (0, 1), (5, 900)]):
        d[i].point_offset, d[i].n_points, d[i].max_ps = 0, n, p
    base = lib.gapro_eval_ap_workspace_bytes(d, 3)
    layout = [(x.ws_offset, x.id_offset) for x in d]
    assert base > 0 and base % 256 == 0
    for T in (0, 1, 2, 32):
        for x in d:
            x.ws_offset = x.id_offset = -1
        assert lib.gapro_eval_ap_workspace_bytes_rows(d, 3, T) == base + T * 905 * 8
        assert [(x.ws_offset, x.id_offset) for x in d] == layout  # the layout gapro_eval_ap_keys checks
    assert lib.gapro_eval_ap_workspace_bytes_rows(d, 3, 33) == 0
    assert lib.gapro_eval_ap_workspace_bytes_rows(d, 3, -1) == 0
    assert lib.gapro_eval_ap_workspace_bytes_rows(None, 3, 1) == 0
    d[1].max_ps = 0
    assert lib.gapro_eval_ap_workspace_bytes_rows(d, 3, 1) == 0


def test_table_from_raw_on_a_hand_built_row():
    """Three keys of the scene, one without a point in the row; four ids: one without a point, one whose first kept
    point has no class.  Key 1 and id 1 / id 2 are dropped and the pair indices count what is left."""
    #          id: -100  0   1   2   3
    pair = np.array([[2, 1, 0, 4, 0],    # void
                     [0, 5, 0, 0, 2],    # 3001 (class 3)
                     [0, 0, 0, 0, 0],    # 3002: no kept point
                     [1, 3, 0, 2, 6]])   # 5001 (class 5)
    t = A.table_from_raw([3001, 3002, 5001], pair[1:].sum(1), pair[:, 1:].sum(0), [3, 0, 0, 5], pair[0, 1:],
                         [9 << 31, 0, 6 << 32, 8 << 30], pair.reshape(-1), "mean_prob")
    want = A.ApTable(gt_code=[3001, 5001], gt_n=[7, 12], pred_id=[0, 3], pred_label=[3, 5], pred_n=[9, 8],
                     pred_void=[1, 0], pred_conf=[0.5, 0.25], pair_gt=[0, 1], pair_pred=[0, 1], pair_inter=[5, 6])
    assert_tables_equal(t, A.ApTable(*[np.asarray(v, dtype=np.float64 if f == "pred_conf" else np.int64)
                                       for f, v in zip(A.ApTable._fields, want)]))
    one = A.table_from_raw([3001, 3002, 5001], pair[1:].sum(1), pair[:, 1:].sum(0), [3, 0, 0, 5], pair[0, 1:],
                           [0, 0, 0, 0], pair.reshape(-1))
    assert one.pred_conf.dtype == np.float64 and one.pred_conf.tolist() == [1.0, 1.0]
    empty = A.table_from_raw([3001], [0], [0, 0], [0, 0], [0, 0], [0, 0], np.zeros(6, np.int64), "mean_prob")
    assert all(len(v) == 0 for v in empty) and empty.pred_conf.dtype == np.float64


def _scenes():
    return fixture_scenes("synth") + [random_scene(5, 700, 9, 11), random_scene(6, 300, 4, 5, prob_levels=(0.25, 0.5, 1.0))]


@pytest.mark.parametrize("conf", ["one", "mean_prob"])
def test_table_from_raw_equals_the_tally_of_the_filtered_scene(conf):
    scenes = _scenes()
    for sc in scenes:
        taus = [0.0] + own_thresholds([sc]) + [0.5, 1.0, 2.0]
        for tau in taus:
            got = A.table_from_raw(**raw_row(sc, kept_mask(sc[4], tau)), confidence=conf)
            assert_tables_equal(got, tally(*filtered(sc, tau), confidence=conf))
        assert_tables_equal(A.table_from_raw(**raw_row(sc, np.ones(len(sc[4]), bool)), confidence=conf),
                            tally(*sc, confidence=conf))


def test_rows_are_nested():
    for sc in _scenes():
        taus = sorted(own_thresholds([sc], qs=(0.1, 0.3, 0.5, 0.7, 0.9, 1.0)))
        rows = [raw_row(sc, np.ones(len(sc[4]), bool))] + [raw_row(sc, kept_mask(sc[4], t)) for t in taus]
        for lo, hi in zip(rows, rows[1:]):
            for f in ("key_n", "ps_n", "ps_void", "ps_sum", "pair"):
                assert (hi[f] <= lo[f]).all(), f
            assert np.array_equal(hi["key_code"], lo["key_code"])
        assert rows[-1]["pair"].sum() < rows[0]["pair"].sum()


@pytest.mark.parametrize("case,conf", [(c, m) for c in ("golden", "synth") for m in ("one", "mean_prob")])
def test_per_row_ap_equals_ap_from_tables_of_the_filtered_tally(case, conf):
    """tally stands in for the device: the rows' reduction is ap_from_tables of every row, and the coverage the share of
    the kept points."""
    scenes = fixture_scenes(case)
    taus = own_thresholds(scenes)
    tables = [[tally(*sc, confidence=conf) for sc in scenes]]
    tables += [[A.table_from_raw(**raw_row(sc, kept_mask(sc[4], tau)), confidence=conf) for sc in scenes] for tau in taus]
    kept = np.array([[len(sc[4])] + [int(kept_mask(sc[4], tau).sum()) for tau in taus] for sc in scenes])
    results, kept_rows, coverage = A.ap_from_tables_rows(tables, kept)
    assert len(results) == len(taus) + 1
    _equal_results(results[0], A.ap_from_tables(tables[0]))
    for r, tau in enumerate(taus, 1):
        _equal_results(results[r], A.ap_from_tables([tally(*filtered(sc, tau), confidence=conf) for sc in scenes]))
    assert np.array_equal(kept_rows, kept.sum(axis=0)) and coverage[0] == 1.0
    assert np.array_equal(coverage, kept.sum(axis=0) / kept.sum(axis=0)[0])
    assert (np.diff(coverage) <= 0).all() and 0 < coverage[-1] < 1
    assert np.isnan(A.ap_from_tables_rows([[]], np.zeros((0, 1), np.int64))[2]).all()


def test_refusals_come_before_any_device_work():
    n = np.zeros(4, dtype=np.int64)
    p = np.zeros(4, dtype=np.float32)
    with pytest.raises(ValueError, match="ps_prob"):
        A.ap_tables_rows([(n, n, n, n)], [0.5], device="cuda:0")
    with pytest.raises(ValueError, match="ps_prob"):
        A.ap_tables_rows([(n, n, n, n, p), dict(zip(A._FIELDS, (n, n, n, n)))], [0.5], device="cuda:0")
    with pytest.raises(ValueError, match="NaN"):
        A.ap_tables_rows([(n, n, n, n, p)], [0.5, float("nan")], device="cuda:0")
    with pytest.raises(ValueError, match="at most 32"):
        A.ap_tables_rows([(n, n, n, n, p)], [k / 40 for k in range(33)], device="cuda:0")
    with pytest.raises(ValueError, match="entries"):
        A.ap_tables_rows([(n, n, n, n, p[:3])], [0.5], device="cuda:0")
    with pytest.raises(ValueError, match="confidence"):
        A.ap_tables_rows([(n, n, n, n, p)], [0.5], confidence="max", device="cuda:0")
    with pytest.raises(ValueError, match="no scene"):
        A.evaluate_ap_rows([], [0.5], device="cuda:0")
    with pytest.raises(ValueError, match="NaN"):
        A.evaluate_ap_rows([(n, n, n, n, p)], [float("nan")], device="cuda:0")


def test_cli_arguments(tmp_path, capsys):
    for bad in ("0.5,nan", ",".join(["0.5"] * 33), "0.5,x"):
        with pytest.raises(SystemExit) as e:
            A.main(["--prob_thresholds", bad])
        assert e.value.code == 2
        assert "--prob_thresholds" in capsys.readouterr().err
    # nothing to evaluate: the flag parses (any order, blanks, a trailing comma), nothing runs, no thresholds key
    import json

    out = str(tmp_path / "ap.json")
    (tmp_path / "train").mkdir()
    rc = A.main(["--prob_thresholds", "0.8, 0.6,", "--data_root", str(tmp_path), "--ps_folder", str(tmp_path),
                 "--json", out])
    assert rc == 2
    got = json.load(open(out))
    assert got["evaluated"] == [] and "thresholds" not in got and "avgs" not in got
