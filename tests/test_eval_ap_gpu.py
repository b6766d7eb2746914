"""ScanNet instance AP of pseudo-labels on the device (gapro_eval_ap_keys / gapro_eval_ap_tables behind
eval_ap_ps_labels.ap_tables) and its CLI: the device tables equal the NumPy tally of ap_tally.py bit for bit, for every
label dtype and batch composition, and evaluate_ap reproduces the reference ScanNetEval's numbers of
tests/golden/ap_eval.npz."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from ap_tally import assert_tables_equal, fixture, fixture_scenes, tally

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AVG_KEYS = ("all_ap", "all_ap_50%", "all_ap_25%", "all_rc", "all_rc_50%", "all_rc_25%")


def _all_scenes():
    return fixture_scenes("golden") + fixture_scenes("synth")


def _as(sc, gt_dt, ps_dt):
    return [sc[0].astype(gt_dt), sc[1].astype(gt_dt), sc[2].astype(ps_dt), sc[3].astype(ps_dt), sc[4]]


@pytest.mark.parametrize("gt_dt", [np.float64, np.int32, np.int64])
@pytest.mark.parametrize("ps_dt", [np.int32, np.int64])
def test_device_tables_equal_the_numpy_tally(gt_dt, ps_dt):
    from gapro_amd.eval_ap_ps_labels import ap_tables

    scenes = [_as(sc, gt_dt, ps_dt) for sc in _all_scenes()]
    for conf in ("one", "mean_prob"):
        ref = [tally(*sc, confidence=conf) for sc in scenes]
        for got, want in zip(ap_tables(scenes, conf), ref):
            assert_tables_equal(got, want)


def test_batch_splits_and_orders_do_not_change_a_bit():
    from gapro_amd.eval_ap_ps_labels import ap_tables

    scenes = _all_scenes()
    ref = [tally(*sc, confidence="mean_prob") for sc in scenes]
    rng = np.random.default_rng(3)
    for split in (1, 2, 3, 7, len(scenes)):
        order = rng.permutation(len(scenes))
        for i in range(0, len(scenes), split):
            part = order[i:i + split]
            for j, got in zip(part, ap_tables([scenes[k] for k in part], "mean_prob")):
                assert_tables_equal(got, ref[j])


@pytest.mark.parametrize("case,conf", [(c, m) for c in ("golden", "synth") for m in ("one", "mean_prob")])
def test_evaluate_ap_reproduces_the_reference(case, conf):
    from gapro_amd.eval_ap_ps_labels import evaluate_ap

    z = fixture()
    res = evaluate_ap(fixture_scenes(case), confidence=conf)
    key = "%s_%s" % (case, conf)
    np.testing.assert_allclose(res.ap, z[key + "_ap"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(res.rc, z[key + "_rc"], rtol=0, atol=1e-12)
    np.testing.assert_allclose([res.avgs[k] for k in AVG_KEYS], z[key + "_avg"], rtol=0, atol=1e-12)


def _big_scene(seed, n=1_000_000, n_gt=260, n_ps=600):
    rng = np.random.default_rng(seed)
    gt = rng.integers(0, n_gt, n)
    sem = (gt % 17 + 2).astype(np.float64)  # classes 1..17 after the remap
    sem[rng.random(n) < 0.05] = 0           # wall / floor: void
    ps = np.where(rng.random(n) < 0.8, gt % n_ps, rng.integers(0, n_ps, n))
    ps[rng.random(n) < 0.05] = -100
    ps_sem = (ps % 17).astype(np.int32)
    prob = rng.random(n).astype(np.float32)
    return [sem, gt.astype(np.float64), ps_sem, ps.astype(np.int32), prob]


def test_stress_beyond_lds_empty_and_no_prediction_scenes():
    import torch
    from gapro_amd.eval_ap_ps_labels import ap_tables

    big = _big_scene(1)
    golden = fixture_scenes("golden")[0]
    empty = [a[:0] for a in golden]
    no_pred = list(golden)
    no_pred[3] = np.full_like(golden[3], -100)
    bg_only = list(golden)
    bg_only[2] = np.full_like(golden[2], 18)  # gen_ps's background class: no prediction has a class
    scenes = [golden, big, empty, no_pred, bg_only]
    got = ap_tables(scenes, "mean_prob")
    for g, sc in zip(got, scenes):
        assert_tables_equal(g, tally(*sc, confidence="mean_prob"))
    assert len(got[1].gt_code) > 200 and len(got[1].pred_id) > 512  # past the LDS pair and per-id tables
    assert len(got[2].gt_code) == 0 and len(got[2].pred_id) == 0
    assert len(got[3].pred_id) == 0 and len(got[4].pred_id) == 0 and len(got[3].gt_code) > 0

    # out-of-range ids and a NaN probability: that scene's status, named; the device stays usable
    for bad_field, value in ((1, 999), (3, -5), (3, 10 ** 6), (4, np.nan), (4, 1.5)):
        bad = [a.copy() for a in golden]
        bad[bad_field][17] = value
        if bad_field == 3:
            bad = dict(zip(("semantic_label", "instance_label", "ps_semantic_label", "ps_instance_label", "ps_prob"),
                           bad), max_ps=int(golden[3].max()) + 1)
        with pytest.raises(ValueError, match=r"scene\(s\) \[1\]"):
            ap_tables([golden, bad, golden], "mean_prob")
    torch.cuda.synchronize()
    assert_tables_equal(ap_tables([golden])[0], tally(*golden))


def _write_layout(tmp_path):
    """The golden scenes as a ScanNet layout, labels as gen_ps 5-tuples, 2-tuples, one missing, one damaged."""
    import torch
    from gapro_amd.gen_ps import write_label_file

    root, ps = tmp_path / "scannetv2", tmp_path / "labels"
    (root / "train").mkdir(parents=True)
    ps.mkdir()
    kinds = {"scene0000_00": ("s0_walls", 5), "scene0001_00": ("s1_nowalls", 2), "scene0002_00": ("s2_dense", 5),
             "scene0003_00": ("s3_bigspp", 5), "scene0004_00": ("s4_dups", 2), "scene0005_00": ("s5_lean", 5),
             "scene0006_00": ("s0_walls", None)}
    for scan, (g, kind) in kinds.items():
        z = np.load(os.path.join(ROOT, "tests", "golden", g + ".npz"))
        torch.save((z["xyz_raw"], z["rgb"], z["sem_gt"], z["inst_gt"]), str(root / "train" / (scan + "_inst_nostuff.pth")))
        path = str(ps / (scan + ".pth"))
        if kind == 5:
            write_label_file(path, (z["out_sem"], z["out_inst"], z["out_prob"], z["out_mu"], z["out_var"]))
        elif kind == 2:
            torch.save((z["out_sem"], z["out_inst"]), path)
    return str(root), str(ps), kinds


def _run_cli(args, timeout=300):
    return subprocess.run([sys.executable, "-m", "gapro_amd.eval_ap_ps_labels"] + args, cwd=ROOT, capture_output=True,
                          text=True, timeout=timeout)


def test_cli_end_to_end(tmp_path):
    root, ps, kinds = _write_layout(tmp_path)
    out = str(tmp_path / "ap.json")
    z = fixture()
    p = _run_cli(["--ps_folder", ps, "--data_root", root, "--json", out, "--batch_scenes", "4"])
    assert p.returncode == 0, p.stdout + p.stderr
    got = json.load(open(out))
    assert got["scanned"] == sorted(kinds) and got["missing"] == ["scene0006_00"] and got["failed"] == {}
    assert got["evaluated"] == sorted(kinds)[:6]
    assert got["confidence"] == "one" and got["min_region_size"] == 100
    want = dict(zip(AVG_KEYS, z["golden_one_avg"]))
    for k in AVG_KEYS:
        assert abs(got["avgs"][k] - want[k]) < 1e-12, k
    assert "AP: {:.3f}. AP_50: {:.3f}. AP_25: {:.3f}".format(*z["golden_one_avg"][:3]) in p.stdout
    assert "#" * 64 in p.stdout and "average        :" in p.stdout
    assert got["avgs"]["classes"]["cabinet"]["ap"] is None or isinstance(got["avgs"]["classes"]["cabinet"]["ap"], float)
    assert sum(got["n_gt"].values()) > 0 and all(k in got for k in ("elapsed_s", "eval_s", "ap_s"))

    # mean_prob: the 2-tuples have no probability and fail cleanly, the others are evaluated
    p = _run_cli(["--ps_folder", ps, "--data_root", root, "--json", out, "--confidence", "mean_prob"])
    assert p.returncode == 3, p.stdout + p.stderr
    got = json.load(open(out))
    assert sorted(got["failed"]) == ["scene0001_00", "scene0004_00"]
    assert all("--confidence mean_prob" in v for v in got["failed"].values())
    assert got["evaluated"] == ["scene0000_00", "scene0002_00", "scene0003_00", "scene0005_00"]

    # an unreadable label file: 3
    with open(os.path.join(ps, "scene0003_00.pth"), "wb") as fh:
        fh.write(b"PK\x03\x04" + b"\x00" * 64)
    p = _run_cli(["--ps_folder", ps, "--data_root", root, "--json", out])
    assert p.returncode == 3 and "scene0003_00" in p.stderr, p.stdout + p.stderr
    assert list(json.load(open(out))["failed"]) == ["scene0003_00"]

    # nothing to evaluate: 2; mean_prob on 2-tuple files only: 2
    p = _run_cli(["--ps_folder", str(tmp_path / "none"), "--data_root", root, "--json", out])
    assert p.returncode == 2 and json.load(open(out))["evaluated"] == []
    two = tmp_path / "two"
    two.mkdir()
    for scan in ("scene0001_00", "scene0004_00"):
        shutil.copy(os.path.join(ps, scan + ".pth"), str(two / (scan + ".pth")))
    p = _run_cli(["--ps_folder", str(two), "--data_root", root, "--confidence", "mean_prob", "--json", out])
    assert p.returncode == 2, p.stdout + p.stderr
    assert "Traceback" not in p.stderr and sorted(json.load(open(out))["failed"]) == ["scene0001_00", "scene0004_00"]


@pytest.mark.parametrize("conf", ["one", "mean_prob"])
def test_evaluate_ap_reproduces_the_reference_on_the_threshold_edges(conf):
    """tests/golden/ap_eval_edges.npz: values on every comparison of evaluate_matches (IoU exactly 0.5 and 0.25, 99 and
    100 points, ignored shares of exactly 0.5 and 0.25), the device tables included."""
    from gapro_amd.eval_ap_ps_labels import ap_tables, evaluate_ap

    z = np.load(os.path.join(ROOT, "tests", "golden", "ap_eval_edges.npz"))
    scenes = [[z["edges%d_%s" % (i, k)] for k in ("sem_gt", "inst_gt", "ps_sem", "ps_inst", "prob")]
              for i in range(int(z["n_edges"]))]
    for got, sc in zip(ap_tables(scenes, conf), scenes):
        assert_tables_equal(got, tally(*sc, confidence=conf))
    res = evaluate_ap(scenes, confidence=conf)
    key = "edges_%s" % conf
    np.testing.assert_allclose(res.ap, z[key + "_ap"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(res.rc, z[key + "_rc"], rtol=0, atol=1e-12)
    np.testing.assert_allclose([res.avgs[k] for k in AVG_KEYS], z[key + "_avg"], rtol=0, atol=1e-12)
