"""The batched pseudo-label evaluator (gapro_eval_batch behind eval_ps_labels.evaluate_scenes) and its CLI on the
device: bit-identical to the per-scene HIP functions and to oracle/eval_oracle.py on the same (filtered) points, for
every batch composition, and the CLI's numbers against the reference main()'s formulas."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = ["s0_walls", "s1_nowalls", "s2_dense", "s3_bigspp", "s4_dups", "s5_lean"]
TAUS = (0.9, 0.5, 1.0, 0.75, 0.999)  # not sorted: rows follow the caller's order


def _golden(name):
    return np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))


def _remap(sem):
    """reference main() :191-197: .int(), then the ScanNet remap."""
    import torch

    s = torch.from_numpy(np.asarray(sem)).int()
    s[s != -100] -= 2
    s[(s == -1) | (s == -2)] = 18
    return s.long()


def _golden_scene(name):
    z = _golden(name)
    return dict(semantic_label=z["sem_gt"], instance_label=z["inst_gt"], ps_semantic_label=z["out_sem"],
                ps_instance_label=z["out_inst"], ps_prob=z["out_prob"])


def _expected(sc, tau=None, remap=True):
    """The per-scene HIP functions and the CPU oracle on the points with prob >= float32(tau)."""
    import torch
    from gapro_amd.eval_ps_labels import get_miou_scene, get_scene_sem_conf
    from oracle import eval_oracle as E

    sem = _remap(sc["semantic_label"]) if remap else torch.from_numpy(np.asarray(sc["semantic_label"])).long()
    ins = torch.from_numpy(np.asarray(sc["instance_label"])).long()
    ps_sem = torch.from_numpy(np.asarray(sc["ps_semantic_label"])).long()
    ps_ins = torch.from_numpy(np.asarray(sc["ps_instance_label"])).long()
    if tau is not None:
        keep = torch.from_numpy(np.asarray(sc["ps_prob"]) >= np.float32(tau))
        sem, ins, ps_sem, ps_ins = sem[keep], ins[keep], ps_sem[keep], ps_ins[keep]
    n = int(sem.numel())
    if n == 0:
        return np.zeros(0, np.float32), np.zeros((19, 19), np.int64), 0
    ious = get_miou_scene(sem.cuda(), ins.cuda(), ps_sem.cuda(), ps_ins.cuda()).cpu().numpy()
    conf = get_scene_sem_conf(sem.cuda(), ps_sem.cuda()).cpu().numpy()
    ref = E.get_miou_scene(sem, ins, ps_sem, ps_ins).numpy()
    np.testing.assert_array_equal(ious, ref)
    assert np.array_equal(conf, E.get_scene_sem_conf(sem, ps_sem).numpy())
    return ious, conf, n


def _check(res, scenes, taus, remap=True):
    conf = np.zeros((len(taus) + 1, 19, 19), np.int64)
    for i, sc in enumerate(scenes):
        for r, tau in enumerate((None,) + tuple(taus)):
            ious, c, n = _expected(sc, tau, remap)
            np.testing.assert_array_equal(res.ious[i][r], ious)
            assert res.ious[i][r].dtype == np.float32
            assert res.kept[i, r] == n
            conf[r] += c
    np.testing.assert_array_equal(res.conf, conf)


def test_golden_scenes_in_one_batch_reproduce_the_reference():
    from gapro_amd.eval_ps_labels import evaluate_scenes

    scenes = [_golden_scene(n) for n in GOLDEN]
    res = evaluate_scenes(scenes)
    for i, name in enumerate(GOLDEN):
        np.testing.assert_array_equal(res.ious[i][0], _golden(name)["ref_ious"])
    _check(res, scenes, ())


def test_probability_thresholds_equal_the_prefiltered_scenes():
    from gapro_amd.eval_ps_labels import evaluate_scenes

    scenes = [_golden_scene(n) for n in GOLDEN]
    res = evaluate_scenes(scenes, prob_thresholds=TAUS)
    assert res.thresholds == tuple(float(np.float32(t)) for t in TAUS)
    _check(res, scenes, TAUS)
    assert (res.kept[:, 0] == [len(s["semantic_label"]) for s in scenes]).all()
    assert res.kept[:, 1].sum() > 0 and res.kept[:, 3].sum() < res.kept[:, 0].sum()  # the filters do filter


def _random_scene(seed, n, n_gt=30, n_ps=40, gt_dtype=np.float64):
    rng = np.random.default_rng(seed)
    sem = rng.integers(0, 20, n).astype(np.float64)
    sem[rng.random(n) < 0.1] = -100
    ins = rng.integers(-1, n_gt, n)
    ins[ins < 0] = -100
    ps_ins = rng.integers(-1, n_ps, n)
    ps_ins[ps_ins < 0] = -100
    ps_sem = rng.integers(0, 19, n)
    ps_sem[ps_ins == -100] = -100
    prob = rng.random(n).astype(np.float32)
    prob[rng.random(n) < 0.05] = 1.0
    return dict(semantic_label=sem.astype(gt_dtype), instance_label=ins.astype(gt_dtype),
                ps_semantic_label=ps_sem.astype(np.int32), ps_instance_label=ps_ins.astype(np.int32), ps_prob=prob)


def test_batch_composition_does_not_change_a_bit():
    from gapro_amd.eval_ps_labels import evaluate_scenes

    scenes = [_golden_scene("s2_dense"), _random_scene(1, 0), _random_scene(2, 250000, 60, 80), _random_scene(3, 7),
              _random_scene(4, 40000, 600, 5), _golden_scene("s4_dups"), _random_scene(5, 1)]
    whole = evaluate_scenes(scenes, prob_thresholds=TAUS)
    conf = np.zeros_like(whole.conf)
    for i, sc in enumerate(scenes):
        one = evaluate_scenes([sc], prob_thresholds=TAUS)
        for r in range(len(TAUS) + 1):
            np.testing.assert_array_equal(one.ious[0][r], whole.ious[i][r])
        assert np.array_equal(one.kept[0], whole.kept[i])
        conf += one.conf
    np.testing.assert_array_equal(conf, whole.conf)
    rev = evaluate_scenes(scenes[::-1], prob_thresholds=TAUS)
    for i in range(len(scenes)):
        for r in range(len(TAUS) + 1):
            np.testing.assert_array_equal(rev.ious[len(scenes) - 1 - i][r], whole.ious[i][r])
    _check(whole, scenes, TAUS)


def test_label_dtypes_select_the_same_results():
    from gapro_amd.eval_ps_labels import evaluate_scenes

    base = _random_scene(9, 30000)
    ref = evaluate_scenes([base], prob_thresholds=(0.5,))
    for gt_dt, ps_dt in [(np.int32, np.int32), (np.int64, np.int64), (np.float64, np.int64), (np.int64, np.int32)]:
        sc = dict(base)
        sc["semantic_label"] = base["semantic_label"].astype(gt_dt)
        sc["instance_label"] = base["instance_label"].astype(gt_dt)
        sc["ps_semantic_label"] = base["ps_semantic_label"].astype(ps_dt)
        sc["ps_instance_label"] = base["ps_instance_label"].astype(ps_dt)
        got = evaluate_scenes([sc], prob_thresholds=(0.5,))
        for r in range(2):
            np.testing.assert_array_equal(got.ious[0][r], ref.ious[0][r])
        assert np.array_equal(got.conf, ref.conf) and np.array_equal(got.kept, ref.kept)


def test_stress_large_ids_empty_pseudo_labels_no_gt_instance_and_overflow():
    import torch
    from gapro_amd.eval_ps_labels import evaluate_scenes

    rng = np.random.default_rng(1)
    n = 20000
    large = dict(semantic_label=rng.integers(0, 21, n), instance_label=rng.integers(-1, 700, n),
                 ps_semantic_label=rng.integers(0, 19, n), ps_instance_label=rng.integers(-1, 900, n),
                 ps_prob=rng.random(n).astype(np.float32))  # beyond the LDS tables
    none = dict(large, ps_semantic_label=np.full(n, -100), ps_instance_label=np.full(n, -100))
    no_gt = dict(large, instance_label=np.full(n, -100))
    scenes = [large, none, no_gt]
    res = evaluate_scenes(scenes, prob_thresholds=(0.3, 0.8))
    _check(res, scenes, (0.3, 0.8))
    assert all(len(r) == 0 for r in res.ious[2])
    assert len(res.ious[1][0]) and not res.ious[1][0].any()
    # the caller's id table too small: a status, not an out-of-bounds write; the device stays usable
    small = dict(large, max_gt=100)
    with pytest.raises(ValueError, match="beyond the id table"):
        evaluate_scenes([_golden_scene("s0_walls"), small])
    torch.cuda.synchronize()
    again = evaluate_scenes([_golden_scene("s0_walls")])
    np.testing.assert_array_equal(again.ious[0][0], _golden("s0_walls")["ref_ious"])


@pytest.mark.parametrize("num_classes", [19, 128])
def test_confusion_only_launch_matches_the_oracle(num_classes):
    """get_scene_sem_conf is gapro_eval_batch without instance arrays: the oracle's matrix with the confusion in LDS
    (C = 19) and beyond it (C = 128), for GT -100, pseudo -100 and labels outside [0, C), in the labels' own dtypes,
    with the inputs left as they were."""
    import torch
    from gapro_amd.eval_ps_labels import get_scene_sem_conf
    from oracle import eval_oracle as E

    c = num_classes
    rng = np.random.default_rng(c)
    n = 200000
    gt = rng.integers(0, c, n)
    gt[rng.random(n) < 0.1] = -100
    ps = rng.integers(-3, c + 3, n)
    ps[rng.random(n) < 0.1] = -100
    # labels outside [0, C) whose flat index gt * C + ps stays in the C * C bins (torch.bincount's domain)
    ps[(gt != -100) & (ps != -100) & ((gt * c + ps < 0) | (gt * c + ps >= c * c))] = -100
    unlabeled = np.full(n, -100)
    for p_np in (ps, unlabeled):
        ref = E.get_scene_sem_conf(torch.from_numpy(gt), torch.from_numpy(p_np), c)
        for gt_dt, ps_dt in ((torch.int64, torch.int64), (torch.float64, torch.int32), (torch.int16, torch.int64)):
            g, p = torch.from_numpy(gt).to(gt_dt).cuda(), torch.from_numpy(p_np).to(ps_dt).cuda()
            g0, p0 = g.clone(), p.clone()
            conf = get_scene_sem_conf(g, p, num_classes=c)
            assert conf.is_cuda and conf.dtype == torch.int64 and conf.shape == (c, c)
            assert torch.equal(conf.cpu(), ref), (gt_dt, ps_dt)
            assert torch.equal(g, g0) and torch.equal(p, p0)
        assert int(ref.sum()) == int((gt != -100).sum())


def _write_layout(tmp_path):
    """The golden scenes as a ScanNet layout (synth.write_scannet_layout's file format) and their outputs as label
    files: 5-tuples, 2-tuples, one scene without a label file, one with a damaged one."""
    import torch
    from gapro_amd.gen_ps import write_label_file

    root, ps = tmp_path / "scannetv2", tmp_path / "labels"
    (root / "train").mkdir(parents=True)
    ps.mkdir()
    kinds = {"scene0000_00": ("s0_walls", 5), "scene0001_00": ("s1_nowalls", 2), "scene0002_00": ("s2_dense", 5),
             "scene0003_00": ("s3_bigspp", 5), "scene0004_00": ("s4_dups", 2), "scene0005_00": ("s5_lean", None),
             "scene0006_00": ("s0_walls", "corrupt")}
    for scan, (g, kind) in kinds.items():
        z = _golden(g)
        torch.save((z["xyz_raw"], z["rgb"], z["sem_gt"], z["inst_gt"]), str(root / "train" / (scan + "_inst_nostuff.pth")))
        path = str(ps / (scan + ".pth"))
        if kind == 5:
            write_label_file(path, (z["out_sem"], z["out_inst"], z["out_prob"], z["out_mu"], z["out_var"]))
        elif kind == 2:
            torch.save((z["out_sem"], z["out_inst"]), path)
        elif kind == "corrupt":
            with open(path, "wb") as fh:
                fh.write(b"PK\x03\x04" + b"\x00" * 64)
    return str(root), str(ps), kinds


def _reference_main_numbers(kinds, scans, tau=None):
    """The reference main()'s reductions (:239-252) over oracle IoUs / confusions, in sorted scene order."""
    import torch
    from oracle import eval_oracle as E

    ious, conf, kept, total = [], torch.zeros((19, 19), dtype=torch.long), 0, 0
    for scan in sorted(scans):
        sc = _golden_scene(kinds[scan][0])
        sem, ins = _remap(sc["semantic_label"]), torch.from_numpy(sc["instance_label"]).long()
        ps_sem, ps_ins = torch.from_numpy(sc["ps_semantic_label"]).long(), torch.from_numpy(sc["ps_instance_label"]).long()
        total += len(sem)
        if tau is not None:
            keep = torch.from_numpy(sc["ps_prob"] >= np.float32(tau))
            sem, ins, ps_sem, ps_ins = sem[keep], ins[keep], ps_sem[keep], ps_ins[keep]
        kept += len(sem)
        ious.append(E.get_miou_scene(sem, ins, ps_sem, ps_ins))
        conf += E.get_scene_sem_conf(sem, ps_sem)
    mean = torch.mean(torch.cat(ious, dim=0)).item()
    tp = torch.diag(conf)
    fp = torch.sum(conf, 0) - tp
    fn = torch.sum(conf, 1) - tp
    iou = tp / (tp + fp + fn) * 100
    sem_iou = [None if v != v else v for v in iou.tolist()]
    return mean, sem_iou, torch.nanmean(iou).item(), kept / total


def _run_cli(args, timeout=300):
    return subprocess.run([sys.executable, "-m", "gapro_amd.eval_ps_labels"] + args, cwd=ROOT, capture_output=True,
                          text=True, timeout=timeout)


def test_cli_end_to_end(tmp_path):
    root, ps, kinds = _write_layout(tmp_path)
    out = str(tmp_path / "eval.json")
    p = _run_cli(["--ps_folder", ps, "--data_root", root, "--stride", "1", "--prob_thresholds", "0.9", "--json", out,
                  "--batch_scenes", "2"])
    assert p.returncode == 3, p.stdout + p.stderr
    got = json.load(open(out))
    five = [s for s, (_, k) in kinds.items() if k == 5]
    two = [s for s, (_, k) in kinds.items() if k == 2]
    assert got["scanned"] == sorted(kinds) and got["missing"] == ["scene0005_00"]
    assert got["evaluated"] == five
    assert sorted(got["failed"]) == sorted(two + ["scene0006_00"])  # thresholds without a probability, the damaged file
    assert all("probability" in got["failed"][s] for s in two)
    assert "scene0006_00" in p.stderr
    mean, sem_iou, miou, _ = _reference_main_numbers(kinds, five)
    assert got["mean_inst_iou"] == mean and got["sem_iou"] == sem_iou and got["sem_miou"] == miou
    assert "mean inst iou %s" % mean in p.stdout and "sem miou %s" % miou in p.stdout
    mean9, sem_iou9, miou9, cov9 = _reference_main_numbers(kinds, five, 0.9)
    row = got["thresholds"][0]
    assert row["threshold"] == 0.9 and row["coverage"] == cov9
    assert row["mean_inst_iou"] == mean9 and row["sem_iou"] == sem_iou9 and row["sem_miou"] == miou9
    assert got["points"] == sum(len(_golden(kinds[s][0])["sem_gt"]) for s in five)

    # without thresholds the 2-tuples are evaluated too; only the damaged file fails
    p = _run_cli(["--ps_folder", ps, "--data_root", root, "--stride", "1", "--json", out])
    assert p.returncode == 3, p.stdout + p.stderr
    got = json.load(open(out))
    assert list(got["failed"]) == ["scene0006_00"] and "scene0006_00" in p.stderr
    assert got["evaluated"] == sorted(five + two) and got["thresholds"] == []
    mean, sem_iou, miou, _ = _reference_main_numbers(kinds, five + two)
    assert got["mean_inst_iou"] == mean and got["sem_iou"] == sem_iou and got["sem_miou"] == miou

    # every listed scene that has a label file evaluated: 0; the reference's stride picks scene0000 and scene0006
    os.remove(os.path.join(ps, "scene0006_00.pth"))
    p = _run_cli(["--ps_folder", ps, "--data_root", root, "--stride", "3", "--json", out])
    assert p.returncode == 0, p.stdout + p.stderr
    got = json.load(open(out))
    assert got["scanned"] == ["scene0000_00", "scene0003_00", "scene0006_00"]
    assert got["evaluated"] == ["scene0000_00", "scene0003_00"] and got["missing"] == ["scene0006_00"]
