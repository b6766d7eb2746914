"""The stand-alone pseudo-label evaluator's host side (gapro_amd/eval_ps_labels.py: evaluate_scenes / main): the
batched ABI, the scene list, the label-file parsing and the reference main()'s reductions.  No GPU needed."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

from gapro_amd import _lib
from gapro_amd import eval_ps_labels as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batched_eval_abi_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "gapro_hip.h")).read()
    for name in ("gapro_eval_batch_workspace_bytes", "gapro_eval_batch"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name)
    assert "gapro_eval_scene" in text
    assert C.sizeof(_lib.EvalScene) == 8 + 8 + 4 + 4 + 8 + 8


def test_per_scene_eval_abi_is_gone():
    """get_miou_scene / get_scene_sem_conf are one-scene calls of gapro_eval_batch: the former per-scene entry points
    are neither declared, exported nor bound."""
    text = open(os.path.join(ROOT, "include", "gapro_hip.h")).read()
    lib = _lib.load()
    for name in ("gapro_eval_workspace_bytes", "gapro_eval_miou", "gapro_eval_sem_confusion"):
        assert not re.search(r"\b%s\b" % name, text), name
        assert name not in _lib.SIGNATURES
        assert not hasattr(lib, name), name
    assert "gapro_eval_header" not in text
    assert not hasattr(_lib, "EvalHeader")


def test_batched_eval_workspace_plan():
    lib = _lib.load()
    d = (_lib.EvalScene * 3)()
    for i, (n, g, p) in enumerate([(10, 3, 4), (0, 1, 1), (5, 700, 900)]):
        d[i].point_offset, d[i].n_points, d[i].max_gt, d[i].max_ps = 0, n, g, p
    for k in (0, 4):
        total = lib.gapro_eval_batch_workspace_bytes(d, 3, k)
        b = k + 1
        sizes = [-(-(b * (g + p) * 8 + b * ((g + 1) * (p + 1) + p) * 4) // 256) * 256
                 for g, p in [(3, 4), (1, 1), (700, 900)]]
        assert total == sum(sizes)
        assert [x.ws_offset for x in d] == [0, sizes[0], sizes[0] + sizes[1]]
        assert [x.row_offset for x in d] == [0, b * 3, b * 4]
    assert lib.gapro_eval_batch_workspace_bytes(d, 3, _lib.GAPRO_EVAL_MAX_THRESHOLDS + 1) == 0
    d[1].max_gt = 0
    assert lib.gapro_eval_batch_workspace_bytes(d, 3, 0) == 0


def _touch(path):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    open(path, "wb").close()


def test_scene_list_takes_the_stride_before_skipping_missing_label_files(tmp_path):
    root, ps = str(tmp_path / "scannetv2"), str(tmp_path / "labels")
    names = ["scene%04d_00" % i for i in range(23)]
    for n in reversed(names):
        _touch(os.path.join(root, "train", n + "_inst_nostuff.pth"))
    # the reference's rule (eval_ps_labels.py:176-179) on the same folder
    ref = sorted(s[:12] for s in os.listdir(os.path.join(root, "train")))[::10]
    assert E.list_scenes(root, "train", 10) == ref == ["scene0000_00", "scene0010_00", "scene0020_00"]
    assert E.list_scenes(root, "train", 1) == names
    # label files only for scenes the stride does not pick: nothing is evaluated (and no device is touched)
    for n in names:
        if n not in ref:
            _touch(os.path.join(ps, n + ".pth"))
    out = str(tmp_path / "out.json")
    rc = E.main(["--ps_folder", ps, "--data_root", root, "--json", out])
    assert rc == 2
    got = json.load(open(out))
    assert got["scanned"] == ref and got["missing"] == ref and got["evaluated"] == [] and got["failed"] == {}


def test_label_file_parsing(tmp_path):
    from gapro_amd.gen_ps import write_label_file

    n, s = 500, 40
    rng = np.random.default_rng(0)
    sem = rng.integers(-100, 18, n).astype(np.int32)
    ins = rng.integers(-100, 30, n).astype(np.int32)
    prob = rng.random(n).astype(np.float32)
    mu, var = rng.random(s).astype(np.float32), rng.random(s).astype(np.float32)

    five = str(tmp_path / "five.pth")
    write_label_file(five, (sem, ins, prob, mu, var))
    a, b, p = E.read_label_file(five, need_prob=True)
    assert a.dtype == np.int32 and np.array_equal(a, sem) and np.array_equal(b, ins) and np.array_equal(p, prob)

    two = str(tmp_path / "two.pth")  # the reference's 2-tuple (eval_ps_labels.py:208)
    torch.save((sem.astype(np.int64), ins.astype(np.int64)), two)
    a, b, p = E.read_label_file(two)
    assert a.dtype == np.int64 and np.array_equal(a, sem) and np.array_equal(b, ins) and p is None
    with pytest.raises(ValueError, match="probability"):
        E.read_label_file(two, need_prob=True)

    spp = str(tmp_path / "spp.pth")  # [2] of superpoint length: not a per-point probability
    torch.save((sem, ins, mu, mu, var), spp)
    assert E.read_label_file(spp)[2] is None
    with pytest.raises(ValueError, match="probability"):
        E.read_label_file(spp, need_prob=True)

    tens = str(tmp_path / "tensors.pth")  # torch tensors: the torch.load fallback
    torch.save((torch.from_numpy(sem), torch.from_numpy(ins), torch.from_numpy(prob)), tens)
    a, b, p = E.read_label_file(tens, need_prob=True)
    assert np.array_equal(a, sem) and np.array_equal(b, ins) and np.array_equal(p, prob)

    bad = str(tmp_path / "bad.pth")
    with open(bad, "wb") as fh:
        fh.write(b"PK\x03\x04 this is not a label file" * 4)
    with pytest.raises(Exception):
        E.read_label_file(bad)


def _reference_reduction(conf_metric):
    """reference eval_ps_labels.py:243-252, literally."""
    true_positive = torch.diag(conf_metric)
    false_positive = torch.sum(conf_metric, 0) - true_positive
    false_negative = torch.sum(conf_metric, 1) - true_positive
    iou = true_positive / (true_positive + false_positive + false_negative)
    iou = iou * 100
    miou = torch.nanmean(iou)
    return iou, miou


@pytest.mark.parametrize("seed", range(4))
def test_semantic_reduction_matches_the_reference_formulas(seed):
    rng = np.random.default_rng(seed)
    conf = rng.integers(0, 5000, size=(19, 19)).astype(np.int64)
    absent = rng.choice(19, size=3, replace=False)
    conf[absent, :] = 0
    conf[:, absent] = 0
    iou, miou = E.sem_iou_from_conf(conf)
    ref_iou, ref_miou = _reference_reduction(torch.from_numpy(conf))
    assert iou.dtype == np.float32
    np.testing.assert_array_equal(iou, ref_iou.numpy())
    assert miou == ref_miou.item()
    assert np.isnan(iou[absent]).all() and not np.isnan(np.delete(iou, absent)).any()
    c = conf.astype(np.float64)
    tp = np.diag(c)
    with np.errstate(invalid="ignore"):
        ref64 = tp / (c.sum(0) + c.sum(1) - tp) * 100
    np.testing.assert_allclose(np.delete(iou, absent), np.delete(ref64, absent), rtol=1e-6)


def test_evaluate_scenes_argument_checks():
    n = np.zeros(4, dtype=np.int64)
    with pytest.raises(ValueError, match="ps_prob"):
        E.evaluate_scenes([(n, n, n, n)], prob_thresholds=(0.5,), device="cuda:0")
    with pytest.raises(ValueError, match="length"):
        E.evaluate_scenes([(n, n, n[:3], n[:3])], device="cuda:0")
    with pytest.raises(ValueError, match="thresholds"):
        E.evaluate_scenes([(n, n, n, n, n)], prob_thresholds=[0.5] * 33, device="cuda:0")
