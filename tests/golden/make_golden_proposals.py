#!/usr/bin/env python3
"""Generate tests/golden/proposals_*.npz by running the REFERENCE's ISBNet.get_instance in this container.

Run from the repo root:  python tests/golden/make_golden_proposals.py
Needs /root/reference (read-only).  What is executed from the reference, on CPU tensors: ``ISBNet.get_instance``
(ISBNet/isbnet/model/isbnet.py:887-1005), unbound, with a ``SimpleNamespace`` as ``self``, and through it ``nms`` with
both ``type_nms`` values, ``custom_scatter_mean``, ``superpoint_align`` and ``rle_encode_gpu_batch``, imported as they
are.  IN THIS HARNESS ONLY: ``spconv.pytorch``, ``isbnet.ops``, ``isbnet.model.aggregator`` and ``isbnet.model.blocks``
are empty stubs (get_instance never calls them); ``isbnet.util`` is the reference's util/rle.py loaded by path plus an
identity ``cuda_cast``; ``torch_scatter`` is the pure-torch shim of make_golden_spp_gt.py (float32 sums, count clamped at
1), extended to ``dim=-1`` with an expanded index and to ``scatter(reduce="mean")``.

The reference leaves the order of its output and every tie to ``torch.topk(sorted=False)`` and an unstable ``argsort``,
so a fixture is only written if the reference alone meets these conditions (asserted below, not tolerances):
  (a) any two candidate scores among the first pre_topk + 1 differ by more than 1e-5 relative;
  (b) every updated score differs from final_score_thresh, and the topk-th from the (topk + 1)-th, by more than 1e-5
      relative;
  (c) no iou lies within 1e-6 of nms_threshold;
  (d) V, N < 2^24.
The fixtures hold the inputs, the parameters and what the reference returned (label_id, conf, the counts of every
instance back to back with their offsets).  Nothing of the reference's text is written.  The restatement
tests/proposals_ref.py is run on the same inputs; the largest relative deviation of its conf from the reference's float32
chain is printed.
"""
import importlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference/ISBNet"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(REPO, "tests"))

import proposals_cases  # noqa: E402
import proposals_ref  # noqa: E402

PRE_TOPK, FINAL_SCORE_THRESH = 300, 0.1


def install_stubs():
    ts = types.ModuleType("torch_scatter")

    def scatter_mean(src, index, dim=0, out=None, dim_size=None):
        assert out is None and src.is_floating_point()
        if dim in (-1, src.dim() - 1) and src.dim() == 2:
            assert index.shape == src.shape
            n = int(index.max()) + 1 if dim_size is None else dim_size
            res = torch.zeros((src.shape[0], n), dtype=src.dtype).scatter_add_(1, index, src)
            cnt = torch.zeros((src.shape[0], n), dtype=src.dtype).scatter_add_(1, index, torch.ones_like(src))
            return res / cnt.clamp_(1)
        assert dim == 0
        n = int(index.max()) + 1 if dim_size is None else dim_size
        res = torch.zeros((n,) + tuple(src.shape[1:]), dtype=src.dtype).index_add_(0, index, src)
        cnt = torch.zeros(n, dtype=src.dtype).index_add_(0, index, torch.ones(src.shape[0], dtype=src.dtype))
        cnt.clamp_(1)
        return res / (cnt[:, None] if res.dim() > 1 else cnt)

    def scatter(src, index, dim=-1, out=None, dim_size=None, reduce="sum"):
        assert reduce == "mean"
        return scatter_mean(src, index, dim=dim, out=out, dim_size=dim_size)

    ts.scatter_mean, ts.scatter = scatter_mean, scatter
    sys.modules["torch_scatter"] = ts
    spconv = types.ModuleType("spconv")
    spconv.pytorch = types.ModuleType("spconv.pytorch")
    pkg = types.ModuleType("isbnet")
    pkg.__path__ = [os.path.join(REF, "isbnet")]
    ops = types.ModuleType("isbnet.ops")
    ops.ballquery_batchflat = ops.voxelization = None
    model = types.ModuleType("isbnet.model")
    model.__path__ = [os.path.join(REF, "isbnet", "model")]
    agg = types.ModuleType("isbnet.model.aggregator")
    agg.LocalAggregator = None
    blocks = types.ModuleType("isbnet.model.blocks")
    for name in ("MLP", "GenericMLP", "ResidualBlock", "UBlock", "conv_with_kaiming_uniform"):
        setattr(blocks, name, None)
    spec = importlib.util.spec_from_file_location("isbnet.util.rle", os.path.join(REF, "isbnet", "util", "rle.py"))
    rle = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rle)
    util = types.ModuleType("isbnet.util")
    util.rle_encode_gpu, util.rle_encode_gpu_batch, util.rle_decode = (rle.rle_encode_gpu, rle.rle_encode_gpu_batch,
                                                                       rle.rle_decode)
    util.cuda_cast = lambda f: f
    sys.modules.update({"spconv": spconv, "spconv.pytorch": spconv.pytorch, "isbnet": pkg, "isbnet.ops": ops,
                        "isbnet.model": model, "isbnet.model.aggregator": agg, "isbnet.model.blocks": blocks,
                        "isbnet.util": util, "isbnet.util.rle": rle})


def rel_gap(a, b):
    return abs(float(a) - float(b)) / max(abs(float(a)), abs(float(b)), 1e-30)


def check_conditions(name, mu, c, p):
    """(a)-(d) on the reference's own float32 numbers."""
    import torch.nn.functional as F
    C = c["instance_classes"]
    cls = F.softmax(torch.from_numpy(c["cls_logits"]), dim=-1)[:, :-1]
    score = torch.sqrt(cls * torch.clamp(torch.from_numpy(c["conf_logits"]), 0.0, 1.0)[:, None]).reshape(-1)
    top, idx = torch.sort(score, descending=True)
    k = min(PRE_TOPK, len(score))
    for i in range(min(k, len(score) - 1)):
        assert rel_gap(top[i], top[i + 1]) > 1e-5, (name, "a", i)
    idx = idx[:k]
    masks = torch.from_numpy(c["mask_logits"][:, c["voxel_spps"]]) >= p["logit_thresh"]
    q = torch.div(idx, C, rounding_mode="floor")
    keep = masks[q].sum(1) >= p["npoint_thresh"]
    m, cat, sc = masks[q][keep], (idx % C)[keep], top[:k][keep]
    boxes = torch.zeros((len(sc), 6))
    if p["type_nms"] == "matrix":
        _, _, upd, _ = mu.matrix_nms(m, cat, sc, boxes, final_score_thresh=-1.0, topk=-1)
        upd, _ = torch.sort(upd, descending=True)
        for u in upd:
            assert rel_gap(u, FINAL_SCORE_THRESH) > 1e-5, (name, "b thresh")
        t = p["topk"]
        if t != -1 and t < len(upd):
            assert rel_gap(upd[t - 1], upd[t]) > 1e-5, (name, "b topk")
    else:
        f = m.float()
        inter = f @ f.T
        n = f.sum(1)
        iou = inter / (n[None, :] + n[:, None] - inter)
        assert (torch.abs(iou - p["nms_threshold"]) > 1e-6).all(), (name, "c")
    assert masks.shape[1] < 2 ** 24 and len(c["v2p_map"]) < 2 ** 24, (name, "d")


# name -> scene arguments, parameters
FIXTURES = (
    ("matrix", dict(seed=501), dict(type_nms="matrix", topk=100, npoint_thresh=30)),
    ("matrix_topk", dict(seed=503), dict(type_nms="matrix", topk=12, npoint_thresh=30)),
    ("matrix_thresh", dict(seed=504), dict(type_nms="matrix", topk=-1, npoint_thresh=30)),
    ("standard", dict(seed=505), dict(type_nms="standard", topk=100, npoint_thresh=30, nms_threshold=0.2)),
    ("s3dis", dict(seed=506, C=13, n_sem_classes=5),
     dict(type_nms="matrix", topk=100, npoint_thresh=30, sem2ins_classes=(0, 1), dataset_name="s3dis")),
    ("few_queries", dict(seed=507, Q=12, C=18, V=400, N=450, S=30, n_inst=4),
     dict(type_nms="matrix", topk=100, npoint_thresh=20)),
)


def main():
    install_stubs()
    mu = importlib.import_module("isbnet.model.model_utils")
    net = importlib.import_module("isbnet.model.isbnet")
    worst = 0.0
    for name, scene_args, par in FIXTURES:
        c = proposals_cases.make_scene(**scene_args)
        p = dict(logit_thresh=0.0, nms_threshold=0.2, sem2ins_classes=(), dataset_name="scannetv2")
        p.update(par)
        check_conditions(name, mu, c, p)
        me = types.SimpleNamespace(
            sem2ins_classes=list(p["sem2ins_classes"]), ignore_label=-100, instance_classes=c["instance_classes"],
            use_spp_pool=True, dataset_name=p["dataset_name"],
            test_cfg=types.SimpleNamespace(type_nms=p["type_nms"], topk=p["topk"], nms_threshold=p["nms_threshold"]))
        t = {k: torch.from_numpy(np.asarray(c[k])) for k in proposals_cases.KEYS}
        got = net.ISBNet.get_instance(me, "scene", t["cls_logits"], t["mask_logits"][:, torch.from_numpy(c["voxel_spps"])],
                                      t["conf_logits"], t["box_preds"], t["v2p_map"], t["semantic_preds"], t["spps"],
                                      logit_thresh=p["logit_thresh"], npoint_thresh=p["npoint_thresh"])
        label = np.array([int(g["label_id"]) for g in got], np.int64)
        conf = np.array([np.float32(g["conf"]) for g in got], np.float32)
        counts = [np.asarray(g["pred_mask"]["counts"], np.int64) for g in got]
        assert all(g["pred_mask"]["length"] == len(c["v2p_map"]) for g in got)
        offsets = np.concatenate([[0], np.cumsum([len(x) for x in counts])]).astype(np.int64)
        shift = {"scannetv2": 1, "s3dis": 3}[p["dataset_name"]]
        ours = proposals_ref.get_instance_ref(
            **c, logit_thresh=p["logit_thresh"], npoint_thresh=p["npoint_thresh"], type_nms=p["type_nms"],
            topk=p["topk"], nms_threshold=p["nms_threshold"], sem2ins_classes=p["sem2ins_classes"], label_shift=shift)
        dev = proposals_ref.compare_with_reference(ours, label, conf, counts)
        worst = max(worst, dev)
        arrays = dict(c)
        arrays.pop("voxel_spps")
        np.savez_compressed(
            os.path.join(OUT, "proposals_%s.npz" % name), voxel_spps=c["voxel_spps"],
            type_nms=np.array(p["type_nms"]), topk=np.int64(p["topk"]), npoint_thresh=np.int64(p["npoint_thresh"]),
            logit_thresh=np.float64(p["logit_thresh"]), nms_threshold=np.float64(p["nms_threshold"]),
            sem2ins_classes=np.asarray(p["sem2ins_classes"], np.int64), label_shift=np.int64(shift),
            ref_label_id=label, ref_conf=conf, ref_counts=np.concatenate(counts) if counts else np.zeros(0, np.int64),
            ref_offsets=offsets, **arrays)
        print("%-14s %-8s instances=%3d  runs=%5d  conf deviation %.3g  %d bytes"
              % (name, p["type_nms"], len(got), int(offsets[-1]) // 2, dev,
                 os.path.getsize(os.path.join(OUT, "proposals_%s.npz" % name))))
    assert [f[0] for f in FIXTURES] == proposals_ref.FIXTURES
    print("wrote %d fixtures; largest relative conf deviation of the restatement: %.3g" % (len(FIXTURES), worst))


if __name__ == "__main__":
    main()
