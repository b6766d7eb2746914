#!/usr/bin/env python3
"""Time forward plus backward of ``consumer_ops.matched_losses`` against a plain torch statement of the loop it replaces
(per sample the chain of ISBNet's ``Criterion.single_layer_loss``: three gathers, the dice loss, a BCE of the whole
block, the IoU, a scatter into the class targets, a weighted cross-entropy, an L1 loss, the GIoU and the level-set loss
with its box test, ``nonzero``, ``unique`` and three scatters), on the same device, in the same run, on synthetic input
of ISBNet's step shape.

    python tools/bench_losses.py [--batch 4] [--queries 256] [--instances 40] [--spps 1500] [--feats 3]
                                 [--seconds 1.0] [--count-launches]

A call is the forward, the weighted sum of the seven losses and its backward, timed between two HIP events on the
stream; ``matched_losses`` is timed with ``check=True`` (one synchronisation for the status) and with ``check=False``.
Each form is warmed up, then called in alternating blocks until it has filled its window; the median, minimum and
maximum of the per-call times are printed and one JSON line.  The two forms' losses and gradients are compared first
(the torch chain is float32: 1e-4 relative to each array's largest magnitude).  ``--count-launches`` also counts the
device kernels of one call of each form with ``torch.profiler``.  Needs the GPU: there is no CPU timing.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

from gapro_amd import consumer_ops  # noqa: E402
from bench_match import make_batch  # noqa: E402
from bench_spp_gt import timed  # noqa: E402

WEIGHTS = (1.0, 1.0, 0.5, 0.5, 0.5, 0.5, 0.5)  # Criterion.loss_weight in the order of consumer_ops.LOSS_NAMES


def make_step(batch, queries, instances, spps, feats, seed=0):
    """bench_match's batch, one matched query per instance, and per superpoint a weight, features and a coordinate that
    mostly lies in its instance's box."""
    rng = np.random.default_rng(seed + 1)
    cls_logits, logits, conf, box_preds, dc = make_batch(batch, queries, instances, spps, seed=seed)
    gt = {k: [] for k in ("row_indices", "inst_labels", "cls_labels", "box_labels")}
    coords = rng.uniform(-5, 8, (batch * spps, 3))
    for b, e in enumerate(dc):
        gt["row_indices"].append(np.sort(rng.permutation(queries)[:instances]).astype(np.int64))
        gt["inst_labels"].append(e["mask"])
        gt["cls_labels"].append(e["cls"])
        gt["box_labels"].append(e["box"])
        owner = np.where(e["mask"].sum(0) > 0, e["mask"].argmax(0), -1)
        inside = (owner >= 0) & (rng.random(spps) < 0.7)
        lo, hi = e["box"][owner[inside], :3], e["box"][owner[inside], 3:]
        coords[b * spps:(b + 1) * spps][inside] = lo + rng.uniform(0.05, 0.95, lo.shape) * (hi - lo)
    return {"cls_logits": cls_logits, "mask_logits": logits, "conf_logits": conf, "box_preds": box_preds,
            "prob_labels": rng.uniform(0.05, 1, batch * spps).astype(np.float32),
            "batch_offsets": [b * spps for b in range(batch + 1)],
            "levelset_feats": rng.uniform(0, 1, (batch * spps, feats)).astype(np.float32),
            "levelset_coords": coords.astype(np.float32)}, gt


def giou_pairs(p, g):
    """model_utils.py:277-306."""
    inter = (torch.min(p[:, 3:], g[:, 3:]) - torch.max(p[:, :3], g[:, :3])).clamp(min=0).prod(-1)
    union = (g[:, 3:] - g[:, :3]).clamp(min=0).prod(-1) + (p[:, 3:] - p[:, :3]).clamp(min=0).prod(-1) - inter
    bound = (torch.max(p[:, 3:], g[:, 3:]) - torch.min(p[:, :3], g[:, :3])).clamp(min=0).prod(-1)
    return inter / (union + 1e-6) - (bound - union) / (bound + 1e-6)


def scatter_sum(src, index, n):
    return torch.zeros((n,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device).index_add(0, index, src)


def torch_levelset(coords, feats, x, box):
    """criterion.py:193-233, torch_scatter's sums and mean as index_add."""
    within = ((coords[None] >= box[:, None, :3] - 0.005).all(-1) & (coords[None] <= box[:, None, 3:] + 0.005).all(-1))
    some = within.sum(1) > 0
    box_i, point_i = torch.nonzero(within[some], as_tuple=True)
    v = torch.sigmoid(x[some][box_i, point_i])
    f = feats[point_i]
    _, norm = torch.unique(box_i, return_inverse=True)
    n = int(some.sum())
    mean = scatter_sum(f * v[:, None], norm, n) / scatter_sum(v, norm, n).clamp(min=0.00001)[:, None]
    dev = f - mean[norm]
    per_point = (dev * dev * v[:, None]).sum(1)
    per_box = scatter_sum(per_point, norm, n) / scatter_sum(torch.ones_like(v), norm, n).clamp(min=1)
    return per_box.sum() / (len(box) + 1e-4)


def torch_losses(cls_logits, mask_logits, conf_logits, box_preds, prob_labels, offsets, feats, coords, gt, weight,
                 voxel_scale=50):
    """criterion.py:235-331 in plain torch on the device, as a consumer writes it today."""
    B, Q, C = cls_logits.shape
    total = [torch.zeros((), device=cls_logits.device) for _ in range(7)]
    for b in range(B):
        rows, x_all = gt["row_indices"][b], mask_logits[b]
        if x_all is None or rows is None:
            continue
        s0, s1 = offsets[b], offsets[b + 1]
        x, conf, boxp = x_all[rows], conf_logits[b][rows], box_preds[b][rows]
        t, cls, boxl, w = gt["inst_labels"][b], gt["cls_labels"][b], gt["box_labels"][b], prob_labels[s0:s1]
        n = len(rows)
        sig = x.sigmoid()
        dice = (1 - (2 * (sig * t).sum(1) + 1) / (sig.sum(-1) + t.sum(-1) + 1)).sum() / (n + 1e-6)
        bce = F.binary_cross_entropy_with_logits(x, t, reduction="none")
        bce = ((bce * w).sum() / w.sum()).sum() / (n + 1e-6)
        with torch.no_grad():
            hit = x.sigmoid() >= 0.5
            inter = (hit * t).sum(-1)
            iou = inter / (hit.sum(-1) + t.sum(-1) - inter + 1e-6)
        target = torch.ones(Q, dtype=torch.int64, device=x.device) * (C - 1)
        target[rows] = cls
        parts = (dice, bce, F.cross_entropy(cls_logits[b], target, weight, reduction="mean"),
                 F.mse_loss(conf, iou, reduction="sum") / n,
                 (voxel_scale / 50.0) * F.l1_loss(boxp, boxl, reduction="sum") / n,
                 torch.sum(1 - giou_pairs(boxp, boxl)) / n, torch_levelset(coords[s0:s1], feats[s0:s1], x, boxl))
        total = [a + p for a, p in zip(total, parts)]
    return dict(zip(consumer_ops.LOSS_NAMES, (v / B for v in total)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--instances", type=int, default=40, help="matched instances per sample")
    ap.add_argument("--spps", type=int, default=1500, help="superpoints (columns) per sample")
    ap.add_argument("--feats", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=1.0, help="timed window per form and block")
    ap.add_argument("--blocks", type=int, default=2, help="alternating blocks per form")
    ap.add_argument("--count-launches", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_losses needs the GPU: a CPU run gives no time")
    dev = torch.device("cuda", 0)
    step, gt = make_step(args.batch, args.queries, args.instances, args.spps, args.feats)
    d = {k: (v if k == "batch_offsets" else [torch.from_numpy(a).to(dev) for a in v] if isinstance(v, list)
             else torch.from_numpy(v).to(dev)) for k, v in step.items()}
    gt_d = {k: [a if k == "row_indices" else torch.from_numpy(a).to(dev) for a in v] for k, v in gt.items()}
    rows_d = {**gt_d, "row_indices": [torch.from_numpy(a).to(dev) for a in gt["row_indices"]]}  # the torch chain's gathers
    weight = torch.ones(d["cls_logits"].shape[2], device=dev)
    weight[-1] = 0.1
    leaves = [d["cls_logits"], d["conf_logits"], d["box_preds"]] + d["mask_logits"]
    for t in leaves:
        t.requires_grad_()
    order = ("cls_logits", "mask_logits", "conf_logits", "box_preds", "prob_labels", "batch_offsets", "levelset_feats",
             "levelset_coords")
    common = tuple(d[k] for k in order)

    def step_of(losses_fn):
        def call():
            for t in leaves:
                t.grad = None
            out = losses_fn()
            sum(w * out[k] for w, k in zip(WEIGHTS, consumer_ops.LOSS_NAMES)).backward()
            return out
        return call

    forms = {"matched_losses": step_of(lambda: consumer_ops.matched_losses(*common, gt_d, empty_weight=weight)),
             "matched_losses_nocheck": step_of(lambda: consumer_ops.matched_losses(*common, gt_d, empty_weight=weight,
                                                                                   check=False)),
             "torch_losses": step_of(lambda: torch_losses(*common, rows_d, weight))}
    results = {}
    for k in ("matched_losses", "torch_losses"):
        out = forms[k]()
        results[k] = ([float(out[n].detach()) for n in consumer_ops.LOSS_NAMES], [t.grad.double().clone() for t in leaves])
    worst = max(abs(a - b) / max(abs(a), 1e-12) for a, b in zip(*(results[k][0] for k in results)))
    for a, b in zip(*(results[k][1] for k in results)):
        worst = max(worst, float((a - b).abs().max() / a.abs().max().clamp(min=1e-30)))
    assert worst < 1e-4, worst

    out = {"batch": args.batch, "queries": args.queries, "instances_per_sample": args.instances,
           "spps_per_sample": args.spps, "feats": args.feats, "max_relative_difference": worst}
    if args.count_launches:
        from torch.profiler import ProfilerActivity, profile

        for k, fn in forms.items():
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            out[k + "_kernels"] = int(sum(e.count for e in prof.key_averages()
                                          if "memcpy" not in e.key.lower() and "memset" not in e.key.lower()))
            print("%-24s %5d device kernels per call" % (k, out[k + "_kernels"]))
    times = {k: [] for k in forms}
    for _ in range(args.blocks):
        for k, fn in forms.items():
            times[k] += timed(fn, args.seconds)
    for k, t in times.items():
        t = np.asarray(t)
        print("%-24s %9.3f ms per call (median of %d; %.3f .. %.3f)" % (k, np.median(t), len(t), t.min(), t.max()))
        out[k + "_ms"] = {"median": float(np.median(t)), "min": float(t.min()), "max": float(t.max()), "calls": len(t)}
    out["speedup"] = out["torch_losses_ms"]["median"] / out["matched_losses_ms"]["median"]
    out["speedup_nocheck"] = out["torch_losses_ms"]["median"] / out["matched_losses_nocheck_ms"]["median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
