#!/usr/bin/env python3
"""Time ``consumer_ops.spformer_predict`` against a plain torch statement of the chain it replaces
(``SPFormer.predict_by_feat``: softmax and top-k, the ``[topk_insts, N]`` expansion of the superpoint masks, three
boolean compactions, a run-length loop with one ``nonzero`` and one blocking copy per instance, and a box loop with a
boolean gather, two reductions and another blocking copy per instance), on the same device, in the same run, on one
synthetic scene at the released configuration.

    python tools/bench_spf_predict.py [--queries 400] [--classes 18] [--spps 1500] [--points 200000] [--topk 100]
                                      [--score-thr 0.0] [--npoint-thr 100] [--seconds 2.0]

A call is timed between two HIP events on the stream and contains its host reads and the building of the list of dicts,
so these are call times, not kernel times.  Each form is warmed up, then called in alternating blocks until it has filled
its window; the median, minimum and maximum of the per-call times are printed and one JSON line.  The two results are
compared first: the same instances (labels, run lengths and boxes, order-free), conf within 2e-6 relative.  Needs the
GPU: there is no CPU timing.
"""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def torch_chain(scan_id, pred_labels, pred_scores, pred_masks, superpoints, coords_float, C, topk, score_thr, npoint_thr):
    """The chain in plain torch, as the consumer runs it: every step a library call, the loops on the host."""
    scores = torch.softmax(pred_labels, dim=-1)[:, :-1] * pred_scores[:, None]
    labels = torch.arange(C, device=scores.device).repeat(pred_labels.shape[0])
    scores, idx = scores.reshape(-1).topk(min(topk, scores.numel()), sorted=False)
    labels = labels[idx] + 1
    logits = pred_masks[torch.div(idx, C, rounding_mode="floor")]
    on = (logits > 0).float()
    scores = scores * ((logits.sigmoid() * on).sum(1) / (on.sum(1) + 1e-6))
    masks = on[:, superpoints].int()
    keep = scores > score_thr
    scores, labels, masks = scores[keep], labels[keep], masks[keep]
    keep = masks.sum(1) > npoint_thr
    scores, labels, masks = scores[keep], labels[keep], masks[keep]
    cls, conf = labels.cpu().numpy(), scores.cpu().numpy()
    zero = torch.zeros((masks.shape[0], 1), dtype=masks.dtype, device=masks.device)
    padded = torch.cat([zero, masks, zero], dim=1)
    out = []
    for i in range(masks.shape[0]):
        runs = torch.nonzero(padded[i, 1:] != padded[i, :-1]).view(-1) + 1
        runs[1::2] -= runs[::2]
        xyz = coords_float[masks[i].bool(), :]
        box = torch.cat([xyz.min(dim=0)[0], xyz.max(dim=0)[0]]).cpu().numpy()
        out.append({"scan_id": scan_id, "label_id": cls[i], "conf": conf[i],
                    "pred_mask": {"length": masks.shape[1], "counts": runs.cpu().numpy()}, "box": box})
    return out


def _key(g):
    return int(g["label_id"]), np.asarray(g["pred_mask"]["counts"], np.int64).tobytes()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--queries", type=int, default=400)
    ap.add_argument("--classes", type=int, default=18)
    ap.add_argument("--spps", type=int, default=1500)
    ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--instances", type=int, default=40)
    ap.add_argument("--topk", type=int, default=100)
    ap.add_argument("--score-thr", type=float, default=0.0)
    ap.add_argument("--npoint-thr", type=int, default=100)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    import spf_predict_cases

    from gapro_amd import consumer_ops

    dev = torch.device("cuda:0")
    c = spf_predict_cases.make_scene(args.seed, Q=args.queries, C=args.classes, S=args.spps, N=args.points,
                                     n_inst=args.instances)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in c.items() if isinstance(v, np.ndarray)}
    out = {"labels": t["labels"][None], "scores": t["pred_scores"][None, :, None], "masks": [t["masks"]]}
    insts = [types.SimpleNamespace(gt_instances=None)]
    cfg = types.SimpleNamespace(topk_insts=args.topk, score_thr=args.score_thr, npoint_thr=args.npoint_thr)

    def ours():
        return consumer_ops.spformer_predict(["scene"], out, t["superpoints"], insts, t["coords_float"],
                                             num_class=args.classes, test_cfg=cfg)["pred_instances"]

    def theirs():
        return torch_chain("scene", out["labels"][0], out["scores"][0, :, 0], out["masks"][0], t["superpoints"],
                           t["coords_float"], args.classes, args.topk, args.score_thr, args.npoint_thr)

    a, b = sorted(ours(), key=_key), sorted(theirs(), key=_key)
    agree = len(a) == len(b) and all(_key(x) == _key(y) and np.array_equal(x["box"], y["box"]) for x, y in zip(a, b))
    conf_dev = max([abs(float(x["conf"]) - float(y["conf"])) / abs(float(y["conf"])) for x, y in zip(a, b)] or [0.0]) \
        if agree else float("nan")
    agree = agree and conf_dev <= 2e-6
    times = {"ours": [], "torch": []}
    for _ in range(3):
        ours(), theirs()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.blocks):
        for name, fn in (("ours", ours), ("torch", theirs)):
            spent = 0.0
            while spent < args.seconds / args.blocks:
                start.record()
                fn()
                stop.record()
                stop.synchronize()
                ms = start.elapsed_time(stop)
                times[name].append(ms)
                spent += ms / 1000.0
    res = {"instances": len(a), "agree": bool(agree), "conf_deviation": conf_dev,
           "shape": {"queries": args.queries, "classes": args.classes, "spps": args.spps, "points": args.points,
                     "topk_insts": args.topk, "score_thr": args.score_thr, "npoint_thr": args.npoint_thr}}
    for name, v in times.items():
        v = np.asarray(v)
        res[name] = {"calls": len(v), "median_ms": float(np.median(v)), "min_ms": float(v.min()), "max_ms": float(v.max())}
        print("%-5s %4d calls  median %8.3f ms  min %8.3f  max %8.3f"
              % (name, len(v), res[name]["median_ms"], res[name]["min_ms"], res[name]["max_ms"]))
    res["speedup_median"] = res["torch"]["median_ms"] / res["ours"]["median_ms"]
    print(json.dumps(res))
    return 0 if agree else 1


if __name__ == "__main__":
    sys.exit(main())
