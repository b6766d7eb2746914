#!/usr/bin/env python3
"""Time ``consumer_ops.get_instance`` against a plain torch statement of the chain it replaces (softmax and top-k, a
float einsum of the masks, matrix or greedy NMS, a scatter mean of the devoxelised masks, and a run-length loop with one
``nonzero`` and one blocking copy per instance), on the same device, in the same run, on one synthetic scene of the
consumer's step shape.

    python tools/bench_proposals.py [--queries 384] [--classes 18] [--voxels 100000] [--points 150000] [--spps 2500]
                                    [--topk 100] [--seconds 1.0] [--config matrix-spp]

Without ``--config`` the four configurations (matrix / standard NMS x mask_logits per superpoint / per voxel) each run
in a child process of their own under a time limit.  A call is timed between two HIP events on the stream and contains
its host reads and the building of the list of dicts, so these are call times, not kernel times.  Each form is warmed
up, then called in alternating blocks until it has filled its window; the median, minimum and maximum of the per-call
times are printed and one JSON line.  With ``mask_logits`` per superpoint the torch form pays for the expansion
``mask_logits[:, voxel_spps]`` the reference does before the chain.  The two results are compared first: the same
instances (labels and run lengths, order-free), conf within 2e-6 relative.  Needs the GPU: there is no CPU timing.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CONFIGS = ("matrix-spp", "matrix-voxel", "standard-spp", "standard-voxel")
CHILD_LIMIT = 240  # seconds a configuration's process may take


def torch_chain(scan_id, cls_logits, mask_logits, conf_logits, v2p, spps, C, npoint_thresh, type_nms, topk, thr):
    """The chain in plain torch, as the consumer runs it: every step a library call, the loops on the host."""
    scores = torch.sqrt(torch.softmax(cls_logits, dim=-1)[:, :-1] * conf_logits.clamp(0.0, 1.0)[:, None]).reshape(-1)
    masks = mask_logits >= 0.0
    top, idx = torch.topk(scores, k=min(300, scores.numel()))
    q = torch.div(idx, C, rounding_mode="floor")
    cat, m = idx % C, masks[q]
    ok = m.sum(1) >= npoint_thresh
    cat, m, top = cat[ok], m[ok], top[ok]
    f = m.float()
    inter = f @ f.T
    n = f.sum(1)
    iou = inter / (n[None, :] + n[:, None] - inter)
    same = (cat[None, :] == cat[:, None])
    if type_nms == "matrix":
        d = iou * same.float().triu(1)
        comp = d.max(0).values
        coef = (torch.exp(-2 * d ** 2) / torch.exp(-2 * comp ** 2)[:, None]).min(0).values
        new = top * coef
        keep = torch.topk(new, k=min(topk, new.numel())).indices
        top = new[keep]
    else:
        ixs, pick = torch.arange(len(top), device=top.device), []
        while len(ixs) > 0:
            i = ixs[0]
            pick.append(i)
            hit = (iou[i, ixs] > thr) & same[i, ixs]
            hit[0] = True
            ixs = ixs[~hit]
        keep = torch.stack(pick) if pick else ixs
        top = top[keep]
    cat, m = cat[keep], m[keep]
    pts = m[:, v2p].float()
    n_spp = int(spps.max()) + 1
    total = torch.zeros((pts.shape[0], n_spp), device=pts.device).index_add_(1, spps, pts)
    count = torch.zeros(n_spp, device=pts.device).index_add_(0, spps, torch.ones_like(spps, dtype=torch.float32))
    pts = ((total / count.clamp(min=1)) >= 0.5)[:, spps]
    ok = pts.sum(1) >= npoint_thresh
    pts, top, cat = pts[ok], top[ok].cpu().numpy(), cat[ok].cpu().numpy()
    zero = torch.zeros((pts.shape[0], 1), dtype=torch.bool, device=pts.device)
    padded = torch.cat([zero, pts, zero], dim=1)
    out = []
    for i in range(pts.shape[0]):
        runs = torch.nonzero(padded[i, 1:] != padded[i, :-1]).view(-1) + 1
        runs[1::2] -= runs[::2]
        out.append({"scan_id": scan_id, "label_id": cat[i] + 1, "conf": top[i],
                    "pred_mask": {"length": pts.shape[1], "counts": runs.cpu().numpy()}})
    return out


def _key(g):
    return int(g["label_id"]), np.asarray(g["pred_mask"]["counts"], np.int64).tobytes()


def run_config(args):
    import proposals_cases

    from gapro_amd import consumer_ops

    type_nms, form = args.config.split("-")
    dev = torch.device("cuda:0")
    c = proposals_cases.make_scene(args.seed, Q=args.queries, C=args.classes, V=args.voxels, N=args.points, S=args.spps,
                                   n_inst=args.instances)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in c.items() if isinstance(v, np.ndarray)}
    wide = t["mask_logits"][:, t["voxel_spps"]].contiguous()
    npoint = args.npoint_thresh

    def ours():
        spp = form == "spp"
        return consumer_ops.get_instance(
            "scene", t["cls_logits"], t["mask_logits"] if spp else wide, t["conf_logits"], t["box_preds"], t["v2p_map"],
            None, t["spps"], 0.0, 0.1, npoint, instance_classes=args.classes, type_nms=type_nms, topk=args.topk,
            nms_threshold=0.2, voxel_spps=t["voxel_spps"] if spp else None, n_spps=args.spps)

    def theirs():
        ml = t["mask_logits"][:, t["voxel_spps"]] if form == "spp" else wide
        return torch_chain("scene", t["cls_logits"], ml, t["conf_logits"], t["v2p_map"], t["spps"], args.classes, npoint,
                           type_nms, args.topk, 0.2)

    a, b = sorted(ours(), key=_key), sorted(theirs(), key=_key)
    agree = len(a) == len(b) and all(_key(x) == _key(y) for x, y in zip(a, b))
    conf_dev = max([abs(float(x["conf"]) - float(y["conf"])) / float(y["conf"]) for x, y in zip(a, b)] or [0.0]) \
        if agree else float("nan")
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
    res = {"config": args.config, "instances": len(a), "agree": bool(agree), "conf_deviation": conf_dev,
           "shape": {"queries": args.queries, "classes": args.classes, "voxels": args.voxels, "points": args.points,
                     "spps": args.spps, "topk": args.topk, "npoint_thresh": npoint}}
    for name, v in times.items():
        v = np.asarray(v)
        res[name] = {"calls": len(v), "median_ms": float(np.median(v)), "min_ms": float(v.min()), "max_ms": float(v.max())}
        print("%-14s %-5s %4d calls  median %8.3f ms  min %8.3f  max %8.3f"
              % (args.config, name, len(v), res[name]["median_ms"], res[name]["min_ms"], res[name]["max_ms"]))
    res["speedup_median"] = res["torch"]["median_ms"] / res["ours"]["median_ms"]
    print(json.dumps(res))
    return 0 if agree else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--queries", type=int, default=384)
    ap.add_argument("--classes", type=int, default=18)
    ap.add_argument("--voxels", type=int, default=100000)
    ap.add_argument("--points", type=int, default=150000)
    ap.add_argument("--spps", type=int, default=2500)
    ap.add_argument("--instances", type=int, default=40)
    ap.add_argument("--topk", type=int, default=100)
    ap.add_argument("--npoint-thresh", type=int, default=100)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--config", choices=CONFIGS)
    args = ap.parse_args()
    if args.config:
        return run_config(args)
    rc = 0
    for config in CONFIGS:  # a process and a time limit each
        cmd = [sys.executable, os.path.abspath(__file__), "--config", config] + [a for a in sys.argv[1:]]
        try:
            rc |= subprocess.run(cmd, timeout=CHILD_LIMIT).returncode
        except subprocess.TimeoutExpired:
            print("%s: no result within %d s" % (config, CHILD_LIMIT))
            return 1
        if rc:
            return rc
    return rc


if __name__ == "__main__":
    sys.exit(main())
