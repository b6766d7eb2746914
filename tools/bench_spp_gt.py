#!/usr/bin/env python3
"""Time ``consumer_ops.get_spp_gt`` and ``get_subsample_gt`` against a plain torch statement of the loops they replace
(per sample two ``unique``s and a filter, then per instance id one scatter mean, one compare and one row write, the id
read from the device every iteration), on the same device, in the same run, on synthetic input of ISBNet's step shape.

    python tools/bench_spp_gt.py [--batch 4] [--voxels 60000] [--spps 1500] [--instances 40] [--seconds 1.0] [--shuffle]

A call is timed between two HIP events on the stream; a call contains its host reads (one for the device form, one per
instance id and more for the loops), so these are call times, not kernel times.  Each form is warmed up, then called in
alternating blocks until it has filled its window; the median, minimum and maximum of the per-call times are printed
and one JSON line.  The results of the two forms are compared for equality first.  ``--shuffle`` permutes the points
of every sample, so that no two neighbouring lanes share a superpoint: the worst case of the tally's lane combining.
Needs the GPU: there is no CPU timing.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gapro_amd import consumer_ops  # noqa: E402


def make_batch(batch, voxels, spps, instances, ignored=0.25, negative=3, shuffle=False, seed=0):
    """Per sample voxels / batch points in runs of one superpoint each, most of a run in one instance; instance and
    superpoint ids run on over the batch, as ISBNet's collate function hands them out."""
    rng = np.random.default_rng(seed)
    n = voxels // batch
    labels, spp_ids, off = [], [], [0]
    for b in range(batch):
        cuts = np.sort(rng.permutation(np.arange(1, n))[:spps - 1])
        run = np.repeat(np.arange(spps), np.diff(np.r_[0, cuts, n]))
        lab = (rng.integers(0, instances, spps) + b * instances)[run]
        noise = rng.random(n) < 0.1
        lab[noise] = rng.integers(0, instances, int(noise.sum())) + b * instances
        lab[rng.random(n) < ignored] = -100
        spp = rng.permutation(spps)[run] + b * spps
        if shuffle:
            p = rng.permutation(n)
            lab, spp = lab[p], spp[p]
        labels.append(lab)
        spp_ids.append(spp)
        off.append(off[-1] + n)
    cls = rng.integers(0, 18, batch * instances).astype(np.int64)
    cls[rng.permutation(len(cls))[:negative]] = -100
    box = rng.uniform(0, 8, (len(cls), 6)).astype(np.float32)
    return (np.concatenate(labels).astype(np.int64), np.concatenate(spp_ids).astype(np.int64), cls, box,
            np.asarray(off, dtype=np.int64))


def _rows(lab, cls, ignore):
    ids = torch.unique(lab)
    ids = ids[ids != ignore]
    return ids[cls[ids] >= 0]


def torch_spp_gt(labels, spps, cls, box, offsets, batch_size, ignore=-100):
    """The loops in plain torch on the device, as a consumer writes them today."""
    out = []
    for b in range(batch_size):
        lab, spp = labels[offsets[b]:offsets[b + 1]], spps[offsets[b]:offsets[b + 1]]
        cols, inv = torch.unique(spp, return_inverse=True)
        ids = _rows(lab, cls, ignore)
        if len(ids) == 0:
            out.append(None)
            continue
        count = torch.zeros(len(cols), dtype=torch.float32, device=lab.device).index_add_(
            0, inv, torch.ones(len(inv), dtype=torch.float32, device=lab.device)).clamp_(min=1)
        mask = torch.zeros((len(ids), len(cols)), dtype=torch.float32, device=lab.device)
        for i, uid in enumerate(ids):
            hit = (lab == uid).float()
            mean = torch.zeros(len(cols), dtype=torch.float32, device=lab.device).index_add_(0, inv, hit) / count
            mask[i] = (mean >= 0.5).float()
        out.append({"mask": mask, "cls": cls[ids], "box": box[ids]})
    return out


def torch_subsample_gt(labels, idxs, cls, box, offsets, batch_size, ignore=-100):
    sub = labels[idxs]
    out = []
    for b in range(batch_size):
        lab = sub[offsets[b]:offsets[b + 1]]
        ids = _rows(lab, cls, ignore)
        if len(ids) == 0:
            out.append(None)
            continue
        mask = torch.zeros((len(ids), len(lab)), dtype=torch.float32, device=lab.device)
        for i, uid in enumerate(ids):
            mask[i] = (lab == uid).float()
        out.append({"mask": mask, "cls": cls[ids], "box": box[ids]})
    return out


def same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g is None) == (w is None)
        if g is not None:
            for k in ("mask", "cls", "box"):
                assert g[k].dtype == w[k].dtype and torch.equal(g[k], w[k]), k


def timed(fn, seconds, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times, total = [], 0.0
    while total < seconds * 1e3 or len(times) < 3:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
        total += times[-1]
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--voxels", type=int, default=60000, help="points of the whole batch")
    ap.add_argument("--spps", type=int, default=1500, help="superpoints per sample")
    ap.add_argument("--instances", type=int, default=40, help="instances per sample")
    ap.add_argument("--subsample", type=int, default=20000, help="subsampled points of the whole batch")
    ap.add_argument("--shuffle", action="store_true", help="permute the points of every sample")
    ap.add_argument("--seconds", type=float, default=1.0, help="timed window per form and block")
    ap.add_argument("--blocks", type=int, default=2, help="alternating blocks per form")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_spp_gt needs the GPU: a CPU run gives no time")
    dev = torch.device("cuda", 0)
    B = args.batch
    labels, spps, cls, box, off = make_batch(B, args.voxels, args.spps, args.instances, shuffle=args.shuffle)
    rng = np.random.default_rng(1)
    per = args.subsample // B
    idxs = np.concatenate([np.sort(rng.permutation(np.arange(off[b], off[b + 1]))[:per]) for b in range(B)])
    sub_off = np.arange(B + 1, dtype=np.int64) * per
    n_spps = B * args.spps
    lab_d, spp_d, cls_d, box_d, off_d, idx_d, sub_off_d = (torch.from_numpy(a).to(dev)
                                                           for a in (labels, spps, cls, box, off, idxs, sub_off))

    forms = {
        "get_spp_gt": lambda: consumer_ops.get_spp_gt(lab_d, spp_d, cls_d, box_d, off_d, B, n_spps=n_spps),
        "torch_spp_gt": lambda: torch_spp_gt(lab_d, spp_d, cls_d, box_d, off_d, B),
        "get_subsample_gt": lambda: consumer_ops.get_subsample_gt(lab_d, idx_d, cls_d, box_d, sub_off_d, B),
        "torch_subsample_gt": lambda: torch_subsample_gt(lab_d, idx_d, cls_d, box_d, sub_off_d, B),
    }
    same(forms["get_spp_gt"](), forms["torch_spp_gt"]())
    same(forms["get_subsample_gt"](), forms["torch_subsample_gt"]())

    times = {k: [] for k in forms}
    for _ in range(args.blocks):
        for k, fn in forms.items():
            times[k] += timed(fn, args.seconds)
    out = {"batch": B, "voxels": len(labels), "spps_per_sample": args.spps, "instances_per_sample": args.instances,
           "subsample": len(idxs), "shuffled": bool(args.shuffle)}
    for k, t in times.items():
        t = np.asarray(t)
        print("%-20s %9.3f ms per call (median of %d; %.3f .. %.3f)" % (k, np.median(t), len(t), t.min(), t.max()))
        out[k + "_ms"] = {"median": float(np.median(t)), "min": float(t.min()), "max": float(t.max()), "calls": len(t)}
    out["speedup_spp_gt"] = out["torch_spp_gt_ms"]["median"] / out["get_spp_gt_ms"]["median"]
    out["speedup_subsample_gt"] = out["torch_subsample_gt_ms"]["median"] / out["get_subsample_gt_ms"]["median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
