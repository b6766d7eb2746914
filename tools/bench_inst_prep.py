#!/usr/bin/env python3
"""Time ``consumer_ops.prepare_instance_labels`` against a plain torch restatement of the two loops it replaces
(get_cropped_instance_label followed by get_instance_info: one pass per instance id, host reads in between), on the
same device, in the same run, on synthetic voxel labels.

    python tools/bench_inst_prep.py [--voxels 250000] [--instances 200] [--missing 0.1] [--seconds 1.0]

A call is timed between two HIP events on the stream; a call contains its one host read (both forms do: the loops
read the device every iteration), so these are call times, not kernel times.  Each form is warmed up, then called in
alternating blocks until it has filled its window; the median, minimum and maximum of the per-call times are printed
and one JSON line.  The results of the two forms are compared first (everything equal, centroid offsets within float32
rounding of the coordinates' scale).  Needs the GPU: there is no CPU timing.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gapro_amd import consumer_ops  # noqa: E402


def make_labels(voxels, instances, missing, seed=0):
    """Voxel-like input: a batch of four scenes' worth of blobs on a 2 cm grid, ids with a share of holes, -100 stuff."""
    rng = np.random.default_rng(seed)
    n_ids = int(round(instances / (1.0 - missing)))
    used = np.sort(rng.permutation(n_ids)[:instances])
    used[-1] = n_ids - 1
    inst = used[rng.integers(0, instances, voxels)]
    centres = rng.uniform(0.5, 7.5, (n_ids, 3))
    xyz = np.rint((centres[inst] + rng.normal(0, 0.4, (voxels, 3))) * 50) / 50
    sem = (inst % 18 + 2).astype(np.int64)
    inst = inst.astype(np.int64)
    stuff = rng.random(voxels) < 0.25
    inst[stuff] = -100
    sem[stuff] = rng.integers(0, 2, int(stuff.sum()))
    return xyz.astype(np.float32), inst, sem


def torch_loops(coords, inst, sem, label_shift):
    """The two loops in plain torch on the device, as a consumer writes them today."""
    inst = inst.clone()
    j = 0
    while j < inst.max():
        if (inst == j).sum() == 0:
            inst[inst == inst.max()] = j
        j += 1
    num = int(inst.max()) + 1
    cen = torch.full((coords.shape[0], 3), -100.0, dtype=coords.dtype, device=coords.device)
    cor = torch.full((coords.shape[0], 6), -100.0, dtype=coords.dtype, device=coords.device)
    cls, box, cnt = [], [], []
    for i in range(num):
        idx = torch.nonzero(inst == i).view(-1)
        p = coords[idx]
        lo, hi = p.min(dim=0)[0], p.max(dim=0)[0]
        cen[idx] = p.mean(dim=0) - p
        cor[idx, 0:3] = lo - p
        cor[idx, 3:6] = hi - p
        box.append(torch.cat([lo, hi]))
        cnt.append(len(idx))
        cls.append(sem[idx[0]])
    cls = torch.stack(cls)
    cls[cls != -100] -= label_shift
    return inst, cls, torch.stack(box), torch.tensor(cnt, dtype=torch.int32, device=coords.device), cen, cor


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
    ap.add_argument("--voxels", type=int, default=250000)
    ap.add_argument("--instances", type=int, default=200)
    ap.add_argument("--missing", type=float, default=0.1)
    ap.add_argument("--seconds", type=float, default=1.0, help="timed window per form and block")
    ap.add_argument("--blocks", type=int, default=2, help="alternating blocks per form")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_inst_prep needs the GPU: a CPU run gives no time")
    dev = torch.device("cuda", 0)
    xyz, inst, sem = make_labels(args.voxels, args.instances, args.missing)
    coords, inst_d, sem_d = (torch.from_numpy(a).to(dev) for a in (xyz, inst, sem))

    got = consumer_ops.prepare_instance_labels(coords, inst_d, sem_d, 2)
    want = torch_loops(coords, inst_d, sem_d, 2)
    for name, g, w in zip(got._fields, got, want):
        if name == "centroid_offset_labels":
            err = float((g.double() - w.double()).abs().max())
            assert err <= 8 * float(np.spacing(np.float32(np.abs(xyz).max()))), err
        else:
            assert torch.equal(g, w.to(g.dtype)), name
    n_inst = int(got.instance_cls.shape[0])

    forms = {"prepare_instance_labels": lambda: consumer_ops.prepare_instance_labels(coords, inst_d, sem_d, 2),
             "torch_loops": lambda: torch_loops(coords, inst_d, sem_d, 2)}
    times = {k: [] for k in forms}
    for _ in range(args.blocks):
        for k, fn in forms.items():
            times[k] += timed(fn, args.seconds)
    out = {"voxels": args.voxels, "instances": n_inst, "ids_missing": args.missing, "centroid_max_abs_diff": err}
    for k, t in times.items():
        t = np.asarray(t)
        print("%-24s %9.3f ms per call (median of %d; %.3f .. %.3f)" % (k, np.median(t), len(t), t.min(), t.max()))
        out[k + "_ms"] = {"median": float(np.median(t)), "min": float(t.min()), "max": float(t.max()), "calls": len(t)}
    out["speedup_median"] = out["torch_loops_ms"]["median"] / out["prepare_instance_labels_ms"]["median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
