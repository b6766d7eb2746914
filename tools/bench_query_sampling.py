#!/usr/bin/env python3
"""Time the consumer's query sampling (``consumer_ops.furthestsampling_batchflat``, ``ballquery_batchflat``,
``ball_query``, ``sample_queries``) against a plain torch statement of the same loops, on the same device, in the same
run, at the step shape of the reference config (configs/scannetv2/boxsup_isbnet_scannetv2.yaml): 12 samples, the object
voxels (0.02 m) of 12 scenes of the project's synthetic scene generator, 2048 samples each.

    python tools/bench_query_sampling.py [--samples 12] [--n-sample 2048] [--points 150000] [--seconds 1.0]

The three ball queries are the aggregator's: batch-flat r = 0.2 with 32 neighbours, batched (12, 2048, 3) r = 0.4 with
64, and batched with 256 queries r = 0.4 / 0.8 with 32.  The torch statement of the sampling is the reference's loop
with every sample padded into one [B, N_max] batch (one arg-max and one distance update per iteration for the whole
batch); the ball query's is a distance matrix per sample, a running count of the hits and a scatter of the first
``nsample``.  A call is timed between two HIP events and contains whatever host reads it makes.  The results are
compared first and the agreement is reported, not required: torch's arg-max leaves the order of equal maxima open.
One JSON line at the end.  Needs the GPU.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def object_voxels(seed, n_points, voxel=0.02):
    from gapro_amd import synth

    sc = synth.make_scene(seed=seed, n_points=n_points)
    pts = sc.xyz[np.asarray(sc.inst) >= 0]
    cells = np.unique(np.floor(pts / voxel).astype(np.int64), axis=0)
    return (cells.astype(np.float32) * np.float32(voxel)).astype(np.float32)


def torch_fps(padded, counts, m):
    """The reference's loop over a padded [B, N, 3] batch: rows beyond a sample's count never win."""
    B, N, _ = padded.shape
    valid = torch.arange(N, device=padded.device)[None, :] < counts[:, None]
    d = torch.where(valid, torch.full((B, N), 1e10, device=padded.device), torch.full((B, N), -1.0, device=padded.device))
    idx = torch.zeros((B, m), dtype=torch.int64, device=padded.device)
    old = torch.zeros(B, dtype=torch.int64, device=padded.device)
    rows = torch.arange(B, device=padded.device)
    for s in range(1, m):
        d = torch.minimum(d, ((padded - padded[rows, old][:, None, :]) ** 2).sum(-1))
        old = torch.argmax(d, dim=1)
        idx[:, s] = old
    return idx


def torch_ball(radius, nsample, xyz, new_xyz):
    """One sample: [M, nsample] local indices, a row of zeros without a hit."""
    d2 = ((new_xyz[:, None, :] - xyz[None, :, :]) ** 2).sum(-1)
    hit = d2 < radius * radius
    rank = hit.cumsum(1)
    q, k = (hit & (rank <= nsample)).nonzero(as_tuple=True)
    out = torch.full((new_xyz.shape[0], nsample), -1, dtype=torch.int64, device=xyz.device)
    out[q, rank[q, k] - 1] = k
    first = torch.where(out[:, :1] >= 0, out[:, :1], torch.zeros_like(out[:, :1]))
    return torch.where(out >= 0, out, first)


def timed(fn, seconds, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times, spent = [], 0.0
    while spent < seconds or len(times) < 3:
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
        spent += times[-1] / 1000.0
    v = np.asarray(times)
    return {"calls": len(v), "median_ms": float(np.median(v)), "min_ms": float(v.min()), "max_ms": float(v.max())}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--samples", type=int, default=12)
    ap.add_argument("--n-sample", type=int, default=2048)
    ap.add_argument("--points", type=int, default=150000)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    from gapro_amd import consumer_ops as ops

    dev = torch.device("cuda:0")
    B, m = args.samples, args.n_sample
    scenes = [object_voxels(args.seed + b, args.points) for b in range(B)]
    counts = [len(s) for s in scenes]
    locs = torch.from_numpy(np.concatenate(scenes)).to(dev)
    off = torch.tensor(np.cumsum(counts), dtype=torch.int32, device=dev)
    off0 = torch.cat([torch.zeros(1, dtype=torch.int32, device=dev), off])
    n_max = max(counts)
    padded = torch.zeros((B, n_max, 3), device=dev)
    for b, s in enumerate(scenes):
        padded[b, :len(s)] = torch.from_numpy(s).to(dev)
    d_counts = torch.tensor(counts, device=dev)
    starts = np.concatenate([[0], np.cumsum(counts)])
    print("object voxels per sample:", counts, "paths:", sorted({ops.fps_plan(c)[0] for c in counts}))

    fps = ops.furthestsampling_batchflat(locs, off, n_sample=m, check=False)
    theirs = torch_fps(padded, d_counts, m) + torch.from_numpy(starts[:-1]).to(dev)[:, None]
    fps_agree = float((fps.view(B, m).to(torch.int64) == theirs).float().mean())
    picked = locs[fps.long()]
    batched = picked.view(B, m, 3).contiguous()
    sub = batched[:, :256].contiguous()
    res = {"shape": {"samples": B, "n_sample": m, "object_voxels": counts}, "fps_index_agreement": fps_agree}

    def flat_torch():
        return [torch_ball(0.2, 32, locs[starts[b]:starts[b + 1]], picked[b * m:(b + 1) * m]) for b in range(B)]

    def batched_torch(r, ns, q):
        return lambda: [torch_ball(r, ns, batched[b], q[b]) for b in range(B)]

    pairs = [
        ("fps", lambda: ops.furthestsampling_batchflat(locs, off, n_sample=m, check=False),
         lambda: torch_fps(padded, d_counts, m)),
        ("ball_flat_r0.2_k32", lambda: ops.ballquery_batchflat(0.2, 32, locs, picked, off, n_sample=m, check=False),
         flat_torch),
        ("ball_batched_r0.4_k64", lambda: ops.ball_query(0.4, 64, batched, batched), batched_torch(0.4, 64, batched)),
        ("ball_256q_r0.4_k32", lambda: ops.ball_query(0.4, 32, batched, sub), batched_torch(0.4, 32, sub)),
        ("ball_256q_r0.8_k32", lambda: ops.ball_query(0.8, 32, batched, sub), batched_torch(0.8, 32, sub)),
        ("sample_queries", lambda: ops.sample_queries(locs, off0, B, m, 0.2, 32, 32), None),
    ]
    for name, ours, torch_fn in pairs:
        if torch_fn is not None and name != "fps":
            a = ours()
            b = torch.cat([t.view(-1, a.shape[-1]) for t in torch_fn()])
            if name.startswith("ball_flat"):
                b = b + torch.from_numpy(np.repeat(starts[:-1], m)).to(dev)[:, None] * (b.sum(1, keepdim=True) > 0)
            res[name + "_row_agreement"] = float((a.view(-1, a.shape[-1]).to(torch.int64) == b).all(1).float().mean())
        res[name] = {"ours": timed(ours, args.seconds)}
        line = "%-24s ours  median %9.3f ms" % (name, res[name]["ours"]["median_ms"])
        if torch_fn is not None:
            res[name]["torch"] = timed(torch_fn, args.seconds, warmup=1)
            res[name]["speedup_median"] = res[name]["torch"]["median_ms"] / res[name]["ours"]["median_ms"]
            line += "   torch median %9.3f ms   x%.1f" % (res[name]["torch"]["median_ms"], res[name]["speedup_median"])
        print(line, flush=True)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
