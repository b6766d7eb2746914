#!/usr/bin/env python3
"""Time the superpoint pooling (``consumer_ops.superpoint_plan`` and ``superpoint_pool``) at the stand-in step shape: 12
samples of 200 000 points, 551 188 voxels, 1500 superpoints a sample, per-voxel features of C = 32 and C = 3 channels
pooled through the point-to-voxel map as SPFormer's ``extract_feat`` does; and once more with one superpoint of 20 000
points in every sample (a floor), where the serial sum of an output is longest.

    python tools/bench_spp_pool.py [--samples 12] [--points 200000] [--voxels 551188] [--spps 1500] [--seconds 1.0]

Reported, each as a median: the plan build (with and without its status read), the forward and the forward plus
backward of the mean and of the max.  Beside them, in the same run, the torch statement on the same device: the gather
``x[v2p]``, then ``index_add_`` + ``bincount`` + a division, or ``scatter_reduce_("amax", include_self=False)`` plus an
arg pass, its backward by autograd -- floating-point atomics in an undefined order, so a timing yardstick only -- and
ISBNet's per-sample ``torch.unique`` loop beside the plan's ``spp_batch_offsets``.  A call is timed between two HIP events
and contains whatever host reads it makes.  One JSON line at the end.  Needs the GPU.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def scene(rng, B, n_points, n_voxels, n_spps, floor):
    """Per point its voxel (every voxel is read) and its superpoint, a voxel lying in one superpoint; ``floor`` points of
    every sample are one superpoint.  Ids are not shared between samples."""
    per_voxels = np.full(B, n_voxels // B)
    per_voxels[: n_voxels - per_voxels.sum()] += 1
    v2p, spps, v0 = [], [], 0
    for b in range(B):
        m = int(per_voxels[b])
        vox = np.concatenate([np.arange(m), rng.integers(0, m, n_points - m)])
        voxel_spp = rng.integers(0, n_spps, m)
        if floor:
            voxel_spp[rng.permutation(m)[: floor * m // n_points]] = 0
        vox = vox[rng.permutation(n_points)]
        v2p.append(v0 + vox)
        spps.append(b * n_spps + voxel_spp[vox])
        v0 += m
    return np.concatenate(v2p).astype(np.int32), np.concatenate(spps).astype(np.int64)


def torch_mean(x, v2p, spps, S):
    sums = torch.zeros((S, x.shape[1]), dtype=torch.float32, device=x.device).index_add_(0, spps, x[v2p])
    return sums / torch.bincount(spps, minlength=S).clamp(min=1)[:, None].float()


def torch_max(x, v2p, spps, S):
    rows = x[v2p]
    idx = spps[:, None].expand_as(rows)
    out = torch.zeros((S, x.shape[1]), dtype=torch.float32, device=x.device).scatter_reduce_(
        0, idx, rows, "amax", include_self=False)
    point = torch.arange(len(spps), device=x.device)[:, None].expand_as(rows)
    cand = torch.where(rows.detach() == out.detach()[spps], point, len(spps))
    arg = torch.full((S, x.shape[1]), len(spps), dtype=torch.int64, device=x.device).scatter_reduce_(
        0, idx, cand, "amin", include_self=True)
    return out, arg


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--samples", type=int, default=12)
    ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--voxels", type=int, default=551188)
    ap.add_argument("--spps", type=int, default=1500)
    ap.add_argument("--floor", type=int, default=20000)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--channels", type=int, nargs="+", default=[32, 3])
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    from gapro_amd import consumer_ops as ops

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(args.seed)
    B, S, R, N = args.samples, args.samples * args.spps, args.voxels, args.samples * args.points
    res = {"shape": {"samples": B, "points": N, "voxels": R, "superpoints": S}}
    for label, floor in (("step", 0), ("floor_%d" % args.floor, args.floor)):
        h_v2p, h_spps = scene(rng, B, args.points, R, args.spps, floor)
        v2p, spps = torch.from_numpy(h_v2p).to(dev), torch.from_numpy(h_spps).to(dev)
        v2p_long = v2p.long()
        offsets = torch.arange(B + 1, device=dev) * args.points
        h_offsets = offsets.tolist()
        build = lambda check=False: ops.superpoint_plan(spps, n_spps=S, point_map=v2p, n_rows=R,  # noqa: E731
                                                        batch_offsets=offsets, check=check)
        plan = build(True)

        def unique_loop():
            out = [0]
            for b in range(B):
                out.append(out[-1] + len(torch.unique(spps[h_offsets[b]:h_offsets[b + 1]])))
            return torch.tensor(out, dtype=torch.long, device=dev)

        assert torch.equal(unique_loop(), plan.spp_batch_offsets)
        r = {"largest_segment": int(plan.counts.max()), "plan": timed(build, args.seconds),
             "plan_check": timed(lambda: build(True), args.seconds),
             "plan_no_map": timed(lambda: ops.superpoint_plan(spps, n_spps=S, batch_offsets=offsets, check=False),
                                  args.seconds),
             "torch_unique_loop": timed(unique_loop, args.seconds, warmup=1)}
        print("%s: largest segment %d  plan %.3f ms (check=True %.3f ms, without a map %.3f ms)  torch.unique loop "
              "%.3f ms" % (label, r["largest_segment"], r["plan"]["median_ms"], r["plan_check"]["median_ms"],
                           r["plan_no_map"]["median_ms"], r["torch_unique_loop"]["median_ms"]), flush=True)
        for Cn in args.channels:
            x = torch.from_numpy(rng.standard_normal((R, Cn)).astype(np.float32)).to(dev).requires_grad_(True)
            g = torch.from_numpy(rng.standard_normal((S, Cn)).astype(np.float32)).to(dev)
            ours = {"mean": lambda t: ops.superpoint_pool(t, plan, "mean"),
                    "max": lambda t: ops.superpoint_pool(t, plan, "max")}
            theirs = {"mean": lambda t: torch_mean(t, v2p_long, spps, S),
                      "max": lambda t: torch_max(t, v2p_long, spps, S)[0]}
            close = torch.allclose(ours["mean"](x), theirs["mean"](x), rtol=1e-3, atol=1e-4)
            o, a = ops.superpoint_pool(x, plan, "max", return_arg=True)
            to, ta = torch_max(x, v2p_long, spps, S)
            assert close and torch.equal(o, to) and torch.equal(a, ta), "the two statements disagree"
            for reduce in ("mean", "max"):
                def both(fn):
                    x.grad = None
                    fn(x).backward(g)

                t = {"forward": timed(lambda: ours[reduce](x.detach()), args.seconds),
                     "forward_backward": timed(lambda: both(ours[reduce]), args.seconds),
                     "plan_forward_backward": timed(lambda: (build(), both(ours[reduce])), args.seconds),
                     "torch_forward": timed(lambda: theirs[reduce](x.detach()), args.seconds, warmup=1),
                     "torch_forward_backward": timed(lambda: both(theirs[reduce]), args.seconds, warmup=1)}
                r["C%d_%s" % (Cn, reduce)] = t
                print("%s C = %2d %-4s forward %8.3f ms  forward + backward %8.3f ms  (with the plan %8.3f ms)   torch "
                      "forward %8.3f ms  forward + backward %8.3f ms"
                      % ((label, Cn, reduce) + tuple(t[k]["median_ms"] for k in (
                          "forward", "forward_backward", "plan_forward_backward", "torch_forward",
                          "torch_forward_backward"))), flush=True)
        res[label] = r
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
