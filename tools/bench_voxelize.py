#!/usr/bin/env python3
"""Time the consumers' voxelisation (``consumer_ops.voxelization_idx`` and ``voxelization``) at the step shape: 12
samples of about 200 000 points each on synthetic planar surfaces, quantised at 2 cm so that voxels hold several points,
with C = 3 and C = 9 channels.

    python tools/bench_voxelize.py [--samples 12] [--points 200000] [--seconds 1.0] [--channels 3 9]

Reported, each as a median with the achieved GB/s against the bytes the call must move (its inputs read once, its
outputs written once): the count + fill pair with its one host read, the pooling forward, the pooling backward.  Beside
them, in the same run: (a) the host path (``voxelization_idx`` on CPU tensors, one thread) and (b) the torch formulation
on the device, ``torch.unique(coords, dim=0, return_inverse=True)`` plus ``index_add_`` -- another numbering and another
rounding, so a timing yardstick only.  A device call is timed between two HIP events and contains whatever host reads
it makes.  One JSON line at the end.  Needs the GPU.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def planar_sample(rng, n_points, voxel=0.02, planes=5, side=2.0):
    """Points on ``planes`` axis-aligned squares of ``side`` metres in a 6 x 6 x 3 m room: float32 xyz and int64 cells."""
    per = np.full(planes, n_points // planes)
    per[0] += n_points - per.sum()
    parts = []
    for k, m in enumerate(per):
        axis = k % 3
        uv = rng.uniform(0.0, side, size=(m, 2))
        origin = rng.uniform(0.0, [4.0, 4.0, 1.0])
        p = np.empty((m, 3))
        p[:, axis] = origin[axis] + rng.normal(0.0, 0.002, size=m)  # a few millimetres of sensor noise
        p[:, (axis + 1) % 3] = origin[(axis + 1) % 3] + uv[:, 0]
        p[:, (axis + 2) % 3] = origin[(axis + 2) % 3] + uv[:, 1] * (0.5 if (axis + 2) % 3 == 2 else 1.0)
        parts.append(p)
    xyz = np.concatenate(parts)[rng.permutation(n_points)].astype(np.float32)
    return xyz, np.floor(xyz / np.float32(voxel)).astype(np.int64)


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


def with_rate(t, nbytes):
    t["bytes"] = int(nbytes)
    t["gb_per_s"] = nbytes / (t["median_ms"] * 1e-3) / 1e9
    return t


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--samples", type=int, default=12)
    ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--channels", type=int, nargs="+", default=[3, 9])
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    from gapro_amd import consumer_ops as ops

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(args.seed)
    B = args.samples
    samples = [planar_sample(rng, args.points) for _ in range(B)]
    cells = np.concatenate([np.concatenate([np.full((len(c), 1), b, np.int64), c], axis=1)
                            for b, (_, c) in enumerate(samples)])
    h_coords = torch.from_numpy(cells)
    coords = h_coords.to(dev)
    N = len(cells)

    t0 = time.perf_counter()
    host = ops.voxelization_idx(h_coords, B, 4)
    host_ms = (time.perf_counter() - t0) * 1e3
    oc, v2p, p2v = ops.voxelization_idx(coords, B, 4)  # the reference's names: p2v is the table
    same = all(torch.equal(a, b.cpu()) for a, b in zip(host, (oc, v2p, p2v)))
    M, width = int(p2v.shape[0]), int(p2v.shape[1])
    res = {"shape": {"samples": B, "points": N, "voxels": M, "max_active": width - 1,
                     "points_per_voxel": N / M}, "device_equals_host": same}
    print("points %d  voxels %d  max_active %d  device == host: %s" % (N, M, width - 1, same), flush=True)

    idx_bytes = N * 4 * 8 + N * 4 + M * 4 * 8 + M * width * 4
    res["count_fill"] = with_rate(timed(lambda: ops.voxelization_idx(coords, B, 4), args.seconds), idx_bytes)
    res["host_path"] = {"median_ms": host_ms, "calls": 1}

    def torch_idx():
        uniq, inv = torch.unique(coords, dim=0, return_inverse=True)
        return uniq, inv

    res["torch_unique"] = timed(torch_idx, args.seconds, warmup=1)
    uniq, inv = torch_idx()
    print("count + fill %9.3f ms  %7.1f GB/s   host path %9.1f ms   torch.unique %9.3f ms"
          % (res["count_fill"]["median_ms"], res["count_fill"]["gb_per_s"], host_ms, res["torch_unique"]["median_ms"]),
          flush=True)

    for Cn in args.channels:
        feats = torch.from_numpy(rng.standard_normal((N, Cn)).astype(np.float32)).to(dev).requires_grad_(True)
        out = ops.voxelization(feats, p2v, 4, check=False)
        grad = torch.ones_like(out)
        table = M * width * 4
        fwd = with_rate(timed(lambda: ops.voxelization(feats.detach(), p2v, 4, check=False), args.seconds),
                        N * Cn * 4 + table + M * Cn * 4)
        checked = timed(lambda: ops.voxelization(feats.detach(), p2v, 4, check=True), args.seconds)

        def backward():
            feats.grad = None
            out.backward(grad, retain_graph=True)

        bwd = with_rate(timed(backward, args.seconds), M * Cn * 4 + table + N * Cn * 4)
        counts = torch.bincount(inv, minlength=len(uniq)).to(torch.float32)[:, None]

        def torch_pool():
            return torch.zeros((len(uniq), Cn), device=dev).index_add_(0, inv, feats.detach()) / counts

        theirs = timed(torch_pool, args.seconds, warmup=1)
        res["C%d" % Cn] = {"forward": fwd, "forward_check": checked, "backward": bwd, "torch_index_add": theirs}
        print("C = %d  forward %8.3f ms %7.1f GB/s (check=True %8.3f ms)  backward %8.3f ms %7.1f GB/s   "
              "torch index_add_ %8.3f ms" % (Cn, fwd["median_ms"], fwd["gb_per_s"], checked["median_ms"],
                                             bwd["median_ms"], bwd["gb_per_s"], theirs["median_ms"]), flush=True)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
