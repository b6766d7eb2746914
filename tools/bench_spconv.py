#!/usr/bin/env python3
"""Time the sparse convolutions (``consumer_ops.subm_conv3d``, ``sparse_conv3d``, ``sparse_inverse_conv3d``) and the two
plan builds at the consumers' step shape: 12 samples and 551 188 voxels at level 1, the coarser levels from
the down plans, 32 l channels at level l, 7 levels.

    python tools/bench_spconv.py [--samples 12] [--voxels 551188] [--levels 7] [--seconds 0.5]

The scans are synthetic surfaces (random axis-aligned rectangles in a 256 x 512 x 512 grid): what matters to the kernels is
the share of the 27 offsets that is occupied, which is printed.  Per level and layer, each a median between two HIP
events after two warm-up calls: the forward, the forward plus backward (gradients of the features and the weight), and
beside them, in the same run, a torch statement on the same device of the native loop over the same rulebook -- per
offset a gather, an ``mm`` and an ``index_add_``, float32, backward by autograd -- which is the only baseline there is
(spconv has no build for this GPU); the two are compared first.  FLOP/s are 2 C_in C_out a (row, offset) pair; bytes/s
are the pairs' gathered rows, the output rows and the table over the forward's time, against the 6.3 TB/s a stream
achieves.  One JSON line at the end.  Needs the GPU.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12


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


def surface_scan(rng, target, shape):
    """``target`` distinct voxels of random axis-aligned rectangles (walls, floors, the faces of furniture) in a grid of
    ``shape``, every cell of a rectangle occupied: a plane has 9 of its 27 offsets occupied."""
    rows = np.zeros((0, 3), dtype=np.int64)
    while len(rows) < target:
        axis = int(rng.integers(0, 3))
        lo = (rng.uniform(0, 0.8, 3) * shape).astype(np.int64)
        ext = np.maximum((rng.uniform(0.02, 0.2, 3) * shape).astype(np.int64), 2)
        ext[axis] = 1
        hi = np.minimum(lo + ext, np.array(shape))
        cells = np.stack(np.meshgrid(*[np.arange(lo[a], hi[a]) for a in range(3)], indexing="ij"), -1).reshape(-1, 3)
        rows = np.concatenate([rows, cells])
        _, first = np.unique(rows, axis=0, return_index=True)
        rows = rows[np.sort(first)]
    return rows[:target]


def pairs_of(table, k_of=None):
    """Per offset the (output rows, input rows) of a table, for the torch loop."""
    out = []
    K = 8 if k_of is not None else table.shape[0]
    for k in range(K):
        t = table[k] if k_of is None else torch.where(k_of == k, table, torch.full_like(table, -1))
        rows = torch.nonzero(t >= 0).flatten()
        out.append((rows, t[rows].long()))
    return out


def torch_loop(x, w, pairs, rows_out):
    Co, Ci = w.shape[0], w.shape[-1]
    wk = w.reshape(Co, -1, Ci)
    y = x.new_zeros((rows_out, Co))
    for k, (rows, src) in enumerate(pairs):
        if len(rows):
            y = y.index_add(0, rows, x[src] @ wk[:, k, :].T)
    return y


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--samples", type=int, default=12)
    ap.add_argument("--voxels", type=int, default=551188)
    ap.add_argument("--levels", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    from gapro_amd import consumer_ops as ops

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(args.seed)
    shape = (256, 512, 512)
    per = [args.voxels // args.samples + (1 if b < args.voxels % args.samples else 0) for b in range(args.samples)]
    coords = np.concatenate([np.concatenate([np.full((n, 1), b), surface_scan(rng, n, shape)], 1)
                             for b, n in enumerate(per)])
    coords = torch.from_numpy(coords).to(dev)
    res = {"samples": args.samples, "levels": []}
    gen = torch.Generator(device=dev).manual_seed(args.seed)

    def rand(*size):
        return torch.randn(*size, device=dev, generator=gen)

    for level in range(1, args.levels + 1):
        C, V = 32 * level, int(coords.shape[0])
        r = {"level": level, "voxels": V, "channels": C, "spatial_shape": list(shape)}
        r["subm_plan"] = timed(lambda: ops.subm_plan(coords, shape, args.samples, check=False), args.seconds)
        sub = ops.subm_plan(coords, shape, args.samples)
        last = level == args.levels
        if not last:
            r["downsample_plan"] = timed(lambda: ops.downsample_plan(coords, shape, args.samples, check=False),
                                         args.seconds)
            down = ops.downsample_plan(coords, shape, args.samples)
        layers = [("subm", ops.subm_conv3d, sub, V, V, C, C, 27, pairs_of(sub.neighbours))]
        if not last:
            Vc = down.n_out
            layers.append(("down", ops.sparse_conv3d, down, V, Vc, C, C + 32, 8, pairs_of(down.children)))
            layers.append(("inverse", ops.sparse_inverse_conv3d, down, Vc, V, C + 32, C, 8,
                           pairs_of(down.parent, down.child_slot)))
        for name, fn, plan, rows_in, rows_out, Ci, Co, K, pairs in layers:
            k = 3 if K == 27 else 2
            x, w = rand(rows_in, Ci).requires_grad_(), (rand(Co, k, k, k, Ci) / (K * Ci) ** 0.5).requires_grad_()
            g = rand(rows_out, Co)
            n_pairs = int(sum(len(p[0]) for p in pairs))
            with torch.no_grad():
                a, b = fn(x, w, plan), torch_loop(x, w, pairs, rows_out)
                assert torch.allclose(a, b, rtol=1e-3, atol=1e-3 * float(b.abs().max())), "the two statements disagree"

            def forward(f):
                with torch.no_grad():
                    f()

            def both(f):
                x.grad = w.grad = None
                f().backward(g)

            ours, theirs = (lambda: fn(x, w, plan)), (lambda: torch_loop(x, w, pairs, rows_out))
            m = {"rows_in": rows_in, "rows_out": rows_out, "c_in": Ci, "c_out": Co, "pairs": n_pairs,
                 "occupied_share": n_pairs / float(K * rows_out),
                 "forward": timed(lambda: forward(ours), args.seconds),
                 "forward_backward": timed(lambda: both(ours), args.seconds),
                 "torch_forward": timed(lambda: forward(theirs), args.seconds, warmup=1),
                 "torch_forward_backward": timed(lambda: both(theirs), args.seconds, warmup=1)}
            sec = m["forward"]["median_ms"] * 1e-3
            m["forward_tflops"] = 2.0 * n_pairs * Ci * Co / sec / 1e12
            m["forward_bytes"] = 4 * (n_pairs * Ci + rows_out * Co + K * rows_out)
            m["forward_share_of_hbm"] = m["forward_bytes"] / sec / HBM_ACHIEVABLE
            print("level %d %-7s %7d -> %7d rows, %3d -> %3d ch, %.0f %% of the offsets occupied: forward %.3f ms "
                  "(%.1f TFLOP/s, %.2f TB/s = %.0f %% of 6.3), torch %.3f ms; forward + backward %.3f ms, torch %.3f ms"
                  % (level, name, rows_in, rows_out, Ci, Co, 100 * m["occupied_share"], m["forward"]["median_ms"],
                     m["forward_tflops"], m["forward_bytes"] / sec / 1e12, 100 * m["forward_share_of_hbm"],
                     m["torch_forward"]["median_ms"], m["forward_backward"]["median_ms"],
                     m["torch_forward_backward"]["median_ms"]), flush=True)
            r[name] = m
            del x, w, g, pairs
        print("level %d plans: subm %.3f ms%s" % (level, r["subm_plan"]["median_ms"],
                                                   "" if last else ", down %.3f ms" % r["downsample_plan"]["median_ms"]),
              flush=True)
        res["levels"].append(r)
        if not last:
            coords, shape = down.coords, down.spatial_shape
        torch.cuda.empty_cache()
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
