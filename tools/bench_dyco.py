#!/usr/bin/env python3
"""Time ISBNet's dynamic-convolution mask head (``consumer_ops.dynamic_mask_head``) at three shapes: the released step
(12 samples, 256 queries, C = 32, 1500 superpoints a sample as the stand-in the other benches use), the
``use_spp_pool: False`` branch (15 000 subsampled points a sample) and one sample at inference (forward only).

    python tools/bench_dyco.py [--samples 12] [--queries 256] [--channels 32] [--points 1500 15000] [--seconds 1.0]

Reported, each as a median: the forward, the forward plus backward (gradients of the controllers, the mask features and
both box tensors) and the peak of ``torch.cuda.max_memory_allocated`` over a forward plus backward, above what the inputs
hold.  Beside them, in the same run, a torch statement of the reference's loop on the same device (isbnet.py:783-885:
per sample the repeat, the concatenation and three einsums, float32, backward by autograd) -- a timing and memory
yardstick; the two are compared to 1e-3 first.  FLOP/s are the definition's 2 ((C + 6) C + C C/2 + C/2) operations a
(query, point) pair over the forward's time.  A call is timed between two HIP events.  One JSON line at the end.
Needs the GPU.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEYS = ("controllers", "mask_features", "locs_float", "box_preds", "queries_locs", "queries_box_preds")
GRAD_KEYS = ("controllers", "mask_features", "box_preds", "queries_box_preds")


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


def torch_loop(t, off):
    """The reference's loop, stated with torch ops on the device."""
    th, C = t["controllers"], t["mask_features"].shape[1]
    H, Q = C // 2, th.shape[1]
    out = []
    for b, (lo, hi) in enumerate(zip(off, off[1:])):
        if hi == lo:
            out.append(None)
            continue
        W1, W2, W3, b1, b2, _ = torch.split(th[b], [(C + 6) * C, C * H, H, C, H, 1], dim=1)
        x = t["mask_features"][lo:hi].T[None].repeat(Q, 1, 1)
        rel = (t["queries_locs"][b].reshape(-1, 1, 3) - t["locs_float"][lo:hi].reshape(1, -1, 3)).permute(0, 2, 1)
        qb, pb = t["queries_box_preds"][b], t["box_preds"][lo:hi]
        dims = torch.abs((qb[:, 3:] - qb[:, :3]).reshape(-1, 1, 3) - (pb[:, 3:] - pb[:, :3]).reshape(1, -1, 3))
        x = torch.cat([rel, dims.permute(0, 2, 1), x], dim=1)
        x = torch.relu(torch.einsum("qab,qan->qbn", W1.reshape(Q, C + 6, C), x) + b1.unsqueeze(-1))
        x = torch.relu(torch.einsum("qab,qan->qbn", W2.reshape(Q, C, H), x) + b2.unsqueeze(-1))
        out.append(torch.einsum("qab,qan->qbn", W3.reshape(Q, H, 1), x).squeeze(1))
    return out


def make_inputs(rng, dev, B, Q, C, n):
    from gapro_amd import consumer_ops as ops
    N, P = B * n, ops.dyco_param_count(C)
    locs, qlocs = rng.uniform(0, 6, (N, 3)), rng.uniform(0, 6, (B, Q, 3))
    h = {"controllers": rng.normal(0, 0.2, (B, Q, P)), "mask_features": rng.normal(0, 1, (N, C)), "locs_float": locs,
         "box_preds": np.concatenate([locs - rng.uniform(0.1, 1, (N, 3)), locs + rng.uniform(0.1, 1, (N, 3))], 1),
         "queries_locs": qlocs,
         "queries_box_preds": np.concatenate([qlocs - rng.uniform(0.1, 1, (B, Q, 3)),
                                              qlocs + rng.uniform(0.1, 1, (B, Q, 3))], 2)}
    t = {k: torch.from_numpy(v.astype(np.float32)).to(dev) for k, v in h.items()}
    return t, [b * n for b in range(B + 1)]


def peak_of(fn, drop=()):
    for x in drop:  # gradients of an earlier call: freed before the base is read, not inside the window
        x.grad = None
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--samples", type=int, default=12)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--channels", type=int, default=32)
    ap.add_argument("--points", type=int, nargs="+", default=[1500, 15000])
    ap.add_argument("--inference-points", type=int, default=1500)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    from gapro_amd import consumer_ops as ops

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(args.seed)
    Q, C = args.queries, args.channels
    flop_pair = 2 * ((C + 6) * C + C * (C // 2) + C // 2)
    shapes = [("step_%d" % n, args.samples, n, True) for n in args.points]
    shapes.append(("inference_%d" % args.inference_points, 1, args.inference_points, False))
    res = {"shape": {"queries": Q, "channels": C}}
    for label, B, n, train in shapes:
        t, off = make_inputs(rng, dev, B, Q, C, n)
        ours = lambda: ops.dynamic_mask_head(*[t[k] for k in KEYS], off)  # noqa: E731
        theirs = lambda: torch_loop(t, off)  # noqa: E731
        with torch.no_grad():
            for a, b in zip(ours(), theirs()):
                assert torch.allclose(a, b, rtol=1e-3, atol=1e-3 * float(b.abs().max())), "the two statements disagree"
        ups = [torch.from_numpy(rng.standard_normal((Q, n)).astype(np.float32)).to(dev) for _ in range(B)]

        def both(fn):
            for k in GRAD_KEYS:
                t[k].grad = None
            torch.autograd.backward(fn(), ups)

        def forward(fn):
            with torch.no_grad():
                fn()

        r = {"samples": B, "points_per_sample": n, "forward": timed(lambda: forward(ours), args.seconds),
             "torch_forward": timed(lambda: forward(theirs), args.seconds, warmup=1),
             "forward_peak_bytes": peak_of(lambda: forward(ours)),
             "torch_forward_peak_bytes": peak_of(lambda: forward(theirs))}
        r["forward_tflops"] = flop_pair * B * Q * n / (r["forward"]["median_ms"] * 1e-3) / 1e12
        line = "%s: forward %.3f ms (%.1f TFLOP/s), torch %.3f ms; peak %.1f MB, torch %.1f MB" % (
            label, r["forward"]["median_ms"], r["forward_tflops"], r["torch_forward"]["median_ms"],
            r["forward_peak_bytes"] / 1e6, r["torch_forward_peak_bytes"] / 1e6)
        if train:
            for k in GRAD_KEYS:
                t[k].requires_grad_()
            both(ours)
            mine = {k: t[k].grad.clone() for k in GRAD_KEYS}
            # The yardstick in float64 where it fits (it then agrees with the device on every active set); in float32
            # a pre-activation within rounding of zero flips a whole term of a sum, so only the norm is compared.
            exact = B * Q * n <= 5_000_000
            d = {k: (v.detach().double() if exact else v.detach()).requires_grad_(k in GRAD_KEYS) for k, v in t.items()}
            torch.autograd.backward(torch_loop(d, off), [u.to(d["controllers"].dtype) for u in ups])
            r["gradient_check"] = {}
            for k in GRAD_KEYS:
                err = float((mine[k].double() - d[k].grad.double()).norm() / d[k].grad.double().norm())
                r["gradient_check"][k] = err
                assert err <= (1e-6 if exact else 1e-2), (k, err)
            print("%s: gradients against torch in %s, relative norm of the difference: %s" % (
                label, "float64" if exact else "float32", ", ".join("%s %.1e" % kv for kv in r["gradient_check"].items())))
            del d
            def one_kernel(keys):  # the backward with one of its two kernels: the others' inputs ask for no gradient
                for k in GRAD_KEYS:
                    t[k].requires_grad_(k in keys)
                res = timed(lambda: both(ours), args.seconds / 2)
                for k in GRAD_KEYS:
                    t[k].requires_grad_()
                return res

            r.update({"forward_backward_by_query_only": one_kernel(("controllers", "queries_box_preds")),
                      "forward_backward_by_point_only": one_kernel(("mask_features", "box_preds")),
                      "forward_backward": timed(lambda: both(ours), args.seconds),
                      "torch_forward_backward": timed(lambda: both(theirs), args.seconds, warmup=1),
                      "forward_backward_peak_bytes": peak_of(lambda: both(ours), [t[k] for k in GRAD_KEYS]),
                      "torch_forward_backward_peak_bytes": peak_of(lambda: both(theirs), [t[k] for k in GRAD_KEYS])})
            line += ("; forward + backward %.3f ms (by-query kernel only %.3f, by-point kernel only %.3f), torch %.3f ms; "
                     "peak %.1f MB, torch %.1f MB") % (
                r["forward_backward"]["median_ms"], r["forward_backward_by_query_only"]["median_ms"],
                r["forward_backward_by_point_only"]["median_ms"], r["torch_forward_backward"]["median_ms"],
                r["forward_backward_peak_bytes"] / 1e6, r["torch_forward_backward_peak_bytes"] / 1e6)
        print(line, flush=True)
        res[label] = r
        del t, ups
        torch.cuda.empty_cache()
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
