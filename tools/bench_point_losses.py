#!/usr/bin/env python3
"""Time forward plus backward of ``consumer_ops.point_wise_losses`` against the torch statement of the chain it replaces
(ISBNet's ``Criterion.cal_point_wise_loss``: ``F.cross_entropy`` over the whole score block, six boolean-mask gathers,
the ``total_pos_inds == 0`` test and ``batch_giou_corres``), on the same device, in the same run, on synthetic input.

    python tools/bench_point_losses.py [--points 1000000] [--classes 20] [--positive 0.6] [--seconds 1.0]
                                       [--kernel-times]

The default shape is a STAND-IN for a batch's voxels: nobody has measured the N of a real training step.  A call is the
forward, the weighted sum of the four losses and its backward, timed between two HIP events on the stream;
``point_wise_losses`` is timed with ``check=True`` (one synchronisation for the status) and with ``check=False``.  Each
form is warmed up, then called in alternating blocks until it has filled its window; the median, minimum and maximum of
the per-call times are printed and one JSON line.  The two forms' losses and gradients are compared first (the torch
chain is float32: 1e-4 relative to each array's largest magnitude).  ``--kernel-times`` also takes the device time of
the library's three kernels from ``torch.profiler`` and sets it against the bytes they must move: the score block once
forward, once backward and its gradient once (about 3 passes), plus the narrow arrays.  Needs the GPU.
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
from bench_spp_gt import timed  # noqa: E402

WEIGHTS = (0.25, 0.25, 0.25, 0.25)  # Criterion.forward's factor on every "pw" key
IGNORE = -100


def make_points(n, classes, positive, seed=0):
    rng = np.random.default_rng(seed)
    lab = np.concatenate([-rng.uniform(0.2, 2.5, (n, 3)), rng.uniform(0.2, 2.5, (n, 3))], 1)
    sem = rng.integers(0, classes, n)
    sem[rng.random(n) < 0.05] = IGNORE
    inst = rng.integers(0, 40, n)
    inst[rng.random(n) >= positive] = IGNORE
    # every predicted face at least 0.01 off its label: float32 and float64 boxes take the same min / max / L1 branches
    pred = lab + rng.choice([-1.0, 1.0], (n, 6)) * rng.uniform(0.01, 0.6, (n, 6))
    return [rng.normal(0, 2, (n, classes)).astype(np.float32), pred.astype(np.float32),
            rng.uniform(0, 1, n).astype(np.float32), sem, inst, lab.astype(np.float32),
            rng.uniform(-6, 6, (n, 3)).astype(np.float32)]


def giou_corres(a, b):
    """model_utils.py:416-444."""
    inter = (torch.min(a[:, 3:], b[:, 3:]) - torch.max(a[:, :3], b[:, :3])).clamp(min=0.0).prod(-1)
    union = (a[:, 3:] - a[:, :3]).clamp(min=0.0).prod(-1) + (b[:, 3:] - b[:, :3]).clamp(min=0.0).prod(-1) - inter
    iou = inter / (union + 1e-6)
    bound = (torch.max(a[:, 3:], b[:, 3:]) - torch.min(a[:, :3], b[:, :3])).clamp(min=0.0).prod(-1)
    return iou, iou - (bound - union) / (bound + 1e-6)


def torch_point_wise(scores, corners, conf, sem, inst, labels, coords, voxel_scale=50):
    """criterion.py:136-191 in plain torch on the device, as a consumer writes it today."""
    out = {"pw_sem_loss": F.cross_entropy(scores, sem, ignore_index=IGNORE)}
    pos = inst != IGNORE
    total = pos.sum()
    if total == 0:
        l1, giou_loss, conf_loss = 0 * corners.sum(), 0 * conf.sum(), 0 * conf.sum()
    else:
        l1 = F.l1_loss(corners[pos], labels[pos], reduction="sum") / total
        iou, giou = giou_corres(corners[pos] + coords[pos].repeat(1, 2), labels[pos] + coords[pos].repeat(1, 2))
        giou_loss = torch.sum(1 - giou) / total
        conf_loss = F.mse_loss(conf[pos], iou.detach(), reduction="sum") / total
    out.update({"pw_corners_loss": l1 * voxel_scale / 50.0, "pw_giou_loss": giou_loss, "pw_conf_loss": conf_loss})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000, help="voxels of the whole batch (a stand-in, see above)")
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--positive", type=float, default=0.6, help="share of the points with an instance")
    ap.add_argument("--seconds", type=float, default=1.0, help="timed window per form and block")
    ap.add_argument("--blocks", type=int, default=2, help="alternating blocks per form")
    ap.add_argument("--kernel-times", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_point_losses needs the GPU: a CPU run gives no time")
    dev = torch.device("cuda", 0)
    d = [torch.from_numpy(a).to(dev) for a in make_points(args.points, args.classes, args.positive)]
    leaves = d[:3]
    for t in leaves:
        t.requires_grad_()

    def step_of(losses_fn):
        def call():
            for t in leaves:
                t.grad = None
            out = losses_fn()
            sum(w * out[k] for w, k in zip(WEIGHTS, consumer_ops.POINT_LOSS_NAMES)).backward()
            return out
        return call

    forms = {"point_wise_losses": step_of(lambda: consumer_ops.point_wise_losses(*d)),
             "point_wise_losses_nocheck": step_of(lambda: consumer_ops.point_wise_losses(*d, check=False)),
             "torch_point_wise": step_of(lambda: torch_point_wise(*d))}
    results = {}
    for k in ("point_wise_losses", "torch_point_wise"):
        out = forms[k]()
        results[k] = ([float(out[n].detach()) for n in consumer_ops.POINT_LOSS_NAMES],
                      [t.grad.double().clone() for t in leaves])
    diffs = [abs(a - b) / max(abs(a), 1e-12) for a, b in zip(*(results[k][0] for k in results))]
    diffs += [float((a - b).abs().max() / a.abs().max().clamp(min=1e-30)) for a, b in zip(*(results[k][1] for k in results))]
    worst = max(diffs)
    assert worst < 1e-4, diffs  # the four losses, then the gradients of the scores, the corners and the confidence

    n, c = args.points, args.classes
    out = {"points": n, "classes": c, "positive": args.positive, "max_relative_difference": worst}
    if args.kernel_times:
        from torch.profiler import ProfilerActivity, profile

        fn = forms["point_wise_losses_nocheck"]
        fn()
        torch.cuda.synchronize()
        reps = 10
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        label_bytes = d[3].element_size() + d[4].element_size()
        must = {"k_point_partial": n * (4 * (c + 6 + 6 + 3 + 1) + label_bytes), "k_point_finish": 0,
                "k_point_backward": n * (4 * (c + 6 + 6 + 3 + 1) + label_bytes + 4 * (c + 6 + 1))}
        for e in prof.key_averages():
            name = next((k for k in must if k in e.key), None)
            if name is None:
                continue
            us = float(getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0)) / max(e.count, 1)
            out[name + "_us"] = us
            if must[name] and us > 0:
                out[name + "_GBps"] = must[name] / us * 1e-3
            print("%-18s %9.1f us per launch (%d launches)%s" % (
                name, us, e.count, "  %.0f GB/s of the bytes it must move" % out[name + "_GBps"] if must[name] else ""))
        out["score_block_MB"] = n * c * 4 / 1e6
    times = {k: [] for k in forms}
    for _ in range(args.blocks):
        for k, fn in forms.items():
            times[k] += timed(fn, args.seconds)
    for k, t in times.items():
        t = np.asarray(t)
        print("%-26s %9.3f ms per call (median of %d; %.3f .. %.3f)" % (k, np.median(t), len(t), t.min(), t.max()))
        out[k + "_ms"] = {"median": float(np.median(t)), "min": float(t.min()), "max": float(t.max()), "calls": len(t)}
    out["speedup"] = out["torch_point_wise_ms"]["median"] / out["point_wise_losses_ms"]["median"]
    out["speedup_nocheck"] = out["torch_point_wise_ms"]["median"] / out["point_wise_losses_nocheck_ms"]["median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
