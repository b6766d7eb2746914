#!/usr/bin/env python3
"""Predict-kernel benchmark (run on the GPU box): N equal models of size M, trained by the fit launch, each predicted
at T rows by gapro_svgp_predict_batch.

python tools/bench_predict.py [--sizes 64,128,256] [--d 6] [--models 64] [--rows 1000000] [--window 1.0]
python tools/bench_predict.py --headline 256     every model of a 256-scene headline batch at its own test set

Per case: ms per launch (HIP events around the launch, warm-up first, a window of at least --window seconds), rows/s,
TFLOP/s of the algorithmic count M^3/3 + 2 M^2 T + 2 D (M^2 + M T) per model (SURVEY 8d's F_pred) against the 78.6
TFLOP/s FP64 matrix peak, bytes moved per second against ~6.3 TB/s, and which of the two bounds.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gapro_amd._lib import PredictDesc  # noqa: E402
from gapro_amd.gaussian_process_utils import fit_gp_spp_batch  # noqa: E402
from gapro_amd.gen_ps_utils import _pipeline  # noqa: E402
from gapro_amd.fit_runner import ROW_FIELDS, _ptr, block_bytes, block_views  # noqa: E402
from gapro_amd.synth import make_gp_problem  # noqa: E402

PEAK_TFLOPS, PEAK_TBS = 78.6, 6.3


def f_pred(m, t, d):
    return m ** 3 / 3.0 + 2.0 * m * m * t + 2.0 * d * (m * m + m * t)


def time_launch(pipe, models, feats, rows, window):
    """One gapro_svgp_predict_batch launch over device-resident inputs, repeated; returns (ms per launch, launches)."""
    lib, ctx = pipe.lib, pipe.ctx
    n, D, R = len(models), int(feats.shape[1]), int(feats.shape[0])
    states = [m.to_state() for m in models]
    descs = (PredictDesc * n)()
    so = ro = 0
    for k in range(n):
        d = descs[k]
        d.state_offset, d.row_offset, d.out_offset, d.t, d.reserved = so, ro, ro, len(rows[k]), 0
        so += len(states[k])
        ro += len(rows[k])
    no = max(ro, 1)
    h_m = np.array([m.m for m in models], dtype=np.int32)
    d_state = torch.from_numpy(np.concatenate(states)).cuda()
    d_rows = torch.from_numpy(np.concatenate(rows).astype(np.int32)).cuda()
    ws_bytes = int(lib.gapro_svgp_predict_workspace_bytes(n, D, _ptr(h_m)))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    out = block_views(ROW_FIELDS, pipe.be.empty(block_bytes(ROW_FIELDS, no)), no, pipe.be)
    stat = torch.empty(n, dtype=torch.int32, device="cuda")

    def launch():
        ctx.check(lib.gapro_svgp_predict_batch(
            ctx.handle, C.c_void_p(torch.cuda.current_stream().cuda_stream), n, D, _ptr(d_state), _ptr(h_m),
            C.cast(descs, C.c_void_p), _ptr(feats), R, _ptr(d_rows), C.byref(pipe.opt), _ptr(ws), ws_bytes,
            _ptr(out["probs"]), _ptr(out["probs_new"]), _ptr(out["labels"]), _ptr(out["mu"]), _ptr(out["var"]),
            _ptr(stat)))

    launch()
    torch.cuda.synchronize()
    assert int(stat.abs().max()) == 0, "a model failed: %s" % stat.cpu().numpy()
    total, reps = 0.0, 0
    while total < 1e3 * window:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        e1.synchronize()
        total += e0.elapsed_time(e1)
        reps += 1
    return total / reps, reps, ws_bytes


def report(tag, models, rows, d, ms, reps, ws_bytes):
    t_rows = sum(len(r) for r in rows)
    flops = sum(f_pred(m.m, len(r), d) for m, r in zip(models, rows))
    # bytes that must move: per row its features, its index and the five outputs; per model its state in and the
    # prepared matrices out and in again
    byts = t_rows * (4 * d + 4 + 17) + sum(8 * (m.m * m.m + m.m * d + m.m) for m in models) + 2 * ws_bytes
    tf, tb = flops / (1e9 * ms), byts / (1e9 * ms)
    bound = "matrix pipe" if flops / (PEAK_TFLOPS * 1e12) >= byts / (PEAK_TBS * 1e12) else "memory"
    print("%s: models %d rows %d  %.2f ms/launch (%d launches)  %.3e rows/s  %.2f TFLOP/s = %.1f %% of the FP64 matrix "
          "peak  %.3f TB/s = %.1f %% of HBM  nearer roof: %s" % (tag, len(models), t_rows, ms, reps, t_rows / (1e-3 * ms),
                                                                tf, 100 * tf / PEAK_TFLOPS, tb, 100 * tb / PEAK_TBS, bound))


def equal_models(m, d, n):
    """n models of size m: four distinct trained problems, repeated."""
    std = 0.3 if d > 8 else 1.0
    parts, probs, base = [], [], 0
    for i in range(4):
        f, b1, b2, it = make_gp_problem(i, m // 2, m - m // 2, 32, d, std=std)
        parts.append(f)
        probs.append((b1 + base, b2 + base, it + base))
        base += len(f)
    _, models = fit_gp_spp_batch(np.concatenate(parts), probs, training_iter=50, return_models=True)
    return [models[i % 4] for i in range(n)]


def _scene(seed):
    import bench

    return bench.build_scene_inputs(seed, 150000, 6, "stream")


def headline(pipe, n_scenes, window):
    from multiprocessing import get_context

    from gapro_amd.pipeline import make_job

    with get_context("spawn").Pool(min(16, n_scenes)) as pool:
        kws = pool.map(_scene, range(n_scenes))
    dev = torch.device("cuda", 0)
    jobs = [make_job(k["coords_float"], k["mask_feats"], k["spp"], k["instance_cls"], k["instance_box"],
                     k["instance_box_volume"], k["wall_box"], k["wall_box_volume"], k["instance_classes"], k["ground_h"],
                     k["thresh_spp_occu"], device=dev) for k in kws]
    pipe.run(jobs, keep_models=True)
    models, rows, tables, base = [], [], [], 0
    for j in jobs:
        if j.fits is None:
            continue
        for f in j.fits:
            models.append(f.model)
            rows.append(np.asarray(f.test, dtype=np.int64) + base)
        tables.append(j.feats_spp)
        base += len(j.feats_spp)
    feats = torch.from_numpy(np.concatenate(tables)).cuda()
    ms, reps, wsb = time_launch(pipe, models, feats, rows, window)
    report("headline batch of %d scenes" % n_scenes, models, rows, 6, ms, reps, wsb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,128,256")
    ap.add_argument("--d", type=int, default=6)
    ap.add_argument("--models", type=int, default=64)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--headline", type=int, default=0, metavar="SCENES")
    args = ap.parse_args()
    pipe = _pipeline(torch.device("cuda", 0), 50)
    if args.headline:
        return headline(pipe, args.headline, args.window)
    rng = np.random.default_rng(1)
    for m in [int(v) for v in args.sizes.split(",")]:
        models = equal_models(m, args.d, args.models)
        table = make_gp_problem(99, m // 2, m - m // 2, 200000, args.d, std=0.3 if args.d > 8 else 1.0)[0]
        feats = torch.from_numpy(table).cuda()
        rows = [rng.integers(0, len(table), size=args.rows) for _ in models]
        ms, reps, wsb = time_launch(pipe, models, feats, rows, args.window)
        report("M=%d D=%d" % (m, args.d), models, rows, args.d, ms, reps, wsb)


if __name__ == "__main__":
    main()
