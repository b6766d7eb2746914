#!/usr/bin/env python3
"""Point-level fit benchmark (run on the GPU box): one synth.make_scene scene of --points points, every GP pair of
its schedule turned into a point-level problem (the points of the pair's superpoints), through FitRunner.fit_points in
both modes.

python tools/bench_fit_gp.py [--points 150000] [--seed 0] [--npoint-nearest 800] [--reps 5] [--max-problems 0]

Per mode: the problems' sizes and the time of every stage of the chain -- prepare (scene statistics and superpoint
ranks), assemble (index upload, training-set kernels; in pool mode also the host's read of the row counts), fit (one
launch on the assembled table) and predict (one launch at every intersection point's own features) -- from HIP events
recorded on the stream at the stage boundaries: the median over --reps runs after one warm-up run, inputs resident on
the device.  A stage time is a span on the stream (it contains the host's work between the launches of that stage), not
a kernel time.  One JSON line per mode at the end.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gapro_amd.fit_runner import pack_point_problems  # noqa: E402
from gapro_amd.gen_ps_utils import _pipeline, gen_pseudo_label_gaussian_process  # noqa: E402

STAGES = ("prepare", "assemble", "fit", "predict")


def scene_problems(seed, n_points):
    """One make_scene scene of n_points points in mesh order, its generator inputs (as __graft_entry__.smoke builds
    them) and its schedule's GP pairs as point index sets."""
    from gapro_amd.gen_ps_utils import getInstanceInfo
    from gapro_amd.synth import make_scene

    sc = make_scene(seed=seed, n_points=n_points, with_walls_json=False, mesh_order=True)
    xyz = sc.aligned_xyz()
    _, cls, box, vol, _ = getInstanceInfo(xyz, sc.inst, sc.sem)
    kw = dict(coords_float=xyz, mask_feats=sc.default_feats().astype(np.float32), spp=sc.spp,
              instance_cls=cls.astype(np.int64), instance_box=box.astype(np.float32),
              instance_box_volume=vol.astype(np.float32), wall_box=[], wall_box_volume=[], instance_classes=18,
              ground_h=0.1, thresh_spp_occu=0.999)
    assert len(xyz) == n_points
    fits = gen_pseudo_label_gaussian_process(**kw, return_models=True, device="cuda:0")[-1].fits
    spp = np.asarray(kw["spp"]).astype(np.int64)
    inv = np.unique(spp, return_inverse=True)[1].reshape(-1)
    problems = []
    for f in fits:
        b1, b2 = f.train[:f.m1], f.train[f.m1:]
        problems.append(tuple(np.nonzero(np.isin(inv, r))[0] for r in (b1, b2, f.test)))
    return kw, problems


def run_mode(pipe, dev_in, problems, n, k, pool, reps):
    descs, h_idx = pack_point_problems(problems, n, k, pool)
    times = {s: [] for s in STAGES}
    res = None
    for rep in range(reps + 1):  # the first run warms every kernel and workspace up
        pipe.stage_events = []
        res = pipe.fit_points(*dev_in, descs, h_idx, k, pool, raise_on_failure=False)
        torch.cuda.synchronize()
        ev = dict(pipe.stage_events)
        pipe.stage_events = None
        if rep:
            prev = ev["start"]
            for s in STAGES:
                times[s].append(prev.elapsed_time(ev[s]))
                prev = ev[s]
    m = np.array([d.m1 + d.m2 for d in descs])
    out = dict(mode="pool" if pool else "nearest", points=n, problems=len(problems), npoint_nearest=None if pool else k,
               side_points=int(sum(d.n1 + d.n2 for d in descs)), test_points=int(sum(d.t for d in descs)),
               m_min=int(m.min()), m_median=float(np.median(m)), m_max=int(m.max()), reps=reps,
               failed=int((res["status"] != 0).sum()))
    for s in STAGES:
        out[s + "_ms"] = round(float(np.median(times[s])), 3)
        out[s + "_ms_min_max"] = [round(float(min(times[s])), 3), round(float(max(times[s])), 3)]
    out["total_ms"] = round(sum(out[s + "_ms"] for s in STAGES), 3)
    print("%(mode)s: %(points)d points, %(problems)d problems, %(side_points)d side points, %(test_points)d test points, "
          "M %(m_min)d / %(m_median).0f / %(m_max)d (min / median / max), %(failed)d failed" % out)
    for s in STAGES:
        print("  %-9s %9.3f ms  (min %.3f, max %.3f over %d runs)" % ((s, out[s + "_ms"]) + tuple(out[s + "_ms_min_max"])
                                                                     + (reps,)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=150000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--npoint-nearest", type=int, default=800)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-problems", type=int, default=0, help="keep only the first so many problems (0 = all)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fit_gp.py needs the GPU: there is nothing to time without it")
    dev = torch.device("cuda", 0)
    kw, problems = scene_problems(args.seed, args.points)
    if args.max_problems:
        problems = problems[:args.max_problems]
    if not problems:
        raise SystemExit("the scene's schedule has no GP pair")
    dev_in = (torch.as_tensor(np.asarray(kw["coords_float"], dtype=np.float64)).to(dev),
              torch.as_tensor(np.asarray(kw["mask_feats"], dtype=np.float32)).to(dev),
              torch.as_tensor(np.asarray(kw["spp"]).astype(np.int64)).to(dev))
    pipe = _pipeline(dev, 50)
    lines = [run_mode(pipe, dev_in, problems, len(dev_in[2]), args.npoint_nearest, pool, args.reps)
             for pool in (True, False)]
    for line in lines:
        print(json.dumps(line))


if __name__ == "__main__":
    main()
