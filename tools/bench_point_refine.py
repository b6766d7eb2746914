#!/usr/bin/env python3
"""Point-level label benchmark (run on the GPU box): one synth.make_scene scene of --points points (the scene of
tools/bench_fit_gp.py) through Pipeline(point_level=True) (--mode winner), Pipeline(point_level="compete") or
Pipeline(point_level="vote").

python tools/bench_point_refine.py [--points 150000] [--seed 0] [--reps 3] [--mode winner|compete|vote]

Reports the point-level stages behind the label broadcast -- gather (row table of the refined superpoints' points),
predict (one gapro_svgp_predict_batch over it, which synchronises the stream once) and apply; with --mode compete also
expand (the row list: a gathered row once per fit that tested its superpoint, R rows -> R2 entries) in front of the
predict and compete (the per-point merge) behind the apply, which is then the mu / var broadcast alone -- as spans between HIP
events recorded on the stream at the stage boundaries (a span contains the host's work between the launches of the
stage, it is not a kernel time), and the host's wall clock for the plan: the median over --reps runs after one warm-up
run, inputs resident on the device.  Also: refined superpoints, rows R, expanded rows R2 and predict models, how many
refined points end with another instance than their superpoint's, how many points end with another instance in the two
modes (the other mode is run once for that), and the scene's mean instance IoU (get_miou_scene) without the refinement and
in both modes.  --mode vote: gather, expand and predict as for compete, then vote (the superpoint vote, written to the
superpoint tables) and labels (the ordinary label broadcast, which in this mode runs last); the spans start where the
merge's tables have been uploaded; the other mode is "compete"; also the superpoints that end in another box than the
merge's and the vote's mean instance IoU.  One JSON line at the end.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gapro_amd.eval_ps_labels import get_miou_scene  # noqa: E402
from gapro_amd.gen_ps_utils import _pipeline, getInstanceInfo  # noqa: E402
from gapro_amd.pipeline import make_job  # noqa: E402
from gapro_amd.synth import make_scene  # noqa: E402

STAGES = {"winner": ("gather", "predict", "apply"), "compete": ("gather", "expand", "predict", "apply", "compete"),
          "vote": ("gather", "expand", "predict", "vote", "labels")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=150000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--mode", choices=("winner", "compete", "vote"), default="winner")
    args = ap.parse_args()
    stages = STAGES[args.mode]
    if not torch.cuda.is_available():
        raise SystemExit("bench_point_refine.py needs the GPU: there is nothing to time without it")
    dev = torch.device("cuda", 0)
    sc = make_scene(seed=args.seed, n_points=args.points, with_walls_json=False, mesh_order=True)
    xyz = sc.aligned_xyz()
    _, cls, box, vol, _ = getInstanceInfo(xyz, sc.inst, sc.sem)
    dev_in = (torch.as_tensor(np.asarray(xyz, dtype=np.float64)).to(dev),
              torch.as_tensor(sc.default_feats().astype(np.float32)).to(dev),
              torch.as_tensor(np.asarray(sc.spp).astype(np.int64)).to(dev))
    rest = (cls.astype(np.int64), box.astype(np.float32), vol.astype(np.float32), [], [])
    opts = dict(instance_classes=18, ground_h=0.1, thresh_spp_occu=0.999, device=dev)

    plain_pipe = _pipeline(dev, 50)
    plain_job = make_job(*dev_in, *rest, **opts)
    plain = plain_pipe.run([plain_job])[0]
    modes = {"winner": True, "compete": "compete", "vote": "vote"}
    pipe = _pipeline(dev, 50, point_level=modes[args.mode])
    times = {s: [] for s in stages}
    plan, total = [], []
    out = None
    for rep in range(args.reps + 1):  # the first run warms every kernel and buffer up
        job = make_job(*dev_in, *rest, **opts)
        torch.cuda.synchronize()
        pipe.stage_events = []
        t0 = time.perf_counter()
        out = pipe.run([job])[0]
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        ev = dict(pipe.stage_events)
        pipe.stage_events = None
        if rep:
            prev = ev["broadcast"]
            for s in stages:
                times[s].append(prev.elapsed_time(ev[s]))
                prev = ev[s]
            plan.append(1e3 * pipe.last_refine["plan_s"])
            total.append(1e3 * (t1 - t0))
    t0 = time.perf_counter()
    plain_pipe.run([make_job(*dev_in, *rest, **opts)])
    torch.cuda.synchronize()
    plain_ms = 1e3 * (time.perf_counter() - t0)

    inv = job.spp_inv.long()
    refined = torch.from_numpy(job.host["winner"] >= 0).to(dev)[inv]
    changed = int(((out[1] != plain[1]) & refined).sum())
    assert int((out[1] != plain[1]).sum()) == changed  # nothing outside a refined superpoint moves
    sem_gt = torch.from_numpy(np.asarray(sc.sem)).to(dev).int()
    ins_gt = torch.from_numpy(np.asarray(sc.inst)).to(dev).int()
    sem_gt[sem_gt != -100] -= 2  # reference gen_ps.py:119-120
    sem_gt[(sem_gt == -1) | (sem_gt == -2)] = 18
    other_mode = "winner" if args.mode == "compete" else "compete"
    other = _pipeline(dev, 50, point_level=modes[other_mode]).run([make_job(*dev_in, *rest, **opts)])[0]
    by_mode = {args.mode: out, other_mode: other}
    if args.mode == "vote":  # the IoU line names all three modes
        by_mode["winner"] = _pipeline(dev, 50, point_level=True).run([make_job(*dev_in, *rest, **opts)])[0]
    miou = [float(get_miou_scene(sem_gt.long(), ins_gt.long(), o[0].long(), o[1].long()).float().mean())
            if o is not None else None for o in (plain, by_mode["winner"], by_mode["compete"], by_mode.get("vote"))]
    res = dict(mode=args.mode, points=args.points, seed=args.seed, reps=args.reps,
               refined_spps=pipe.last_refine["refined_spps"], refined_points=int(refined.sum()),
               rows=pipe.last_refine["rows"], expanded_rows=pipe.last_refine["expanded_rows"],
               multi_spps=pipe.last_refine.get("multi_spps"), models=pipe.last_refine["models"],
               changed_instance=changed, differs_between_modes=int((out[1] != other[1]).sum()),
               miou_spp_level=round(miou[0], 6), miou_point_level=round(miou[{"winner": 1, "compete": 2, "vote": 3}[args.mode]], 6),
               miou_winner=round(miou[1], 6), miou_compete=round(miou[2], 6),
               changed_spps=int(torch.unique(inv[(out[1] != plain[1]) | (out[0] != plain[0])]).numel()),
               plan_host_ms=round(float(np.median(plan)), 3), run_ms=round(float(np.median(total)), 3),
               run_ms_plain_once=round(plain_ms, 3))
    for s in stages:
        res[s + "_ms"] = round(float(np.median(times[s])), 3)
        res[s + "_ms_min_max"] = [round(float(min(times[s])), 3), round(float(max(times[s])), 3)]
    print("%(mode)s, %(points)d points: %(refined_spps)d refined superpoints, %(rows)d rows -> %(expanded_rows)d, "
          "%(models)d models; %(changed_instance)d refined points end with another instance, %(differs_between_modes)d "
          "points differ between the modes; mean instance IoU %(miou_spp_level).4f -> %(miou_winner).4f (winner) / "
          "%(miou_compete).4f (compete)" % res)
    if args.mode == "vote":
        print("  vote: %(changed_spps)d superpoints end in another box than the merge's; mean instance IoU "
              "%(miou_point_level).4f" % res)
    for s in stages:
        print("  %-8s %8.3f ms  (min %.3f, max %.3f over %d runs)" % ((s, res[s + "_ms"]) + tuple(res[s + "_ms_min_max"])
                                                                     + (args.reps,)))
    print("  plan     %8.3f ms  (host wall clock)" % res["plan_host_ms"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
