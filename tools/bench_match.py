#!/usr/bin/env python3
"""Time ``consumer_ops.match_cost`` and ``hungarian_match`` against a plain torch statement of the loop they replace
(per sample the expression chain of ISBNet's ``HungarianMatcher.get_match``: three einsums, two BCEs of the whole logit
matrix, a softmax, the box terms, the NaN / inf patches, two copies to the host and two SciPy calls), on the same
device, in the same run, on synthetic input of ISBNet's step shape.

    python tools/bench_match.py [--batch 4] [--queries 256] [--instances 40] [--spps 1500] [--dup-gt 4] [--seconds 1.0]
                                [--solver-threads N]

A call is timed between two HIP events on the stream; a call contains its host reads and, for the matchers, the
assignments on the host, so these are call times, not kernel times.  Each form is warmed up, then called in alternating
blocks until it has filled its window; the median, minimum and maximum of the per-call times are printed and one JSON
line.  The costs of the two forms are compared first (the torch chain is float32: 1e-4); whether the two matchers
return the same dicts is reported (``matchers_agree``), not asserted.  Without SciPy only the cost chains are compared
and timed.  Needs the GPU: there is no CPU timing.
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
from gapro_amd.gen_ps_utils import batch_giou_cross  # noqa: E402
from bench_spp_gt import timed  # noqa: E402

try:
    from scipy.optimize import linear_sum_assignment as scipy_lsa
except ImportError:
    scipy_lsa = None


def make_batch(batch, queries, instances, spps, classes=18, seed=0):
    """Per sample instances that share out most superpoints, queries that follow one instance each, predicted boxes
    near the boxes of the instances they follow."""
    rng = np.random.default_rng(seed)
    dc, logits = [], []
    cls_logits = rng.normal(0, 1.5, (batch, queries, classes)).astype(np.float32)
    conf = rng.normal(0, 1, (batch, queries)).astype(np.float32)
    box_preds = np.empty((batch, queries, 6), dtype=np.float32)
    for b in range(batch):
        owner = rng.integers(0, instances + 1, spps)
        owner[rng.permutation(spps)[:instances]] = np.arange(instances)
        mask = (owner[None, :] == np.arange(instances)[:, None]).astype(np.float32)
        cls = rng.integers(0, classes, instances).astype(np.int64)
        lo = rng.uniform(-4, 4, (instances, 3))
        box = np.concatenate([lo, lo + rng.uniform(0.3, 3, (instances, 3))], 1).astype(np.float32)
        follows = rng.integers(0, instances, queries)
        sharp = rng.uniform(0.5, 4.0, queries)[:, None]
        logits.append((sharp * (2 * mask[follows] - 1) + rng.normal(0, 2.0, (queries, spps))).astype(np.float32))
        cls_logits[b, np.arange(queries), cls[follows]] += rng.uniform(0, 4, queries).astype(np.float32)
        box_preds[b] = box[follows] + rng.normal(0, 0.4, (queries, 6))
        dc.append({"mask": mask, "cls": cls, "box": box})
    return cls_logits, logits, conf, box_preds, dc


def torch_cost(cls_b, x, conf_b, box_b, e):
    """matcher.py:156-197 in plain torch on the device, as a consumer writes it today."""
    t = e["mask"]
    sig = x.sigmoid()
    dice = 1 - (2 * torch.einsum("nc,mc->nm", sig, t) + 1) / (sig.sum(-1)[:, None] + t.sum(-1)[None, :] + 1)
    pos = F.binary_cross_entropy_with_logits(x, torch.ones_like(x), reduction="none")
    neg = F.binary_cross_entropy_with_logits(x, torch.zeros_like(x), reduction="none")
    bce = (torch.einsum("nc,mc->nm", pos, t) + torch.einsum("nc,mc->nm", neg, 1 - t)) / x.shape[1]
    cls_cost = -F.softmax(cls_b, dim=-1)[:, e["cls"]]
    conf_cost = -conf_b[:, None].repeat(1, t.shape[0])
    giou_cost = -batch_giou_cross(box_b, e["box"])[1]
    cost = 0.5 * cls_cost + 1 * dice + 1 * bce + 0.2 * conf_cost + 0.2 * giou_cost
    cost[torch.isnan(cost)] = 100000
    cost[torch.isinf(cost)] = 100000
    return cost


def torch_costs(cls_logits, logits, conf, box_preds, dc):
    return [None if e is None else torch_cost(cls_logits[b], logits[b], conf[b], box_preds[b], e)
            for b, e in enumerate(dc)]


def torch_match(cls_logits, logits, conf, box_preds, dc, dup_gt):
    """forward_dup (matcher.py:208-284): per sample the chain, two copies to the host, two SciPy calls, the gathers."""
    keys = ("row_indices", "inst_labels", "cls_labels", "box_labels")
    gt, aux = ({k: [] for k in keys} for _ in range(2))
    for b, e in enumerate(dc):
        if e is None:
            for d in (gt, aux):
                for k in keys:
                    d[k].append(None)
            continue
        cost = torch_cost(cls_logits[b], logits[b], conf[b], box_preds[b], e)
        rows, cols = scipy_lsa(cost.cpu().numpy())
        arows, acols = scipy_lsa(cost.repeat(1, dup_gt).cpu().numpy())
        for d, r, c, rep in ((gt, rows, cols, 1), (aux, arows, acols, dup_gt)):
            d["row_indices"].append(r)
            d["inst_labels"].append(e["mask"].repeat(rep, 1)[c])
            d["cls_labels"].append(e["cls"].repeat(rep)[c])
            d["box_labels"].append(e["box"].repeat(rep, 1)[c])
    return gt, aux


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--instances", type=int, default=40, help="kept instances per sample")
    ap.add_argument("--spps", type=int, default=1500, help="superpoints per sample")
    ap.add_argument("--dup-gt", type=int, default=4)
    ap.add_argument("--seconds", type=float, default=1.0, help="timed window per form and block")
    ap.add_argument("--blocks", type=int, default=2, help="alternating blocks per form")
    ap.add_argument("--solver-threads", type=int, default=consumer_ops.MATCH_SOLVER_THREADS,
                    help="host threads of hungarian_match's assignments (1: the caller's thread)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_match needs the GPU: a CPU run gives no time")
    consumer_ops.MATCH_SOLVER_THREADS = args.solver_threads
    dev = torch.device("cuda", 0)
    cls_logits, logits, conf, box_preds, dc = make_batch(args.batch, args.queries, args.instances, args.spps)
    cls_d, conf_d, box_d = (torch.from_numpy(a).to(dev) for a in (cls_logits, conf, box_preds))
    logits_d = [torch.from_numpy(a).to(dev) for a in logits]
    dc_d = [{k: torch.from_numpy(v).to(dev) for k, v in e.items()} for e in dc]
    common = (cls_d, logits_d, conf_d, box_d, dc_d)

    forms = {"match_cost": lambda: consumer_ops.match_cost(*common),
             "torch_cost": lambda: torch_costs(*common)}
    ours, theirs = forms["match_cost"](), forms["torch_cost"]()
    dev_err = max(float((a.double() - b.double()).abs().max()) for a, b in zip(ours, theirs))
    assert dev_err < 1e-4, dev_err
    if scipy_lsa is not None:
        forms["hungarian_match"] = lambda: consumer_ops.hungarian_match(*common, dup_gt=args.dup_gt)
        forms["torch_match"] = lambda: torch_match(*common, args.dup_gt)
        a, b = forms["hungarian_match"](), forms["torch_match"]()
        # reported, not asserted: the torch chain's float32 cost may order a near-tie the other way
        agree = all((np.array_equal(u, v) if k == "row_indices" else torch.equal(u, v))
                    for mine, ref in zip(a, b) for k in mine for u, v in zip(mine[k], ref[k]))

    with torch.no_grad():
        times = {k: [] for k in forms}
        for _ in range(args.blocks):
            for k, fn in forms.items():
                times[k] += timed(fn, args.seconds)
    out = {"batch": args.batch, "queries": args.queries, "instances_per_sample": args.instances,
           "spps_per_sample": args.spps, "dup_gt": args.dup_gt, "solver_threads": args.solver_threads,
           "max_abs_cost_difference": dev_err,
           "scipy": scipy_lsa is not None}
    for k, t in times.items():
        t = np.asarray(t)
        print("%-16s %9.3f ms per call (median of %d; %.3f .. %.3f)" % (k, np.median(t), len(t), t.min(), t.max()))
        out[k + "_ms"] = {"median": float(np.median(t)), "min": float(t.min()), "max": float(t.max()), "calls": len(t)}
    out["speedup_cost"] = out["torch_cost_ms"]["median"] / out["match_cost_ms"]["median"]
    if scipy_lsa is not None:
        out["speedup_match"] = out["torch_match_ms"]["median"] / out["hungarian_match_ms"]["median"]
        out["matchers_agree"] = bool(agree)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
