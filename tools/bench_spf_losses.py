#!/usr/bin/env python3
"""Time SPFormer's criterion on the device (``consumer_ops.spformer_criterion``: one cost launch and one synchronisation
for all heads and samples, two loss kernels forward and one backward for all heads) against a plain torch statement of
the loop it replaces (per head and sample: a cost matrix of about ten launches, a host copy and SciPy; then gathers, a
whole-block BCE, dice, the IoU, a ``where``, the level-set loss with its box test, ``nonzero``, ``unique`` and three
scatters; ``.item()`` for every reported value), on the same device, in the same run.

    python tools/bench_spf_losses.py [--batch 10] [--queries 400] [--heads 7] [--instances 40] [--spps 1500]
                                     [--feats 3] [--seconds 1.0]

The default is the released step shape (configs/boxsup_spf_scannet.yaml: batch 10, 400 queries, 6 decoder layers with
``iter_pred``: 7 prediction heads, 19 classes).  THE INSTANCE AND SUPERPOINT COUNTS ARE STAND-INS, those of the other
loss benches (40 instances and 1500 superpoints a sample), not measured on the data.

Timed between two HIP events on the stream, each form warmed up, then called in alternating blocks: forward plus
backward of the criterion (``check=True``, ``check=False`` and the torch chain, which reads its values like the
reference's ``.item()``s); the matcher alone (``spformer_match`` against the torch cost chain with SciPy); and the three
kernels singly, as ``torch.profiler`` reports their device times.  The two forms' losses and gradients are compared
first (the torch chain is float32: 1e-4 relative to each array's largest magnitude).  Prints one JSON line.  Needs the
GPU: there is no CPU timing.
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
from bench_losses import scatter_sum  # noqa: E402
from bench_spp_gt import timed  # noqa: E402

LOSS_WEIGHT = (1.0, 1.0, 1.0, 1.0, 0.5)  # Criterion.loss_weight: cls, mask BCE, dice, score, level set
N_CLASS = 18


def make_step(batch, queries, heads, instances, spps, feats, seed=0):
    """Per sample instances that share out most superpoints and whose columns mostly lie in their boxes; per head
    queries that follow one instance each."""
    rng = np.random.default_rng(seed)
    insts, coords, masks = [], [], [[] for _ in range(heads)]
    for b in range(batch):
        owner = rng.integers(0, instances + 1, spps)
        owner[rng.permutation(spps)[:instances]] = np.arange(instances)
        mask = (owner[None, :] == np.arange(instances)[:, None]).astype(np.float32)
        lo = rng.uniform(-4, 4, (instances, 3))
        box = np.concatenate([lo, lo + rng.uniform(0.3, 3, (instances, 3))], 1).astype(np.float32)
        c = rng.uniform(-5, 8, (spps, 3))
        inside = (owner < instances) & (rng.random(spps) < 0.7)
        o = owner[inside]
        c[inside] = box[o, :3] + rng.uniform(0.05, 0.95, (len(o), 3)) * (box[o, 3:] - box[o, :3])
        coords.append(c)
        insts.append({"gt_labels": rng.integers(0, N_CLASS, instances).astype(np.int64), "gt_spmasks": mask,
                      "gt_boxes": box})
        for h in range(heads):
            follows = rng.integers(0, instances, queries)
            sharp = rng.uniform(0.5, 4.0, queries)[:, None]
            masks[h].append((sharp * (2 * mask[follows] - 1) + rng.normal(0, 2.0, (queries, spps))).astype(np.float32))
    N = batch * spps
    mu = rng.uniform(0, 1, N).astype(np.float32)
    var = rng.uniform(1e-5, 0.3, N).astype(np.float32)
    mu[rng.random(N) < 0.2] = -100.0
    return {"labels": [rng.normal(0, 1.5, (batch, queries, N_CLASS + 1)).astype(np.float32) for _ in range(heads)],
            "scores": [rng.uniform(0, 1, (batch, queries, 1)).astype(np.float32) for _ in range(heads)],
            "masks": masks, "insts": insts, "sp_coords": np.concatenate(coords).astype(np.float32),
            "sp_rgb_feats": rng.uniform(0, 1, (N, feats)).astype(np.float32),
            "sp_prob_labels": rng.uniform(0.05, 1, N).astype(np.float32),
            "batch_offsets": np.arange(batch + 1, dtype=np.int64) * spps, "sp_mu_labels": mu, "sp_var_labels": var,
            "sp_mu_preds": rng.uniform(0, 1, N).astype(np.float32),
            "sp_logvar_preds": rng.normal(-1.5, 0.5, N).astype(np.float32)}


# ---- the torch chain, as a consumer writes it today ---------------------------------------------------------------------
def torch_match(labels, masks, insts):
    from scipy.optimize import linear_sum_assignment

    out = []
    for z, x, inst in zip(labels, masks, insts):
        t = inst["gt_spmasks"]
        sig = x.sigmoid()
        dice = 1 - (2 * torch.einsum("nc,mc->nm", sig, t) + 1) / (sig.sum(-1)[:, None] + t.sum(-1)[None, :] + 1)
        pos = F.binary_cross_entropy_with_logits(x, torch.ones_like(x), reduction="none")
        neg = F.binary_cross_entropy_with_logits(x, torch.zeros_like(x), reduction="none")
        bce = (torch.einsum("nc,mc->nm", pos, t) + torch.einsum("nc,mc->nm", neg, 1 - t)) / x.shape[1]
        cost = -z.softmax(-1)[:, inst["gt_labels"]] + bce + dice
        r, c = linear_sum_assignment(cost.detach().cpu())
        out.append((torch.as_tensor(r, dtype=torch.int64), torch.as_tensor(c, dtype=torch.int64)))
    return out


def torch_levelset(coords, feats, x, box, min_points=100):
    within = ((coords[None] >= box[:, None, :3] - 0.005).all(-1) & (coords[None] <= box[:, None, 3:] + 0.005).all(-1))
    some = within.sum(1) >= min_points
    box_i, point_i = torch.nonzero(within[some], as_tuple=True)
    v = torch.sigmoid(x[some][box_i, point_i])
    f = feats[point_i]
    _, norm = torch.unique(box_i, return_inverse=True)
    n = int(some.sum())
    mean = scatter_sum(f * v[:, None], norm, n) / scatter_sum(v, norm, n).clamp(min=0.00001)[:, None]
    dev = f - mean[norm]
    per_box = scatter_sum((dev * dev * v[:, None]).sum(1), norm, n) / scatter_sum(torch.ones_like(v), norm, n).clamp(min=1)
    return per_box.sum() / (len(box) + 1e-4)


def torch_head(z, score, masks, insts, d, weight, main):
    dev = z.device
    B, Q, C = z.shape
    idx = torch_match(z.detach(), [x.detach() for x in masks], insts)
    target = torch.full((B, Q), C - 1, dtype=torch.int64, device=dev)
    for b, (r, c) in enumerate(idx):
        target[b, r.to(dev)] = insts[b]["gt_labels"][c.to(dev)]
    cls = F.cross_entropy(z.transpose(1, 2), target, weight)
    out = {"cls_loss": cls.item()}
    s_loss, bce, dice, ls = (torch.zeros(1, device=dev) for _ in range(4))
    for b, (r, c) in enumerate(idx):
        s0, s1 = d["offsets"][b], d["offsets"][b + 1]
        x, t = masks[b][r], insts[b]["gt_spmasks"][c]
        with torch.no_grad():
            hit = (x.sigmoid() >= 0.5).float()
            inter = (hit * t).sum(-1)
            iou = (inter / (t.sum(-1) + hit.sum(-1) - inter + 1e-6)).unsqueeze(1)
        keep, _ = torch.where(iou > 0.5)
        if keep.numel():
            s_loss = s_loss + F.mse_loss(score[b][r][keep], iou[keep])
        w = d["sp_prob_labels"][s0:s1]
        mean = F.binary_cross_entropy_with_logits(x, t)  # as released: the mean, then sum(w) / sum(w)
        bce = bce + ((mean * w[None, :]).sum(1) / w.sum()).mean()
        sig = x.sigmoid()
        dice = dice + (1 - (2 * (sig * t).sum(-1) + 1) / (sig.sum(-1) + t.sum(-1) + 1)).mean()
        ls = ls + torch_levelset(d["sp_coords"][s0:s1], d["sp_rgb_feats"][s0:s1], x, insts[b]["gt_boxes"][c])
    s_loss, bce, ls = s_loss / B, bce / B, ls / B
    if not main:
        dice = dice / B
    out.update({"score_loss": s_loss.item(), "mask_bce_loss": bce.item(), "mask_dice_loss": dice.item(),
                "levelset_loss": ls.item()})
    lw = LOSS_WEIGHT
    return lw[0] * cls + lw[1] * bce + lw[2] * dice + lw[3] * s_loss + lw[4] * ls, out


def torch_kl(d, eps=1e-4):
    mu_l, var_l, mu_p, lv_p = d["sp_mu_labels"], d["sp_var_labels"], d["sp_mu_preds"], d["sp_logvar_preds"]
    labelled = (mu_l != -100) & (var_l != -100)
    zero, some = labelled & (var_l <= eps), labelled & (var_l > eps)
    kl = torch.zeros((), device=mu_l.device)
    if zero.sum() > 0:
        kl = kl + 0.1 * (((lv_p[zero].exp() - 1) ** 2 + (mu_p[zero] - mu_l[zero]) ** 2).sum() / (zero.sum() + 1e-4))
    if some.sum() > 0:
        term = (lv_p[some] - var_l[some].log()) + ((mu_p[some] - mu_l[some]) ** 2 + var_l[some] ** 2) \
            * (-2 * lv_p[some]).exp() - 0.5
        kl = kl + 0.1 * (term.sum() / (some.sum() + 1e-4))
    return kl


def torch_criterion(d, insts, weight):
    L1 = len(d["labels"])
    loss, out = torch_head(d["labels"][-1], d["scores"][-1], d["masks"][-1], insts, d, weight, True)
    kl = torch_kl(d)
    out["kl_loss"] = kl
    loss = loss + kl
    for h in range(L1 - 1):
        loss_h, out_h = torch_head(d["labels"][h], d["scores"][h], d["masks"][h], insts, d, weight, False)
        loss = loss + loss_h
        out.update({"layer_%d_%s" % (h, k): v for k, v in out_h.items()})
    out["loss"] = loss.item()
    return loss, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--queries", type=int, default=400)
    ap.add_argument("--heads", type=int, default=7)
    ap.add_argument("--instances", type=int, default=40, help="instances per sample (a stand-in)")
    ap.add_argument("--spps", type=int, default=1500, help="superpoints per sample (a stand-in)")
    ap.add_argument("--feats", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=1.0, help="timed window per form and block")
    ap.add_argument("--blocks", type=int, default=2, help="alternating blocks per form")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_spf_losses needs the GPU: a CPU run gives no time")
    dev = torch.device("cuda", 0)
    step = make_step(args.batch, args.queries, args.heads, args.instances, args.spps, args.feats)
    up = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    d = {k: ([[up(a) for a in head] for head in v] if k == "masks" else [up(a) for a in v] if isinstance(v, list)
             else up(v)) for k, v in step.items() if k != "insts"}
    d["offsets"] = step["batch_offsets"].tolist()
    insts = [{k: up(a) for k, a in inst.items()} for inst in step["insts"]]
    leaves = d["labels"] + d["scores"] + [x for head in d["masks"] for x in head] + [d["sp_mu_preds"], d["sp_logvar_preds"]]
    for t in leaves:
        t.requires_grad_()
    weight = torch.ones(N_CLASS + 1, device=dev)
    weight[-1] = 0.1
    pred = {k: d[k] for k in ("sp_coords", "sp_rgb_feats", "batch_offsets", "sp_prob_labels", "sp_mu_labels",
                              "sp_var_labels", "sp_mu_preds", "sp_logvar_preds")}
    pred.update({"labels": d["labels"][-1], "scores": d["scores"][-1], "masks": d["masks"][-1],
                 "aux_outputs": [{"labels": d["labels"][h], "scores": d["scores"][h], "masks": d["masks"][h]}
                                 for h in range(args.heads - 1)]})

    def step_of(fn):
        def call():
            for t in leaves:
                t.grad = None
            loss, out = fn()
            loss.sum().backward()
            return out
        return call

    ours = lambda **kw: consumer_ops.spformer_criterion(pred, insts, loss_weight=LOSS_WEIGHT,  # noqa: E731
                                                        cost_weight=(1.0, 1.0, 1.0), as_floats=True, **kw)
    forms = {"spformer_criterion": step_of(ours), "spformer_criterion_nocheck": step_of(lambda: ours(check=False)),
             "torch_criterion": step_of(lambda: torch_criterion(d, insts, weight))}
    results = {}
    for k in ("spformer_criterion", "torch_criterion"):
        out = forms[k]()
        results[k] = ({n: float(v) for n, v in out.items()}, [t.grad.double().clone() for t in leaves])
    assert list(results["spformer_criterion"][0]) == list(results["torch_criterion"][0])
    worst = max(abs(a - results["torch_criterion"][0][n]) / max(abs(a), 1e-12)
                for n, a in results["spformer_criterion"][0].items())
    for a, b in zip(*(results[k][1] for k in results)):
        worst = max(worst, float((a - b).abs().max() / a.abs().max().clamp(min=1e-30)))
    assert worst < 1e-4, worst

    labels_d, masks_d = [z.detach() for z in d["labels"]], [[x.detach() for x in head] for head in d["masks"]]
    forms["spformer_match"] = lambda: consumer_ops.spformer_match(labels_d, masks_d, insts)
    forms["torch_match"] = lambda: [torch_match(z, head, insts) for z, head in zip(labels_d, masks_d)]
    same = sum(int(a[0].equal(b[0]) and a[1].equal(b[1])) for ha, hb in zip(forms["spformer_match"](), forms["torch_match"]())
               for a, b in zip(ha, hb))
    out = {"batch": args.batch, "queries": args.queries, "heads": args.heads, "instances_per_sample": args.instances,
           "spps_per_sample": args.spps, "feats": args.feats, "max_relative_difference": worst,
           "equal_assignments": same, "assignments": args.heads * args.batch}

    from torch.profiler import ProfilerActivity, profile

    calls = 5
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            forms["spformer_criterion_nocheck"]()
        torch.cuda.synchronize()
    for e in prof.key_averages():
        for name in ("k_spf_rows", "k_spf_finish", "k_spf_backward", "k_match_cost"):
            if name in e.key:
                dt = getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0)
                out[name + "_us"] = float(dt) / max(e.count, 1)
                print("%-28s %9.1f us per launch (%d launches)" % (name, out[name + "_us"], e.count))
    times = {k: [] for k in forms}
    for _ in range(args.blocks):
        for k, fn in forms.items():
            times[k] += timed(fn, args.seconds)
    for k, t in times.items():
        t = np.asarray(t)
        print("%-28s %9.3f ms per call (median of %d; %.3f .. %.3f)" % (k, np.median(t), len(t), t.min(), t.max()))
        out[k + "_ms"] = {"median": float(np.median(t)), "min": float(t.min()), "max": float(t.max()), "calls": len(t)}
    out["speedup"] = out["torch_criterion_ms"]["median"] / out["spformer_criterion_ms"]["median"]
    out["speedup_nocheck"] = out["torch_criterion_ms"]["median"] / out["spformer_criterion_nocheck_ms"]["median"]
    out["speedup_match"] = out["torch_match_ms"]["median"] / out["spformer_match_ms"]["median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
