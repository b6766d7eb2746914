#!/usr/bin/env python3
"""Generate tests/golden/losses_*.npz by running the REFERENCE's Criterion.single_layer_loss in this container.

Run from the repo root:  python tests/golden/make_golden_losses.py
Needs /root/reference (read-only) and SciPy.  What is executed from the reference, on CPU tensors:
``HungarianMatcher.forward_dup`` (ISBNet/isbnet/model/matcher.py:208-284) for the row indices and the label lists, then
``Criterion.single_layer_loss`` (isbnet/model/criterion.py:235-331) and autograd's backward of
``sum(UPSTREAM[k] * loss[k])``, imported as they are, with the stub set-up of make_golden_spp_gt.py.  IN THIS HARNESS
ONLY ``torch_scatter.scatter`` is a pure-torch shim (``sum`` and ``mean`` along dim 0 by ``index_add``).
``Criterion.forward`` does not run as released (it passes ``cls_logits.shape[:1]`` as ``batch_size`` and ``range()`` of
a ``torch.Size`` is a ``TypeError``), so ``single_layer_loss`` is called itself, with an int.

The function runs twice: in float32 as released, and with every tensor and the criterion (``empty_weight``) cast to
float64.  ``levelset_loss`` casts three intermediates with ``.float()``; during the float64 run alone the harness makes
``Tensor.float`` the identity on float64 tensors, so that run is float64 throughout.  A fixture holds the inputs, the row
indices and labels of the reference's matcher, both runs' seven losses and four gradient sets (the mask-logit gradients
as their matched rows: the generator asserts that every other row is exactly zero) and ``ref_dev`` per loss and per
gradient array, max |float32 run - float64 run|.

Asserted per fixture (a seed that fails is replaced): tests/loss_ref.py equals the float64 run at least 1000 times more
closely than ``ref_dev``, so the restatement can stand in for the reference; and the inputs stay off the kinks where the
two runs could take different branches: |x| > 1e-3, every min / max / clamp / L1 operand pair differs by more than
1e-3, every coordinate is more than 1e-4 from a padded box face, A > 1e-3.  Nothing of the reference's text is written.
"""
import importlib
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, OUT)

import loss_ref  # noqa: E402
from make_golden_match import sample  # noqa: E402
from make_golden_spp_gt import install_stubs  # noqa: E402

N_FEATS = 3
# name -> n_queries, per sample (n_inst, n_cols) or None, (sample, instance) of the box that holds no column
CASES = {
    "two": (48, [(7, 150), (11, 230)], (1, 3)),
    "wide": (16, [(20, 65), None, (5, 90)], None),
    "long": (32, [(12, 400)], None),
}


def install_scatter():
    def scatter(src, index, dim=-1, reduce="sum"):
        assert dim in (0, -1) and (dim == 0 or src.dim() == 1) and reduce in ("sum", "mean")
        n = int(index.max()) + 1 if index.numel() else 0
        out = torch.zeros((n,) + tuple(src.shape[1:]), dtype=src.dtype).index_add(0, index, src)
        if reduce == "mean":
            cnt = torch.zeros(n, dtype=src.dtype).index_add(0, index, torch.ones(src.shape[0], dtype=src.dtype))
            out = out / (cnt.clamp(min=1)[:, None] if out.dim() > 1 else cnt.clamp(min=1))
        return out

    sys.modules["torch_scatter"].scatter = scatter


def geometry(rng, s, far):
    """Coordinates, features and weights of a sample's columns: most columns of an instance lie inside its box."""
    mask, box = s["mask"], s["box"].copy()
    n_cols = mask.shape[1]
    owner = np.where(mask.sum(0) > 0, mask.argmax(0), -1)
    coords = rng.uniform(-5, 8, (n_cols, 3))
    for c in range(n_cols):
        if owner[c] >= 0 and rng.random() < 0.7:
            lo, hi = box[owner[c], :3], box[owner[c], 3:]
            coords[c] = lo + rng.uniform(0.05, 0.95, 3) * (hi - lo)
    if far is not None:
        box[far] += np.float32(60.0)
        s["box"] = box
    s["coords"] = coords.astype(np.float32)
    s["feats"] = rng.uniform(0, 1, (n_cols, N_FEATS)).astype(np.float32)
    s["prob"] = rng.uniform(0.05, 1.0, n_cols).astype(np.float32)


def run(crit, dtype, inputs, gt, n_batch):
    """single_layer_loss and the backward of the weighted sum: losses [7] and the four gradient sets, as NumPy."""
    cast = lambda a: None if a is None else torch.from_numpy(a).to(dtype)  # noqa: E731
    leaf = lambda a: None if a is None else cast(a).requires_grad_()  # noqa: E731
    cls_logits, conf, box_preds = leaf(inputs["cls_logits"]), leaf(inputs["conf_logits"]), leaf(inputs["box_preds"])
    mask_logits = [leaf(a) for a in inputs["mask_logits"]]
    out = crit.to(dtype).single_layer_loss(
        cls_logits, mask_logits, conf, box_preds, cast(inputs["prob_labels"]), inputs["batch_offsets"].tolist(),
        cast(inputs["levelset_feats"]), cast(inputs["levelset_coords"]), gt["row_indices"],
        gt["cls_labels"], [None if t is None else t.to(dtype) for t in gt["inst_labels"]],
        [None if t is None else t.to(dtype) for t in gt["box_labels"]], n_batch)
    assert set(loss_ref.NAMES) < set(out) and all(out[k].dtype == dtype for k in loss_ref.NAMES)
    sum(float(u) * out[k] for u, k in zip(loss_ref.UPSTREAM, loss_ref.NAMES)).backward()
    grads = {"cls": cls_logits.grad.numpy(), "conf": conf.grad.numpy(), "box": box_preds.grad.numpy(),
             "mask": [None if x is None or x.grad is None else x.grad.numpy() for x in mask_logits]}
    return np.array([out[k].item() for k in loss_ref.NAMES], dtype=np.float64), grads


def off_the_kinks(inputs, gt):
    for b, rows in enumerate(gt["row_indices"]):
        if rows is None:
            continue
        s0, s1 = inputs["batch_offsets"][b:b + 2]
        x = inputs["mask_logits"][b][rows].astype(np.float64)
        p = inputs["box_preds"][b][rows].astype(np.float64)
        g = gt["box_labels"][b].numpy().astype(np.float64)
        a0, a1, b0, b1 = p[:, :3], p[:, 3:], g[:, :3], g[:, 3:]
        pairs = [a1 - b1, a0 - b0, np.minimum(a1, b1) - np.maximum(a0, b0), a1 - a0, b1 - b0,
                 np.maximum(a1, b1) - np.minimum(a0, b0)]
        coords = inputs["levelset_coords"][s0:s1].astype(np.float64)
        faces = np.concatenate([(g[:, :3].astype(np.float32) - np.float32(0.005)).astype(np.float64),
                                (g[:, 3:].astype(np.float32) + np.float32(0.005)).astype(np.float64)], 1)
        gap = np.abs(np.tile(coords, (1, 2))[None, :, :] - faces[:, None, :]).min()
        mem = loss_ref.members(coords, g)
        sig = 1.0 / (1.0 + np.exp(-x))
        a = (sig * mem).sum(1)
        if not (np.abs(x).min() > 1e-3 and min(np.abs(v).min() for v in pairs) > 1e-3 and gap > 1e-4
                and a[mem.any(1)].min() > 1e-3):
            return False
    return True


def build(name, seed, matcher_mod, crit_mod):
    n_queries, shapes, far = CASES[name]
    rng = np.random.default_rng(seed)
    samples = [None if s is None else sample(rng, n_queries, *s) for s in shapes]
    for b, s in enumerate(samples):
        if s is not None:
            geometry(rng, s, far[1] if far is not None and far[0] == b else None)
    B = len(samples)
    fill = next(s for s in samples if s is not None)
    stack = lambda k: np.stack([(fill if s is None else s)[k] for s in samples])  # noqa: E731
    cat = lambda k: np.concatenate([s[k] for s in samples if s is not None])  # noqa: E731
    offsets = np.cumsum([0] + [0 if s is None else s["mask"].shape[1] for s in samples]).astype(np.int64)
    inputs = {"cls_logits": stack("cls_logits"), "conf_logits": stack("conf"), "box_preds": stack("box_preds"),
              "mask_logits": [None if s is None else s["mask_logits"] for s in samples], "prob_labels": cat("prob"),
              "batch_offsets": offsets, "levelset_feats": cat("feats"), "levelset_coords": cat("coords")}
    dc = [None if s is None else {k: torch.from_numpy(s[k]) for k in ("mask", "cls", "box")} for s in samples]
    with torch.no_grad():
        gt, _ = matcher_mod.HungarianMatcher().forward_dup(
            torch.from_numpy(inputs["cls_logits"]), [None if x is None else torch.from_numpy(x)
                                                     for x in inputs["mask_logits"]],
            torch.from_numpy(inputs["conf_logits"]), torch.from_numpy(inputs["box_preds"]), dc, dup_gt=4)
    gt = {k: list(gt[k]) for k in ("row_indices", "inst_labels", "cls_labels", "box_labels")}
    gt["row_indices"] = [None if r is None else np.asarray(r, dtype=np.int64) for r in gt["row_indices"]]
    if not off_the_kinks(inputs, gt):
        return None
    if far is not None:
        g = gt["box_labels"][far[0]].numpy()
        mem = loss_ref.members(samples[far[0]]["coords"], g)
        assert (~mem.any(1)).sum() >= 1 and mem.any(1).sum() >= 1, "a box without a column, and one with"

    crit = crit_mod.Criterion(instance_classes=inputs["cls_logits"].shape[2] - 1)
    l32, g32 = run(crit, torch.float32, inputs, gt, B)
    real_float = torch.Tensor.float
    torch.Tensor.float = lambda self, *a, **k: self if self.dtype == torch.float64 else real_float(self, *a, **k)
    try:
        l64, g64 = run(crit, torch.float64, inputs, gt, B)
    finally:
        torch.Tensor.float = real_float
    weight = crit.empty_weight.float().numpy()
    assert np.array_equal(weight, loss_ref.default_weight(len(weight)))

    gt_np = {k: [None if t is None else np.asarray(t) for t in gt[k]] for k in gt}
    ours, og = loss_ref.losses(inputs["cls_logits"], inputs["mask_logits"], inputs["conf_logits"], inputs["box_preds"],
                               inputs["prob_labels"], offsets, inputs["levelset_feats"], inputs["levelset_coords"],
                               gt_np, upstream=loss_ref.UPSTREAM)
    arrays = {"batch_size": np.int64(B), "n_queries": np.int64(n_queries), "upstream": loss_ref.UPSTREAM,
              "is_none": np.array([s is None for s in samples]), "ref_losses32": l32.astype(np.float32),
              "ref_losses64": l64}
    arrays.update({k: v for k, v in inputs.items() if k != "mask_logits"})
    dev = {"losses": np.abs(l32 - l64)}
    assert (np.abs(ours - l64) * 1000 <= dev["losses"]).all(), (name, ours - l64, dev["losses"])
    for k in ("cls", "conf", "box"):
        dev[k] = np.abs(g32[k].astype(np.float64) - g64[k]).max()
        assert np.abs(og[k] - g64[k]).max() * 1000 <= dev[k], (name, k)
        arrays["ref_g%s32" % k], arrays["ref_g%s64" % k] = g32[k], g64[k]
    dev["mask"] = 0.0
    for b, s in enumerate(samples):
        if s is None:
            assert gt["row_indices"][b] is None and g32["mask"][b] is None
            continue
        rows = gt["row_indices"][b]
        rest = np.setdiff1d(np.arange(n_queries), rows)
        assert not g32["mask"][b][rest].any() and not g64["mask"][b][rest].any() and not og["mask"][b][rest].any()
        m32, m64 = g32["mask"][b][rows], g64["mask"][b][rows]
        dev["mask"] = max(dev["mask"], float(np.abs(m32.astype(np.float64) - m64).max()))
        arrays.update({"mask_logits_%d" % b: s["mask_logits"], "row_%d" % b: rows, "inst_%d" % b: gt_np["inst_labels"][b],
                       "cls_%d" % b: gt_np["cls_labels"][b], "box_%d" % b: gt_np["box_labels"][b],
                       "ref_gmask32_%d" % b: m32, "ref_gmask64_%d" % b: m64})
    for b, s in enumerate(samples):
        if s is not None:
            rows = gt["row_indices"][b]
            assert np.abs(og["mask"][b][rows] - arrays["ref_gmask64_%d" % b]).max() * 1000 <= dev["mask"], (name, b)
    for k, v in dev.items():
        assert np.all(np.asarray(v) > 0.0) or k == "losses", (name, k)
        arrays["ref_dev_%s" % k] = np.asarray(v, dtype=np.float64)
    return arrays


def main():
    install_stubs()
    install_scatter()
    matcher_mod = importlib.import_module("isbnet.model.matcher")
    crit_mod = importlib.import_module("isbnet.model.criterion")
    for i, name in enumerate(CASES):
        seed = 9701 + 10 * i
        while True:
            arrays = build(name, seed, matcher_mod, crit_mod)
            if arrays is not None:
                break
            print("%s: seed %d sits on a kink; the next one" % (name, seed))
            seed += 1
        path = os.path.join(OUT, "losses_%s.npz" % name)
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        assert size <= 300 * 1024, size
        print("%-5s seed %d  B=%d  Q=%d  shapes=%s  ref_dev losses=%s cls=%.3g mask=%.3g conf=%.3g box=%.3g  %d bytes"
              % (name, seed, int(arrays["batch_size"]), CASES[name][0], CASES[name][1],
                 np.array2string(arrays["ref_dev_losses"], precision=2), float(arrays["ref_dev_cls"]),
                 float(arrays["ref_dev_mask"]), float(arrays["ref_dev_conf"]), float(arrays["ref_dev_box"]), size))
    assert list(CASES) == loss_ref.FIXTURES
    print("wrote %d cases" % len(CASES))


if __name__ == "__main__":
    main()
