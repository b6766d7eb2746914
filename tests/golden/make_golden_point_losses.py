#!/usr/bin/env python3
"""Generate tests/golden/point_losses_*.npz and criterion_two.npz by running the REFERENCE's Criterion in this container.

Run from the repo root:  python tests/golden/make_golden_point_losses.py
Needs /root/reference (read-only) and SciPy.  What is executed from the reference, on CPU tensors, imported as it is with
the stub set-up of make_golden_spp_gt.py (and make_golden_losses.py's pure-torch ``torch_scatter.scatter``):

``point_losses_*``: ``Criterion.cal_point_wise_loss`` (ISBNet/isbnet/model/criterion.py:136-191) and autograd's backward
of ``sum(UPSTREAM[k] * loss[k])``, twice: in float32 as released, and with every floating-point tensor cast to float64
(``cal_point_wise_loss`` builds its class weights with ``dtype=torch.float``; the float64 run hands it a criterion whose
``semantic_weight`` is ``None`` and patches ``F.cross_entropy``'s ``weight`` argument with the float64 weights, so that
run is float64 throughout).  A fixture holds the inputs, both runs' four losses and three gradient arrays and ``ref_dev``
per loss and per gradient array, max |float32 run - float64 run|.
  mixed     N = 700, C = 20, about 60 % positive, about 5 % of the semantic labels ignored
  weighted  N = 300, C = 13, with a semantic_weight
  nopos     N = 130, every instance label ignored
Asserted per fixture (a seed that fails is replaced): tests/point_loss_ref.py equals the float64 run at least 1000 times
more closely than ``ref_dev``; every L1 pair and every min / max / clamp operand pair of the boxes differs by more than
1e-3.  Also asserted, once: with every semantic label ignored torch's loss is NaN and its backward gives ZEROS for the
scores (not NaN), which is what the kernel does.

``criterion_two``: the whole ``Criterion.forward`` with ``trainall=True`` on the ``two`` shapes of make_golden_losses.py
plus point-wise inputs of N = 400 and KL inputs.  ``forward`` does not run as released (it passes
``cls_logits.shape[:1]`` as ``batch_size``), so it runs through a subclass defined here whose ``single_layer_loss`` turns
the ``torch.Size`` into an int and calls the parent.  All twelve returned values in float32 and float64 and their
``ref_dev``.  Nothing of the reference's text is written.
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

import point_loss_ref as ref  # noqa: E402
import make_golden_losses as mgl  # noqa: E402
from make_golden_match import sample  # noqa: E402
from make_golden_spp_gt import install_stubs  # noqa: E402

IGNORE = -100
# name -> N, C, share of positive instance labels, share of ignored semantic labels, with class weights
CASES = {"mixed": (700, 20, 0.6, 0.05, False), "weighted": (300, 13, 0.6, 0.05, True), "nopos": (130, 20, 0.0, 0.05, False)}
KEYS = ("pw_sem_loss", "pw_corners_loss", "pw_giou_loss", "pw_conf_loss", "dice_loss", "bce_loss", "cls_loss",
        "iou_loss", "box_loss", "giou_loss", "levelset_loss", "kl_loss")


def point_inputs(rng, N, C, p_pos, p_ignore):
    """Voxels of a few boxes: label corners around the point, predicted corners near them."""
    xyz = rng.uniform(-6, 6, (N, 3))
    lab = np.concatenate([-rng.uniform(0.2, 2.5, (N, 3)), rng.uniform(0.2, 2.5, (N, 3))], 1)
    pred = lab + rng.choice([-1.0, 1.0], (N, 6)) * rng.uniform(0.01, 0.6, (N, 6))  # no L1 pair near its kink
    sem = rng.integers(0, C, N)
    sem[rng.random(N) < p_ignore] = IGNORE
    inst = rng.integers(0, 9, N)
    inst[rng.random(N) >= p_pos] = IGNORE
    z = rng.normal(0, 2.0, (N, C))
    hit = sem != IGNORE
    z[hit, sem[hit]] += rng.uniform(0, 4, int(hit.sum()))
    return {"semantic_scores": z.astype(np.float32), "corners_offset": pred.astype(np.float32),
            "box_conf": rng.uniform(0, 1, N).astype(np.float32), "semantic_labels": sem.astype(np.int64),
            "instance_labels": inst.astype(np.int64), "corners_offset_labels": lab.astype(np.float32),
            "coords_float": xyz.astype(np.float32)}


def off_the_kinks(inp):
    pos = inp["instance_labels"] != IGNORE
    if not pos.any():
        return True
    c, l = inp["corners_offset"].astype(np.float64)[pos], inp["corners_offset_labels"].astype(np.float64)[pos]
    for a, b in (ref.boxes(c, l, inp["coords_float"][pos]),  # the float64 boxes
                 ((inp["corners_offset"][pos] + np.tile(inp["coords_float"][pos], (1, 2))).astype(np.float64),
                  (inp["corners_offset_labels"][pos] + np.tile(inp["coords_float"][pos], (1, 2))).astype(np.float64))):
        a0, a1, b0, b1 = a[:, :3], a[:, 3:], b[:, :3], b[:, 3:]
        pairs = [a1 - b1, a0 - b0, np.minimum(a1, b1) - np.maximum(a0, b0), a1 - a0, b1 - b0,
                 np.maximum(a1, b1) - np.minimum(a0, b0)]
        if min(np.abs(v).min() for v in pairs) <= 1e-3:
            return False
    return np.abs(c - l).min() > 1e-3


def run_point(crit_mod, dtype, inp, weight):
    """cal_point_wise_loss and the backward of the weighted sum: losses [4] and the three gradient arrays, as NumPy."""
    import torch.nn.functional as F

    leaf = lambda k: torch.from_numpy(inp[k]).to(dtype).requires_grad_()  # noqa: E731
    z, c, conf = leaf("semantic_scores"), leaf("corners_offset"), leaf("box_conf")
    released = dtype == torch.float32
    crit = crit_mod.Criterion(instance_classes=inp["semantic_scores"].shape[1] - 2,
                              semantic_weight=list(map(float, weight)) if weight is not None and released else None)
    real = F.cross_entropy
    if not released and weight is not None:
        w64 = torch.from_numpy(weight.astype(np.float64))
        crit_mod.F.cross_entropy = lambda *a, **k: real(*a, **{**k, "weight": w64})
    try:
        out = crit.cal_point_wise_loss(z, c, conf, torch.from_numpy(inp["semantic_labels"]),
                                       torch.from_numpy(inp["instance_labels"]),
                                       torch.from_numpy(inp["corners_offset_labels"]).to(dtype),
                                       torch.from_numpy(inp["coords_float"]).to(dtype))
    finally:
        crit_mod.F.cross_entropy = real
    assert list(out) == list(ref.NAMES) and all(out[k].dtype == dtype for k in ref.NAMES)
    sum(float(u) * out[k] for u, k in zip(ref.UPSTREAM, ref.NAMES)).backward()
    grads = {"scores": z.grad.numpy(), "corners": c.grad.numpy(), "conf": conf.grad.numpy()}
    return np.array([out[k].item() for k in ref.NAMES], dtype=np.float64), grads


def build_point(name, seed, crit_mod):
    N, C, p_pos, p_ignore, weighted = CASES[name]
    rng = np.random.default_rng(seed)
    inp = point_inputs(rng, N, C, p_pos, p_ignore)
    weight = rng.uniform(0.3, 2.0, C).astype(np.float32) if weighted else None
    if not off_the_kinks(inp):
        return None
    l32, g32 = run_point(crit_mod, torch.float32, inp, weight)
    l64, g64 = run_point(crit_mod, torch.float64, inp, weight)
    ours, og = ref.losses(semantic_weight=weight, upstream=ref.UPSTREAM, **inp)
    arrays = dict(inp)
    arrays.update({"upstream": ref.UPSTREAM, "ref_losses32": l32.astype(np.float32), "ref_losses64": l64,
                   "ref_dev_losses": np.abs(l32 - l64)})
    if weight is not None:
        arrays["semantic_weight"] = weight
    n_pos = int((inp["instance_labels"] != IGNORE).sum())
    assert (np.abs(ours - l64) * 1000 <= arrays["ref_dev_losses"]).all(), (name, ours - l64, arrays["ref_dev_losses"])
    for k in ("scores", "corners", "conf"):
        dev = np.abs(g32[k].astype(np.float64) - g64[k]).max()
        assert np.abs(og[k] - g64[k]).max() * 1000 <= dev, (name, k, np.abs(og[k] - g64[k]).max(), dev)
        assert dev > 0.0 or (n_pos == 0 and k != "scores"), (name, k)
        arrays["ref_g%s32" % k], arrays["ref_g%s64" % k], arrays["ref_dev_%s" % k] = g32[k], g64[k], np.float64(dev)
    if n_pos == 0:
        assert not l32[1:].any() and not g32["corners"].any() and not g32["conf"].any()
    return arrays


def all_ignored(crit_mod):
    """What torch does when every semantic label is ignored: the loss is NaN, the backward gives zeros."""
    rng = np.random.default_rng(5)
    inp = point_inputs(rng, 40, 7, 0.5, 0.0)
    inp["semantic_labels"][:] = IGNORE
    for dtype in (torch.float32, torch.float64):
        losses, grads = run_point(crit_mod, dtype, inp, None)
        assert np.isnan(losses[0]) and np.isfinite(losses[1:]).all()
        assert not grads["scores"].any() and not np.isnan(grads["scores"]).any()
    ours, og = ref.losses(upstream=ref.UPSTREAM, **inp)
    assert np.isnan(ours[0]) and not og["scores"].any()


def build_criterion(crit_mod):
    """Criterion.forward, trainall, on the `two` shapes of make_golden_losses.py."""
    class Runs(crit_mod.Criterion):
        def single_layer_loss(self, *args):
            return super().single_layer_loss(*args[:-1], int(args[-1][0]))

    name = "two"
    n_queries, shapes, far = mgl.CASES[name]
    seed = 9701
    while mgl.build(name, seed, importlib.import_module("isbnet.model.matcher"), crit_mod) is None:
        seed += 1
    rng = np.random.default_rng(seed)
    samples = [sample(rng, n_queries, *s) for s in shapes]
    for b, s in enumerate(samples):
        mgl.geometry(rng, s, far[1] if far is not None and far[0] == b else None)
    rng = np.random.default_rng(seed + 1000)
    pw_seed = 4400
    while True:
        pw = point_inputs(np.random.default_rng(pw_seed), 400, 20, 0.6, 0.05)
        if off_the_kinks(pw):
            break
        pw_seed += 1
    stack = lambda k: np.stack([s[k] for s in samples])  # noqa: E731
    cat = lambda k: np.concatenate([s[k] for s in samples])  # noqa: E731
    offsets = np.cumsum([0] + [s["mask"].shape[1] for s in samples]).astype(np.int64)
    S = int(offsets[-1])
    mu_l, var_l = rng.uniform(0, 1, S), rng.uniform(0.01, 0.3, S)
    var_l[rng.random(S) < 0.3] = 0.0
    hole = rng.random(S) < 0.15
    mu_l[hole], var_l[hole] = -100.0, -100.0
    arrays = {"batch_size": np.int64(len(samples)), "n_queries": np.int64(n_queries), "batch_offsets": offsets,
              "cls_logits": stack("cls_logits"), "conf_logits": stack("conf"), "box_preds": stack("box_preds"),
              "dc_prob_labels": cat("prob"), "dc_rgb_feats": cat("feats"), "dc_coords_float": cat("coords"),
              "dc_mu_labels": mu_l.astype(np.float32), "dc_var_labels": var_l.astype(np.float32),
              "mu_pred": rng.uniform(0, 1, S).astype(np.float32), "logvar_pred": rng.normal(-2, 1, S).astype(np.float32)}
    for b, s in enumerate(samples):
        arrays.update({"mask_logits_%d" % b: s["mask_logits"], "mask_%d" % b: s["mask"], "cls_%d" % b: s["cls"],
                       "box_%d" % b: s["box"]})
    arrays.update({"pw_" + k: v for k, v in pw.items()})

    def forward(dtype):
        t = lambda a: torch.from_numpy(a).to(dtype) if a.dtype == np.float32 else torch.from_numpy(a)  # noqa: E731
        crit = Runs(instance_classes=arrays["cls_logits"].shape[2] - 1, semantic_only=False, trainall=True).to(dtype)
        batch = {"semantic_labels": t(pw["semantic_labels"]), "instance_labels": t(pw["instance_labels"]),
                 "coords_float": t(pw["coords_float"]), "corners_offset_labels": t(pw["corners_offset_labels"])}
        model = {k: t(pw[k]) for k in ("semantic_scores", "corners_offset", "box_conf")}
        model.update({k: t(arrays[k]) for k in ("cls_logits", "conf_logits", "box_preds", "dc_prob_labels",
                                                "dc_rgb_feats", "dc_coords_float", "dc_mu_labels", "dc_var_labels",
                                                "mu_pred", "logvar_pred")})
        model["mask_logits"] = [t(s["mask_logits"]) for s in samples]
        model["dc_inst_mask_arr"] = [{k: t(s[k]) for k in ("mask", "cls", "box")} for s in samples]
        model["dc_batch_offsets"] = offsets.tolist()
        with torch.no_grad():
            out = crit(batch, model)
        assert list(out) == list(KEYS), list(out)
        return np.array([float(out[k]) for k in KEYS], dtype=np.float64)

    v32 = forward(torch.float32)
    real_float = torch.Tensor.float
    torch.Tensor.float = lambda self, *a, **k: self if self.dtype == torch.float64 else real_float(self, *a, **k)
    try:
        v64 = forward(torch.float64)
    finally:
        torch.Tensor.float = real_float
    arrays.update({"ref_values32": v32.astype(np.float32), "ref_values64": v64, "ref_dev": np.abs(v32 - v64)})
    return arrays


def save(name, arrays):
    path = os.path.join(OUT, name)
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size <= 300 * 1024, size
    return size


def main():
    install_stubs()
    mgl.install_scatter()
    crit_mod = importlib.import_module("isbnet.model.criterion")
    all_ignored(crit_mod)
    print("every semantic label ignored: the loss is NaN, torch's backward gives zeros")
    for i, name in enumerate(CASES):
        seed = 8801 + 10 * i
        while True:
            arrays = build_point(name, seed, crit_mod)
            if arrays is not None:
                break
            print("%s: seed %d sits on a kink; the next one" % (name, seed))
            seed += 1
        size = save("point_losses_%s.npz" % name, arrays)
        print("%-8s seed %d  N=%d C=%d  ref_dev losses=%s scores=%.3g corners=%.3g conf=%.3g  %d bytes"
              % (name, seed, CASES[name][0], CASES[name][1], np.array2string(arrays["ref_dev_losses"], precision=2),
                 float(arrays["ref_dev_scores"]), float(arrays["ref_dev_corners"]), float(arrays["ref_dev_conf"]), size))
    assert list(CASES) == ref.FIXTURES
    arrays = build_criterion(crit_mod)
    size = save("criterion_two.npz", arrays)
    print("criterion_two  ref_dev=%s  %d bytes" % (np.array2string(arrays["ref_dev"], precision=2), size))


if __name__ == "__main__":
    main()
