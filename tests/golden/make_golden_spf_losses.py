#!/usr/bin/env python3
"""Generate tests/golden/spf_losses_*.npz by running the REFERENCE's SPFormer Criterion.forward in this container.

Run from the repo root:  python tests/golden/make_golden_spf_losses.py
Needs /root/reference (read-only) and SciPy.  ``SPFormer/spformer/model/loss.py`` is loaded by path, as it is, with two
stubs IN THIS HARNESS ONLY: ``gorilla`` (a registry whose decorator returns the class) and ``torch_scatter`` (the
pure-torch ``scatter`` of make_golden_losses.py).  The instances are a stand-in class with ``gt_labels``,
``gt_spmasks``, ``gt_boxes`` and ``len()``.  The real ``Criterion.forward`` (matcher, every head, KL term) runs with
autograd on CPU tensors twice: in float32 as released, and in float64 under ``torch.set_default_dtype(torch.float64)``
-- the function's own ``torch.tensor([0.0])`` accumulators are otherwise float32 and round every addition -- with
``Tensor.float`` standing for ``Tensor.double`` in that run alone (the identity on its float64 tensors; the 0 / 1 masks
of ``get_iou`` become float64, so that the IoU is not rounded to float32 on its way into ``mse_loss``).

A fixture holds the inputs, the assignments the real matcher found for every head and sample (the same in both runs:
asserted), both runs' ``loss_out`` as a table ``[L1, 5]`` (tests/spf_loss_ref.py NAMES' order, the main head last),
``kl_loss`` and ``loss``, the gradients of ``loss`` by every head's labels, scores and mask logits (the latter as their
matched rows: every other row is asserted to be exactly zero) and ``ref_dev``, |float32 run - float64 run|, per value
and per gradient array.

Asserted per fixture (a seed that fails is replaced): tests/spf_loss_ref.py equals the float64 run at least 1000 times
more closely than ``ref_dev``; every assignment survives noise of +-16 ``ref_dev`` of its cost matrix; the inputs stay
off the kinks: |x| > 1e-3, no row with 2 inter == union, every coordinate more than 1e-4 from a padded box face,
A > 1e-3.  Nothing of the reference's text is written.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, OUT)

import loss_ref  # noqa: E402
import spf_loss_ref  # noqa: E402
from make_golden_losses import install_scatter  # noqa: E402

N_CLASS, N_FEATS = 18, 3
# name -> heads, queries, per sample (the members of every instance's box, S, whether the logits follow the masks)
CASES = {
    "three": (3, 24, [((150, 101, 99, 20, 10, 5), 400, True), ((104, 9, 7, 3), 130, True)]),
    "one": (1, 16, [((60, 30, 20, 12), 130, True), ((), 150, True), ((100, 40, 25, 10, 8, 6, 5), 230, False)]),
    "wide": (2, 48, [((110, 10, 8, 6, 5, 4, 3), 150, True), ((), 140, True), ((120, 30, 20, 12, 9), 200, False)]),
}


class Insts:
    """The stand-in for the reference's Instances3D: the three fields the criterion reads, and a length."""

    def __init__(self, gt_labels, gt_spmasks, gt_boxes):
        self.gt_labels, self.gt_spmasks, self.gt_boxes = gt_labels, gt_spmasks, gt_boxes

    def __len__(self):
        return len(self.gt_labels)


def load_reference():
    gorilla = types.ModuleType("gorilla")

    class Registry:
        def register_module(self, *a, **k):
            return lambda cls: cls

    gorilla.LOSSES = Registry()
    sys.modules["gorilla"] = gorilla
    sys.modules["torch_scatter"] = types.ModuleType("torch_scatter")
    install_scatter()
    spec = importlib.util.spec_from_file_location(
        "spformer_loss", os.path.join(REF, "SPFormer", "spformer", "model", "loss.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def off_zero(rng, shape, scale):
    x = rng.normal(0.0, scale, shape)
    return np.where(np.abs(x) < 2e-3, 2e-3, x).astype(np.float32)


def make_sample(rng, n_heads, Q, sizes, S, follow):
    n = len(sizes)
    owner = np.full(S, -1)
    owner[:sum(sizes)] = np.repeat(np.arange(n), sizes)
    owner = owner[rng.permutation(S)]
    mask = (owner[None, :] == np.arange(n)[:, None]).astype(np.float32)
    centre = 3.0 * np.stack([np.arange(n) % 4, np.arange(n) // 4, np.zeros(n)], 1) + rng.uniform(-0.3, 0.3, (n, 3))
    half = rng.uniform(0.4, 1.0, (n, 3))
    box = np.concatenate([centre - half, centre + half], 1).astype(np.float32)
    coords = rng.uniform(50.0, 60.0, (S, 3))
    for s in range(S):
        if owner[s] >= 0:
            lo, hi = box[owner[s], :3].astype(np.float64), box[owner[s], 3:].astype(np.float64)
            coords[s] = lo + rng.uniform(0.05, 0.95, 3) * (hi - lo)
    heads = []
    for _ in range(n_heads):
        x = off_zero(rng, (Q, S), 2.0)
        if follow and n:
            for i, q in enumerate(rng.permutation(Q)[:n]):
                sign = np.where(rng.random(S) < 0.1, -1.0, 1.0) * (2.0 * mask[i] - 1.0)
                x[q] = (sign * rng.uniform(1.0, 4.0, S)).astype(np.float32)
        heads.append(x)
    return {"gt_labels": rng.integers(0, N_CLASS, n).astype(np.int64), "gt_spmasks": mask, "gt_boxes": box,
            "coords": coords.astype(np.float32), "feats": rng.uniform(0, 1, (S, N_FEATS)).astype(np.float32),
            "prob": rng.uniform(0.05, 1.0, S).astype(np.float32), "masks": heads, "sizes": sizes}


def run(mod, dtype, inp, samples):
    """Criterion.forward and the backward of its loss: the table, kl, loss, the assignments and the gradients."""
    L1, B = len(inp["labels"]), len(samples)
    leaf = lambda a: torch.from_numpy(a).to(dtype).requires_grad_()  # noqa: E731
    cast = lambda a: torch.from_numpy(a).to(dtype)  # noqa: E731
    labels, scores = [leaf(a) for a in inp["labels"]], [leaf(a) for a in inp["scores"]]
    masks = [[leaf(s["masks"][h]) for s in samples] for h in range(L1)]
    insts = [Insts(torch.from_numpy(s["gt_labels"]), cast(s["gt_spmasks"]), cast(s["gt_boxes"])) for s in samples]
    crit = mod.Criterion(num_class=N_CLASS)
    pred = {"labels": labels[-1], "scores": scores[-1], "masks": masks[-1], "sp_coords": cast(inp["sp_coords"]),
            "sp_rgb_feats": cast(inp["sp_rgb_feats"]), "batch_offsets": torch.from_numpy(inp["batch_offsets"]),
            "sp_prob_labels": cast(inp["sp_prob_labels"]), "sp_mu_labels": cast(inp["sp_mu_labels"]),
            "sp_var_labels": cast(inp["sp_var_labels"]), "sp_mu_preds": cast(inp["sp_mu_preds"]),
            "sp_logvar_preds": cast(inp["sp_logvar_preds"])}
    if L1 > 1:
        pred["aux_outputs"] = [{"labels": labels[h], "scores": scores[h], "masks": masks[h]} for h in range(L1 - 1)]
    loss, out = crit(pred, insts)
    loss.sum().backward()
    assert list(out) == list(spf_loss_ref.OUT_NAMES) + ["kl_loss"] + [
        "layer_%d_%s" % (i, k) for i in range(L1 - 1) for k in spf_loss_ref.OUT_NAMES] + ["loss"], list(out)
    prefix = ["layer_%d_" % i for i in range(L1 - 1)] + [""]
    table = np.array([[float(out[p + k]) for k in spf_loss_ref.NAMES] for p in prefix])
    indices = [crit.matcher(labels[h].detach(), [x.detach() for x in masks[h]], insts) for h in range(L1)]
    indices = [[(np.asarray(r, dtype=np.int64), np.asarray(c, dtype=np.int64)) for r, c in head] for head in indices]
    grads = {"labels": [z.grad.numpy() for z in labels], "scores": [s.grad.numpy() for s in scores],
             "masks": [[None if x.grad is None else x.grad.numpy() for x in head] for head in masks]}
    return table, float(out["kl_loss"]), float(out["loss"]), indices, grads


def cost_dev_and_stability(mod, rng, inp, samples, indices):
    """Per head and kept sample: the assignment is SciPy's on the float64 cost, and on 8 copies of it with noise of
    +-16 max |float32 cost - float64 cost|."""
    from scipy.optimize import linear_sum_assignment

    for h, head in enumerate(indices):
        for b, s in enumerate(samples):
            if not len(s["gt_labels"]):
                continue
            c64 = spf_loss_ref.cost_matrix(inp["labels"][h][b], s["masks"][h], s["gt_labels"], s["gt_spmasks"])
            z, x, t = (torch.from_numpy(a) for a in (inp["labels"][h][b], s["masks"][h], s["gt_spmasks"]))
            c32 = (-z.softmax(-1)[:, torch.from_numpy(s["gt_labels"])] + mod.batch_sigmoid_bce_loss(x, t)
                   + mod.batch_dice_loss(x, t)).numpy()
            dev = float(np.abs(c32.astype(np.float64) - c64).max())
            assert 0.0 < dev < 1e-4, dev
            want = tuple(np.asarray(v) for v in linear_sum_assignment(c64))
            assert np.array_equal(want[0], head[b][0]) and np.array_equal(want[1], head[b][1]), (h, b)
            for _ in range(8):
                got = linear_sum_assignment(c64 + rng.uniform(-16 * dev, 16 * dev, c64.shape))
                if not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])):
                    return False
    return True


def off_the_kinks(samples, indices):
    for h, head in enumerate(indices):
        for b, s in enumerate(samples):
            rows, cols = head[b]
            if not len(rows):
                continue
            x = s["masks"][h][rows].astype(np.float64)
            t = s["gt_spmasks"][cols].astype(np.float64)
            g = s["gt_boxes"][cols]
            pos = x >= 0
            inter = (pos * t).sum(1)
            union = pos.sum(1) + t.sum(1) - inter
            coords = s["coords"].astype(np.float64)
            faces = np.concatenate([(g[:, :3] - np.float32(0.005)).astype(np.float64),
                                    (g[:, 3:] + np.float32(0.005)).astype(np.float64)], 1)
            gap = np.abs(np.tile(coords, (1, 2))[None, :, :] - faces[:, None, :]).min()
            mem = loss_ref.members(coords, g)
            a = ((1.0 / (1.0 + np.exp(-x))) * mem).sum(1)
            if not (np.abs(x).min() > 1e-3 and (2 * inter != union).all() and gap > 1e-4
                    and a[mem.any(1)].min() > 1e-3):
                return False
    return True


def build(name, seed, mod):
    L1, Q, shapes = CASES[name]
    rng = np.random.default_rng(seed)
    samples = [make_sample(rng, L1, Q, *shape) for shape in shapes]
    B = len(samples)
    total = sum(s["coords"].shape[0] for s in samples)
    cat = lambda k: np.concatenate([s[k] for s in samples])  # noqa: E731
    var = rng.uniform(0.01, 0.3, total).astype(np.float32)
    var[rng.random(total) < 0.15] = np.float32(5e-5)
    mu = rng.uniform(0.0, 1.0, total).astype(np.float32)
    unlabelled = rng.random(total) < 0.2
    mu[unlabelled], var[unlabelled] = np.float32(-100), np.float32(-100)
    inp = {"labels": [rng.normal(0, 1.5, (B, Q, N_CLASS + 1)).astype(np.float32) for _ in range(L1)],
           "scores": [rng.uniform(0.05, 0.95, (B, Q, 1)).astype(np.float32) for _ in range(L1)],
           "sp_coords": cat("coords"), "sp_rgb_feats": cat("feats"), "sp_prob_labels": cat("prob"),
           "batch_offsets": np.cumsum([0] + [s["coords"].shape[0] for s in samples]).astype(np.int64),
           "sp_mu_labels": mu, "sp_var_labels": var, "sp_mu_preds": rng.uniform(0, 1, total).astype(np.float32),
           "sp_logvar_preds": rng.normal(-1.5, 0.5, total).astype(np.float32)}

    t32, kl32, loss32, idx32, g32 = run(mod, torch.float32, inp, samples)
    real_float = torch.Tensor.float
    torch.set_default_dtype(torch.float64)
    torch.Tensor.float = lambda self, *a, **k: self.double()  # the identity on float64; get_iou's masks: 0 / 1 exactly
    try:
        t64, kl64, loss64, idx64, g64 = run(mod, torch.float64, inp, samples)
    finally:
        torch.Tensor.float = real_float
        torch.set_default_dtype(torch.float32)
    for a, b in zip(idx32, idx64):
        for (r1, c1), (r2, c2) in zip(a, b):
            assert np.array_equal(r1, r2) and np.array_equal(c1, c2), "the two runs' assignments differ"
    if not off_the_kinks(samples, idx64) or not cost_dev_and_stability(mod, rng, inp, samples, idx64):
        return None

    # what the case is there for
    kept_any = {b: False for b in range(B)}
    counts = []
    for h in range(L1):
        for b, s in enumerate(samples):
            rows, cols = idx64[h][b]
            assert len(rows) == len(s["gt_labels"])
            if len(rows):
                x, t = s["masks"][h][rows], s["gt_spmasks"][cols]
                inter = ((x >= 0) * t).sum(1)
                kept_any[b] = kept_any[b] or bool((2 * inter > (x >= 0).sum(1) + t.sum(1) - inter).any())
                nr = loss_ref.members(s["coords"], s["gt_boxes"][cols]).sum(1)
                assert sorted(nr.tolist()) == sorted(s["sizes"])
                counts += nr.tolist()
    assert min(counts) < 100 <= max(counts), "boxes below and above min_points"
    for b, (_, _, follow) in enumerate(shapes):
        assert kept_any[b] == (follow and len(samples[b]["gt_labels"]) > 0), (name, b, kept_any)

    gts = [None if not len(s["gt_labels"]) else (s["gt_labels"], s["gt_spmasks"], s["gt_boxes"]) for s in samples]
    masks = [[s["masks"][h] for s in samples] for h in range(L1)]
    up = np.tile(spf_loss_ref.LOSS_WEIGHT, (L1, 1))
    ours, og = spf_loss_ref.layer_losses(inp["labels"], inp["scores"], masks, gts, idx64, inp["sp_coords"],
                                         inp["sp_rgb_feats"], inp["sp_prob_labels"], inp["batch_offsets"], upstream=up)
    dev_table = np.abs(t32 - t64)
    assert (np.abs(ours - t64) * 1000 <= dev_table).all(), (name, ours - t64, dev_table)
    arrays = {"n_heads": np.int64(L1), "batch_size": np.int64(B), "n_queries": np.int64(Q), "upstream": up,
              "is_skipped": np.array([g is None for g in gts]), "ref_table32": t32.astype(np.float32),
              "ref_table64": t64, "ref_kl32": np.float32(kl32), "ref_kl64": np.float64(kl64),
              "ref_loss32": np.float32(loss32), "ref_loss64": np.float64(loss64), "ref_dev_table": dev_table,
              "ref_dev_kl": np.float64(abs(kl32 - kl64)), "ref_dev_loss": np.float64(abs(loss32 - loss64))}
    arrays.update({k: v for k, v in inp.items() if k not in ("labels", "scores")})
    dev = {k: np.zeros(L1) for k in ("labels", "scores", "masks")}
    for b, s in enumerate(samples):
        arrays.update({"gt_labels_%d" % b: s["gt_labels"], "gt_spmasks_%d" % b: s["gt_spmasks"].astype(np.uint8),
                       "gt_boxes_%d" % b: s["gt_boxes"]})
    for h in range(L1):
        arrays["labels_%d" % h], arrays["scores_%d" % h] = inp["labels"][h], inp["scores"][h]
        for k in ("labels", "scores"):
            a32, a64 = g32[k][h], g64[k][h]
            dev[k][h] = np.abs(a32.astype(np.float64) - a64).max()
            assert np.abs(og[k][h].reshape(a64.shape) - a64).max() * 1000 <= dev[k][h], (name, k, h)
            arrays["ref_g%s32_%d" % (k, h)], arrays["ref_g%s64_%d" % (k, h)] = a32, a64
        for b, s in enumerate(samples):
            rows, cols = idx64[h][b]
            arrays.update({"masks_%d_%d" % (h, b): s["masks"][h], "rows_%d_%d" % (h, b): rows,
                           "cols_%d_%d" % (h, b): cols})
            if gts[b] is None:
                assert g32["masks"][h][b] is None and g64["masks"][h][b] is None and og["masks"][h][b] is None
                continue
            rest = np.setdiff1d(np.arange(Q), rows)
            m32, m64, mo = g32["masks"][h][b], g64["masks"][h][b], og["masks"][h][b]
            assert not m32[rest].any() and not m64[rest].any() and not mo[rest].any()
            dev["masks"][h] = max(dev["masks"][h], float(np.abs(m32[rows].astype(np.float64) - m64[rows]).max()))
            arrays["ref_gmasks32_%d_%d" % (h, b)], arrays["ref_gmasks64_%d_%d" % (h, b)] = m32[rows], m64[rows]
        for b in range(B):
            if gts[b] is not None:
                rows = idx64[h][b][0]
                assert np.abs(og["masks"][h][b][rows] - arrays["ref_gmasks64_%d_%d" % (h, b)]).max() * 1000 \
                    <= dev["masks"][h], (name, h, b)
    for k, v in dev.items():
        assert (v > 0.0).all(), (name, k)
        arrays["ref_dev_%s" % k] = v
    return arrays


def main():
    mod = load_reference()
    for i, name in enumerate(CASES):
        seed = 4301 + 10 * i
        while True:
            arrays = build(name, seed, mod)
            if arrays is not None:
                break
            print("%s: seed %d sits on a kink or a near-tie; the next one" % (name, seed))
            seed += 1
        path = os.path.join(OUT, "spf_losses_%s.npz" % name)
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        assert size <= 600 * 1024, size
        print("%-5s seed %d  heads=%d  B=%d  Q=%d  ref_dev table max=%s loss=%.3g labels=%.3g scores=%.3g masks=%.3g"
              "  %d bytes" % (name, seed, int(arrays["n_heads"]), int(arrays["batch_size"]), CASES[name][1],
                              np.array2string(arrays["ref_dev_table"].max(0), precision=2),
                              float(arrays["ref_dev_loss"]), arrays["ref_dev_labels"].max(),
                              arrays["ref_dev_scores"].max(), arrays["ref_dev_masks"].max(), size))
    assert list(CASES) == spf_loss_ref.FIXTURES
    print("wrote %d cases" % len(CASES))


if __name__ == "__main__":
    main()
