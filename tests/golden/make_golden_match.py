#!/usr/bin/env python3
"""Generate tests/golden/match_*.npz by running the REFERENCE's HungarianMatcher in this container.

Run from the repo root:  python tests/golden/make_golden_match.py
Needs /root/reference (read-only) and SciPy.  What is executed from the reference, on CPU tensors:
``HungarianMatcher.forward_dup`` and through it ``get_match`` (ISBNet/isbnet/model/matcher.py:144-284), imported as
they are, with the stub set-up of make_golden_spp_gt.py (``torch_scatter`` and ``isbnet.ops``, which the matcher never
calls).  ``get_match`` keeps its cost and its column indices to itself, so IN THIS HARNESS ONLY the
``linear_sum_assignment`` name of the reference's module is wrapped by a recorder that hands every call on to SciPy
unchanged and keeps the matrix it was given and the indices it returned.

A fixture holds the inputs of one batch and, per sample, the reference's float32 cost ``ref_cost``, its four index
arrays ``row``, ``col``, ``aux_row``, ``aux_col`` (dup_gt = 4; aux_col indexes the repeated instances) and, for the
batch, ``ref_dev`` = max |ref_cost - tests/match_ref.py cost|.  Per fixture this script asserts that the assignments are
separated: on the float64 restatement, 20 draws of uniform noise of +-16 ref_dev leave the main and the aux assignment
unchanged, compared as sorted (row, col % I) pairs -- a seed that fails is replaced.  Nothing of the reference's text
is written.
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

import match_ref  # noqa: E402
from make_golden_spp_gt import install_stubs  # noqa: E402

N_CLASSES = 18


def sample(rng, n_queries, n_inst, n_cols):
    """Instances that partition most of the columns, queries that follow one instance each (more or less), boxes of the
    predictions near the boxes of the instances they follow."""
    owner = rng.integers(0, n_inst + 1, n_cols)            # n_inst: a column of no instance
    assert n_inst <= n_cols
    owner[rng.permutation(n_cols)[:n_inst]] = np.arange(n_inst)  # no instance without a column
    mask = (owner[None, :] == np.arange(n_inst)[:, None]).astype(np.float32)
    cls = rng.integers(0, N_CLASSES, n_inst).astype(np.int64)
    lo = rng.uniform(-4, 4, (n_inst, 3))
    box = np.concatenate([lo, lo + rng.uniform(0.3, 3, (n_inst, 3))], 1).astype(np.float32)
    follows = rng.integers(0, n_inst, n_queries)
    sharp = rng.uniform(0.5, 4.0, n_queries)[:, None]
    mask_logits = (sharp * (2 * mask[follows] - 1) + rng.normal(0, 2.0, (n_queries, n_cols))).astype(np.float32)
    cls_logits = rng.normal(0, 1.5, (n_queries, N_CLASSES)).astype(np.float32)
    cls_logits[np.arange(n_queries), cls[follows]] += rng.uniform(0, 4, n_queries).astype(np.float32)
    conf = rng.normal(0, 1, n_queries).astype(np.float32)
    box_preds = (box[follows] + rng.normal(0, 0.4, (n_queries, 6))).astype(np.float32)
    return {"mask_logits": mask_logits, "mask": mask, "cls": cls, "box": box, "cls_logits": cls_logits, "conf": conf,
            "box_preds": box_preds}


# name -> n_queries, per sample (n_inst, n_cols) or None
CASES = {
    "two": (48, [(7, 150), (11, 230)]),                # rows > 4 x cols in both samples
    "wide": (16, [(20, 65), None, (5, 90)]),           # Q < I; a sample without instances; Q < 4 I
    "sixty_four": (64, [(33, 400)]),                   # I < Q < 4 I
}


def separated(c64, ref_dev, n_inst, seed):
    from scipy.optimize import linear_sum_assignment

    rng = np.random.default_rng(seed)
    want = [match_ref.pairs(*linear_sum_assignment(np.tile(c64, (1, d))), n_inst) for d in (1, match_ref.DUP_GT)]
    for _ in range(20):
        noisy = c64 + rng.uniform(-16 * ref_dev, 16 * ref_dev, c64.shape)
        got = [match_ref.pairs(*linear_sum_assignment(np.tile(noisy, (1, d))), n_inst) for d in (1, match_ref.DUP_GT)]
        if got != want:
            return False
    return True


def build(name, seed, matcher_mod):
    n_queries, shapes = CASES[name]
    rng = np.random.default_rng(seed)
    samples = [None if s is None else sample(rng, n_queries, *s) for s in shapes]
    B = len(samples)
    fill = next(s for s in samples if s is not None)
    stack = lambda k: np.stack([(fill if s is None else s)[k] for s in samples])  # noqa: E731
    cls_logits, conf, box_preds = stack("cls_logits"), stack("conf"), stack("box_preds")
    dc = [None if s is None else {k: torch.from_numpy(s[k]) for k in ("mask", "cls", "box")} for s in samples]
    mask_logits = [None if s is None else torch.from_numpy(s["mask_logits"]) for s in samples]

    calls = []
    real = matcher_mod.linear_sum_assignment

    def recorder(c):
        r = real(c)
        calls.append((np.array(c, copy=True), np.asarray(r[0]), np.asarray(r[1])))
        return r

    matcher_mod.linear_sum_assignment = recorder
    try:
        gt, aux = matcher_mod.HungarianMatcher().forward_dup(torch.from_numpy(cls_logits), mask_logits,
                                                             torch.from_numpy(conf), torch.from_numpy(box_preds), dc,
                                                             dup_gt=match_ref.DUP_GT)
    finally:
        matcher_mod.linear_sum_assignment = real
    arrays = {"batch_size": np.int64(B), "n_queries": np.int64(n_queries), "dup_gt": np.int64(match_ref.DUP_GT),
              "cls_logits": cls_logits, "conf_logits": conf, "box_preds": box_preds,
              "is_none": np.array([s is None for s in samples])}
    ref_dev, k = 0.0, 0
    for b, s in enumerate(samples):
        if s is None:
            assert gt["row_indices"][b] is None and aux["inst_labels"][b] is None
            continue
        (c_main, row, col), (c_aux, aux_row, aux_col) = calls[k], calls[k + 1]
        k += 2
        n_inst = len(s["cls"])
        assert c_main.dtype == np.float32 and c_main.shape == (n_queries, n_inst)
        assert np.array_equal(c_aux, np.tile(c_main, (1, match_ref.DUP_GT)))
        assert np.array_equal(gt["row_indices"][b], row) and np.array_equal(aux["row_indices"][b], aux_row)
        assert torch.equal(gt["inst_labels"][b], dc[b]["mask"][col])
        assert torch.equal(aux["cls_labels"][b], dc[b]["cls"][aux_col % n_inst])
        args = (s["cls_logits"], s["mask_logits"], s["conf"], s["box_preds"], s["mask"], s["cls"], s["box"])
        ours = match_ref.cost(*args)
        ref_dev = max(ref_dev, float(np.abs(c_main.astype(np.float64) - ours.astype(np.float64)).max()))
        arrays.update({"mask_logits_%d" % b: s["mask_logits"], "mask_%d" % b: s["mask"], "cls_%d" % b: s["cls"],
                       "box_%d" % b: s["box"], "ref_cost_%d" % b: c_main, "row_%d" % b: row.astype(np.int64),
                       "col_%d" % b: col.astype(np.int64), "aux_row_%d" % b: aux_row.astype(np.int64),
                       "aux_col_%d" % b: aux_col.astype(np.int64)})
    assert k == len(calls) and ref_dev > 0.0
    arrays["ref_dev"] = np.float64(ref_dev)
    for b, s in enumerate(samples):
        if s is None:
            continue
        c64 = match_ref.cost64(s["cls_logits"], s["mask_logits"], s["conf"], s["box_preds"], s["mask"], s["cls"],
                               s["box"])
        n_inst = len(s["cls"])
        if not separated(c64, ref_dev, n_inst, seed + 1000 + b):
            return None
        from scipy.optimize import linear_sum_assignment
        for d, (r, c) in ((1, (arrays["row_%d" % b], arrays["col_%d" % b])),
                          (match_ref.DUP_GT, (arrays["aux_row_%d" % b], arrays["aux_col_%d" % b]))):
            assert match_ref.pairs(*linear_sum_assignment(np.tile(c64, (1, d))), n_inst) == match_ref.pairs(r, c, n_inst)
    return arrays


def main():
    install_stubs()
    matcher_mod = importlib.import_module("isbnet.model.matcher")
    names = []
    for i, name in enumerate(CASES):
        seed = 9301 + 10 * i
        while True:
            arrays = build(name, seed, matcher_mod)
            if arrays is not None:
                break
            print("%s: seed %d is not separated; the next one" % (name, seed))
            seed += 1
        path = os.path.join(OUT, "match_%s.npz" % name)
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        assert size <= 300 * 1024, size
        print("%-11s seed %d  B=%d  Q=%d  shapes=%s  ref_dev=%.3g  %d bytes"
              % (name, seed, int(arrays["batch_size"]), CASES[name][0], CASES[name][1], float(arrays["ref_dev"]), size))
        names.append(name)
    assert names == match_ref.FIXTURES
    print("wrote %d cases" % len(names))


if __name__ == "__main__":
    main()
