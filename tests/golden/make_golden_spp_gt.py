#!/usr/bin/env python3
"""Generate tests/golden/spp_gt_*.npz by running the REFERENCE's get_spp_gt and get_subsample_gt in this container.

Run from the repo root:  python tests/golden/make_golden_spp_gt.py
Needs /root/reference (read-only).  What is executed from the reference, on CPU tensors: ``get_spp_gt``
(ISBNet/isbnet/model/model_utils.py:692-738) and ``get_subsample_gt`` (:647-689), imported as they are.
``torch_scatter`` is not installed here; it is replaced IN THIS HARNESS ONLY by the pure-torch shim
make_golden_consumer.py uses (float32 sums, count clamped at 1 -- the CPU semantics of torch_scatter.scatter_mean).
``isbnet.ops`` (a compiled extension model_utils imports but these functions never call) is an empty stub.

The fixtures hold the inputs and, per sample, what the functions returned: ``is_none[b]``, ``mask_b``, ``cls_b``,
``box_b``.  The restatement tests/spp_gt_ref.py is run on the same inputs and must agree exactly.  Nothing of the
reference's text is written.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference/ISBNet"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(REPO, "tests"))

import spp_gt_ref  # noqa: E402


def install_stubs():
    ts = types.ModuleType("torch_scatter")

    def scatter_mean(src, index, dim=0, out=None, dim_size=None):
        assert dim == 0 and out is None
        n = int(index.max()) + 1 if dim_size is None else dim_size
        res = torch.zeros((n,) + tuple(src.shape[1:]), dtype=src.dtype).index_add_(0, index, src)
        cnt = torch.zeros(n, dtype=src.dtype).index_add_(0, index, torch.ones(src.shape[0], dtype=src.dtype))
        cnt.clamp_(1)
        return res / (cnt[:, None] if res.dim() > 1 else cnt)

    ts.scatter_mean = scatter_mean
    sys.modules["torch_scatter"] = ts
    pkg = types.ModuleType("isbnet")
    pkg.__path__ = [os.path.join(REF, "isbnet")]
    ops = types.ModuleType("isbnet.ops")
    ops.ballquery_batchflat = None
    model = types.ModuleType("isbnet.model")
    model.__path__ = [os.path.join(REF, "isbnet", "model")]
    sys.modules.update({"isbnet": pkg, "isbnet.ops": ops, "isbnet.model": model})


def batch(seed, sizes, n_inst, n_spp, p_ignore=0.25, n_neg_cls=2, shared_spp=False, empty=()):
    """A batch like ISBNet's: per sample its own instance ids (consecutive over the batch, as the collate function
    hands them out) and superpoints that are runs of points, mostly inside one instance."""
    rng = np.random.default_rng(seed)
    labels, spps, off = [], [], [0]
    total_inst = n_inst * len(sizes)
    cls = rng.integers(0, 18, total_inst).astype(np.int64)
    cls[rng.permutation(total_inst)[:n_neg_cls]] = -100
    box = rng.uniform(-8, 8, (total_inst, 6)).astype(np.float32)
    spp0 = 0
    for b, n in enumerate(sizes):
        cuts = np.sort(rng.permutation(np.arange(1, n))[:n_spp - 1])
        spp = np.repeat(np.arange(n_spp), np.diff(np.r_[0, cuts, n]))
        owner = rng.integers(0, n_inst, n_spp) + b * n_inst          # the instance most of a superpoint belongs to
        lab = owner[spp]
        noise = rng.random(n) < 0.15                                  # points of another instance of the sample
        lab[noise] = rng.integers(0, n_inst, int(noise.sum())) + b * n_inst
        lab[rng.random(n) < p_ignore] = -100
        if b in empty:
            lab[:] = -100
        perm = rng.permutation(n_spp)                                 # superpoint ids in no order along the points
        labels.append(lab)
        spps.append(perm[spp] + (0 if shared_spp else spp0))
        spp0 += 0 if shared_spp else n_spp
        off.append(off[-1] + n)
    return (np.concatenate(labels).astype(np.int64), np.concatenate(spps).astype(np.int64), cls, box,
            np.asarray(off, dtype=np.int64))


def half_splits(seed):
    """Superpoints of 2, 4 and 6 points split exactly in half between two instances, between an instance and ignored
    points, and between an instance and one whose class is negative; superpoints of 3 with 1 and 2 points."""
    labels, spps, cls, box, off = batch(seed, [600, 500], 6, 40, p_ignore=0.1, n_neg_cls=0)
    cls[3] = -100
    s = int(spps.max()) + 1
    extra_lab = [0, 0, 1, 1,  2, -100,  4, 4, 4, 5, 5, 5,  3, 0,  1, 2, 2,  -100, -100, 0]
    extra_spp = [s] * 4 + [s + 1] * 2 + [s + 2] * 6 + [s + 3] * 2 + [s + 4] * 3 + [s + 5] * 3
    labels = np.r_[labels[:off[1]], extra_lab, labels[off[1]:]].astype(np.int64)
    spps = np.r_[spps[:off[1]], extra_spp, spps[off[1]:]].astype(np.int64)
    off = off.copy()
    off[1:] += len(extra_lab)
    return labels, spps, cls, box, off


# name -> (labels, spps or subsample_idxs, cls, box, offsets), mode
def cases():
    yield "two", batch(9101, [2500, 1800], 12, 160), "spp"
    yield "four", batch(9102, [1500, 900, 1300, 1100], 10, 120), "spp"
    yield "second_empty", batch(9103, [1200, 700, 900], 8, 90, empty=(1,)), "spp"
    yield "shared_spp", batch(9104, [1000, 1400], 9, 100, shared_spp=True), "spp"
    yield "half_splits", half_splits(9105), "spp"
    labels, _, cls, box, _ = batch(9106, [2000, 1600, 1200], 10, 100)
    rng = np.random.default_rng(9107)
    idxs = np.concatenate([rng.permutation(2000)[:700], 2000 + rng.integers(0, 1600, 500),
                           3600 + rng.permutation(1200)[:300]]).astype(np.int64)
    yield "subsample", (labels, idxs, cls, box, np.asarray([0, 700, 1200, 1500], dtype=np.int64)), "subsample"


def main():
    install_stubs()
    mu = importlib.import_module("isbnet.model.model_utils")
    names = []
    for name, (labels, second, cls, box, off), mode in cases():
        B = len(off) - 1
        t = [torch.from_numpy(a) for a in (labels, second, cls, box, off)]
        if mode == "spp":
            got = mu.get_spp_gt(t[0], t[1], t[2], t[3], t[4], B, ignore_label=-100, pool=True)
            ours = spp_gt_ref.get_spp_gt(labels, second, cls, box, off, B)
        else:
            got = mu.get_subsample_gt(t[0], t[1], t[2], t[3], t[4], B, ignore_label=-100)
            ours = spp_gt_ref.get_subsample_gt(labels, second, cls, box, off, B)
        got = [None if g is None else {k: v.numpy() for k, v in g.items()} for g in got]
        spp_gt_ref.same(ours, got)
        arrays = {"labels": labels, ("spps" if mode == "spp" else "subsample_idxs"): second, "cls": cls, "box": box,
                  "offsets": off, "batch_size": np.int64(B), "is_none": np.array([g is None for g in got])}
        for b, g in enumerate(got):
            if g is not None:
                arrays.update({"mask_%d" % b: g["mask"], "cls_%d" % b: g["cls"], "box_%d" % b: g["box"]})
        path = os.path.join(OUT, "spp_gt_%s.npz" % name)
        np.savez_compressed(path, **arrays)
        print("%-13s %s  B=%d  points=%5d  rows=%s  cols=%s  none=%s  %d bytes"
              % (name, mode, B, len(second), [0 if g is None else g["mask"].shape[0] for g in got],
                 [0 if g is None else g["mask"].shape[1] for g in got], [g is None for g in got],
                 os.path.getsize(path)))
        names.append(name)
    assert names == spp_gt_ref.FIXTURES
    print("wrote %d cases" % len(names))


if __name__ == "__main__":
    main()
