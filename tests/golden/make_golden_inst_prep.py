#!/usr/bin/env python3
"""Generate tests/golden/inst_prep_*.npz by running the REFERENCE's instance-label preparation in this container.

Run from the repo root:  python tests/golden/make_golden_inst_prep.py
Needs /root/reference (read-only).  What is executed from the reference, on CPU tensors:

* ``get_cropped_instance_label`` -- imported as-is from ISBNet/isbnet/model/model_utils.py:589-597 and from
  gapro/gen_ps_utils.py:64-72 (the same function twice; both are run and must agree), on int64, int32 and float64
  labels, in place and through ``valid_idxs``;
* ``get_instance_info`` -- imported as-is from ISBNet/isbnet/model/model_utils.py:519-555, on the cropped labels, as
  isbnet.py:254-270 calls the two.

``torch_scatter``, ``isbnet.ops`` and ``gaussian_process_utils`` (imported by those modules, never called by these
functions) are empty stubs IN THIS HARNESS ONLY, as in make_golden_consumer.py.  The fixtures hold inputs and the values
the functions returned; the point counts (which get_instance_info computes and drops) are a bincount of the cropped
labels.  Nothing of the reference's text is written.

The script also measures the one deliberate deviation: the largest |centroid offset of the reference's
float32 mean - centroid offset of the exact rule (tests/inst_prep_ref.py)| over the cases, stored in
inst_prep_summary.npz; the GPU test allows 4 x that value.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import inst_prep_ref  # noqa: E402


def install_stubs():
    sys.modules["torch_scatter"] = types.ModuleType("torch_scatter")
    pkg = types.ModuleType("isbnet")
    pkg.__path__ = [os.path.join(REF, "ISBNet", "isbnet")]
    ops = types.ModuleType("isbnet.ops")
    ops.ballquery_batchflat = None
    model = types.ModuleType("isbnet.model")
    model.__path__ = [os.path.join(REF, "ISBNet", "isbnet", "model")]
    gpu = types.ModuleType("gaussian_process_utils")
    gpu.fit_gp_spp = None
    sys.modules.update({"isbnet": pkg, "isbnet.ops": ops, "isbnet.model": model, "gaussian_process_utils": gpu})
    sys.path.insert(0, os.path.join(REF, "gapro"))


# name, points, ids handed out, share of the ids left empty, share of unlabelled points, coordinates, label_shift
CASES = [
    ("one", 200, 1, 0.0, 0.3, "grid", 0),         # a single instance, carried by id 5
    ("floats", 1000, 7, 0.3, 0.2, "uniform", 2),  # full-entropy float32 coordinates
    ("mid", 5000, 40, 0.25, 0.1, "blobs", 0),     # consecutive holes
    ("nohole", 3000, 25, 0.0, 0.0, "blobs", 2),   # nothing to move, every point labelled
    ("blobs", 12000, 60, 0.1, 0.15, "blobs_f32", 2),  # blobs off the grid: a few hundred float32 terms per mean
    ("many", 20000, 300, 0.1, 0.1, "blobs", 0),
]


def make_case(name, n, n_ids, p_empty, p_unlabelled, kind, seed):
    rng = np.random.default_rng(seed)
    ids = np.arange(n_ids)
    empty = rng.random(n_ids) < p_empty
    if name == "mid":
        empty[3:7] = True   # consecutive holes
        empty[0] = True     # a hole at 0
    if name == "one":
        ids = np.array([5])
        empty = np.array([False])
    if n_ids > 1:
        empty[-1] = False   # the largest id is in use
    used = ids[~empty]
    inst = used[rng.integers(0, len(used), n)]
    inst[rng.permutation(n)[:len(used)]] = used  # every used id owns a point
    centres = rng.uniform(-12, 12, (int(ids.max()) + 1, 3))
    if kind == "uniform":
        xyz = rng.uniform(-16, 16, (n, 3)).astype(np.float32)
    elif kind == "grid":
        xyz = (rng.integers(-800, 800, (n, 3)) / 50.0).astype(np.float32)
    else:  # voxel-like: blobs around the instance centres on a 1/512 grid
        xyz = centres[inst] + rng.normal(0, 0.7, (n, 3))
        xyz = np.clip(xyz, -16, 16)
        xyz = (xyz if kind == "blobs_f32" else np.rint(xyz * 512) / 512).astype(np.float32)
    sem_of = rng.integers(2, 20, int(ids.max()) + 1)
    sem = sem_of[inst].astype(np.int64)
    sem[rng.random(n) < 0.05] = -100            # ignored points inside instances, some of them first points
    noise = rng.random(n) < 0.05
    sem[noise] = rng.integers(2, 20, int(noise.sum()))
    inst = inst.astype(np.int64)
    off = rng.random(n) < p_unlabelled
    inst[off] = -100
    for u in used:                               # ... but no used id loses its last point
        if not np.any(inst == u):
            inst[np.nonzero(off)[0][0]] = u
            off[np.nonzero(off)[0][0]] = False
    valid = np.sort(rng.permutation(n)[: max(1, (2 * n) // 3)])
    return xyz, inst, sem, valid


def main():
    install_stubs()
    mu = importlib.import_module("isbnet.model.model_utils")
    gu = importlib.import_module("gen_ps_utils")
    worst = 0.0
    names = []
    for k, (name, n, n_ids, p_empty, p_off, kind, shift) in enumerate(CASES):
        xyz, inst, sem, valid = make_case(name, n, n_ids, p_empty, p_off, kind, 7000 + k)
        cropped = mu.get_cropped_instance_label(torch.from_numpy(inst.copy())).numpy()
        for fn in (mu.get_cropped_instance_label, gu.get_cropped_instance_label):
            for dt in (torch.int64, torch.int32, torch.float64):
                t = torch.from_numpy(inst.copy()).to(dt)
                got = fn(t)
                assert got is t and np.array_equal(got.numpy().astype(np.int64), cropped), (name, dt)
        cropped_valid = mu.get_cropped_instance_label(torch.from_numpy(inst.copy()), torch.from_numpy(valid)).numpy()
        assert np.array_equal(cropped_valid, gu.get_cropped_instance_label(torch.from_numpy(inst.copy()),
                                                                           torch.from_numpy(valid)).numpy())
        cls, box, cen, cor = mu.get_instance_info(torch.from_numpy(xyz), torch.from_numpy(cropped),
                                                  torch.from_numpy(sem), label_shift=shift)
        cls, box, cen, cor = cls.numpy(), box.numpy(), cen.numpy(), cor.numpy()
        pointnum = np.bincount(cropped[cropped >= 0], minlength=len(cls)).astype(np.int32)
        # the restatement on the same inputs: equal everywhere but the centroid, whose distance is measured
        w = inst_prep_ref.prepare_instance_labels(xyz, inst, sem, shift)
        assert np.array_equal(w[0], cropped) and np.array_equal(w[1], cls) and np.array_equal(w[2], box)
        assert np.array_equal(w[3], pointnum) and np.array_equal(w[5], cor)
        assert np.array_equal(w[4] == -100.0, cen == -100.0)
        diff = float(np.max(np.abs(w[4].astype(np.float64) - cen.astype(np.float64))))
        worst = max(worst, diff)
        print("%-7s V=%5d I=%3d  holes moved=%3d  max |centroid offset diff| = %.3g"
              % (name, n, len(cls), int(np.sum(np.unique(inst[inst >= 0]) >= len(cls))), diff))
        np.savez_compressed(os.path.join(OUT, "inst_prep_%s.npz" % name), coords=xyz, inst=inst, sem=sem, valid=valid,
                            label_shift=np.int64(shift), cropped=cropped, cropped_valid=cropped_valid, cls=cls, box=box,
                            pointnum=pointnum, centroid_offset=cen, corners_offset=cor)
        names.append(name)
    np.savez_compressed(os.path.join(OUT, "inst_prep_summary.npz"), names=np.array(names),
                        centroid_max_abs_diff=np.float64(worst))
    print("wrote %d cases; centroid_max_abs_diff = %.6g" % (len(names), worst))


if __name__ == "__main__":
    main()
