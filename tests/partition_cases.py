"""Inputs of the scene-partition edge tests (test_partition_edges_cpu.py / test_partition_edges_gpu.py) and what every
partition test shares: the launch helper, the comparison with the oracle, and the case tables.

A grid scene is uniform points in a 4 x 4 x 2 box whose superpoint id is the index of the point's grid cell, with
cell-aligned instance boxes: at cell 0.25 a superpoint has ~3 points of a 6000-point scene and a 1024-point run of a
shuffled scene touches several hundred superpoints (more than any LDS table of k_pool_lds has slots: the global-atomics
branch); at cell 0.5 a superpoint has ~25 points and a run of a coherent (sorted by id) scene touches ~45 (the
shuffle-reduced one_spp branch).  The floor box of a grid scene is one cell high (ground_h = cell), so that the LAST box
of every scene -- bit 63 of word 0 at 64 boxes, bit 0 of word 1 at 65 -- is occupied by the whole bottom layer of cells.

"Boxes" in a case table is the TOTAL count the kernels see, the floor box included; the pooling variant a case must take
(gapro_partition_pool_plan) is part of the case and asserted on both sides.
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
K_POOL_RUN = 1024  # points per workgroup of k_pool_lds


def grid_scene(seed, n, n_boxes, d, cell, order, id_scale=1, id_base=0):
    """Keyword inputs of one scene: n points uniform in 4 x 4 x 2, superpoint id = grid cell index * id_scale + id_base,
    order "coherent" (stable sort by id) or "shuffled", n_boxes cell-aligned float32 instance boxes of 2 .. 4 cells per
    edge, features 3 N(0, 1) float32[n, d]."""
    assert order in ("coherent", "shuffled")
    rng = np.random.default_rng(seed)
    ext = np.array([4.0, 4.0, 2.0])
    cells = np.round(ext / cell).astype(np.int64)
    coords = rng.uniform(0.0, 1.0, size=(n, 3)) * ext
    ijk = np.minimum((coords / cell).astype(np.int64), cells - 1)
    spp = ((ijk[:, 0] * cells[1] + ijk[:, 1]) * cells[2] + ijk[:, 2]) * int(id_scale) + int(id_base)
    feats = (3.0 * rng.standard_normal((n, d))).astype(np.float32)
    perm = np.argsort(spp, kind="stable") if order == "coherent" else rng.permutation(n)
    coords, spp, feats = coords[perm], spp[perm].astype(np.int64), feats[perm]
    size = rng.integers(2, 5, size=(n_boxes, 3))
    size = np.minimum(size, cells[None, :])
    lo = (rng.uniform(0.0, 1.0, size=(n_boxes, 3)) * (cells[None, :] - size + 1)).astype(np.int64)
    box = np.concatenate([lo * cell, (lo + size) * cell], 1).astype(np.float32)
    vol = np.prod(box[:, 3:] - box[:, :3], axis=1).astype(np.float32)
    return dict(coords_float=coords, mask_feats=feats, spp=spp, instance_cls=rng.integers(0, 18, size=n_boxes),
                instance_box=box, instance_box_volume=vol, wall_box=[], wall_box_volume=[], ground_h=float(cell))


def boxes_kw(coords, feats, spp, box, ground_h=0.1):
    """Keyword inputs from explicit arrays (instance boxes float32[B, 6])."""
    box = np.asarray(box, np.float32).reshape(-1, 6)
    return dict(coords_float=np.asarray(coords, np.float64), mask_feats=np.asarray(feats, np.float32),
                spp=np.asarray(spp, np.int64), instance_cls=np.arange(len(box)) % 18, instance_box=box,
                instance_box_volume=np.prod(box[:, 3:] - box[:, :3], axis=1).astype(np.float32), wall_box=[],
                wall_box_volume=[], ground_h=float(ground_h))


# ------------------------------------------------------------------------------------------ launch + comparison
def make_partition_job(kw, thresh):
    from gapro_amd.pipeline import make_job

    return make_job(kw["coords_float"], kw["mask_feats"], kw["spp"], kw["instance_cls"], kw["instance_box"],
                    kw["instance_box_volume"], kw["wall_box"], kw["wall_box_volume"], 18, kw.get("ground_h", 0.1), thresh)


def _run_partition(kw, thresh=0.999, spp_range_cap=None):
    import torch
    from gapro_amd.pipeline import Pipeline

    pipe = Pipeline(device=0, training_iter=0, spp_range_cap=spp_range_cap)
    job = make_partition_job(kw, thresh)
    pipe._prepare(job)  # launches gapro_partition_prepare_async, one sync, checks the header status
    feats_spp = torch.empty((job.n_spps, job.feats.shape[1]), dtype=torch.float32, device=pipe.device)
    pipe._pool(job, feats_spp)
    torch.cuda.synchronize()
    return pipe, job


def oracle_partition(kw, thresh=0.999):
    """(boxes f64[B, 6] with the floor box, classes, volumes, Partition) of the oracle."""
    from oracle import gen_ps_oracle as O

    boxes, cls, vol = O.assemble_boxes(kw["coords_float"], kw["instance_cls"], kw["instance_box"],
                                       kw["instance_box_volume"], kw["wall_box"], kw["wall_box_volume"],
                                       ground_h=kw.get("ground_h", 0.1))
    return boxes, cls, vol, O.partition(kw["coords_float"], kw["mask_feats"], kw["spp"], boxes, cls, vol, thresh)


def unpack_bits(bits, n_boxes):
    """bool[S, B] of the occupancy words u64[S, W]."""
    bits = np.asarray(bits).view(np.uint64)
    got = np.zeros((bits.shape[0], n_boxes), dtype=bool)
    for b in range(n_boxes):
        got[:, b] = (bits[:, b // 64] >> np.uint64(b % 64)) & np.uint64(1)
    return got


def _check_against_oracle(kw, job, thresh=0.999, part=None):
    from oracle import gen_ps_oracle as O

    boxes, cls, vol, part = oracle_partition(kw, thresh) if part is None else part
    h = job.header
    coords = np.asarray(kw["coords_float"], dtype=np.float64)
    np.testing.assert_array_equal(np.array(list(h.coord_min)), coords.min(0))
    np.testing.assert_array_equal(np.array(list(h.coord_max)), coords.max(0))
    assert (h.spp_min, h.spp_max) == (int(np.min(kw["spp"])), int(np.max(kw["spp"])))
    assert job.n_spps == part.n_spps
    np.testing.assert_array_equal(job.boxes, boxes)  # incl. the float64 floor box
    np.testing.assert_array_equal(job.boxes_cls, cls)
    np.testing.assert_array_equal(job.boxes_volume, vol)
    np.testing.assert_array_equal(job.spp_inv.cpu().numpy(), part.spp_inv)
    np.testing.assert_array_equal(job.dev["occ_count"].cpu().numpy(), part.occ_count)
    np.testing.assert_array_equal(job.dev["point_count"].cpu().numpy(), part.point_count)
    np.testing.assert_array_equal(job.dev["n_bbs"].cpu().numpy(), part.n_bbs_per_spp)
    bits = job.dev["occ_bits"].cpu().numpy().view(np.uint64)
    assert bits.shape == (part.n_spps, (len(boxes) + 63) // 64)
    np.testing.assert_array_equal(unpack_bits(bits, len(boxes)), part.occ_spp)
    assert int(h.fixed_shift) == O.fixed_point_shift(float(np.max(np.abs(np.asarray(kw["mask_feats"], np.float32)))),
                                                    len(coords))
    np.testing.assert_array_equal(job.dev["feats_spp"].cpu().numpy(), part.feats_spp)  # bit-exact
    return part


# ------------------------------------------------------------------------------------------ the variant sweep
SWEEP_THRESH = 0.8
SWEEP_N = 6000

SweepCase = namedtuple("SweepCase", "name d boxes order plan cell seed")


def _sweep():
    # total boxes on both sides of every tier of gapro_partition_pool_plan (60 KiB: 48 B of corners per box, a slot of
    # 8 + 4 boxes + 8 D bytes) and of the 64-bit occupancy word
    tiers = ((6, ((63, 6), (64, 6), (65, 6), (128, 6), (129, 6), (190, 6), (191, 5), (338, 5), (339, 4), (540, 4),
                  (541, 0))),
             (32, ((146, 6), (147, 5), (510, 4), (511, 0))))
    out = []
    for d, rows in tiers:
        for boxes, plan in rows:
            for order in ("coherent", "shuffled"):
                out.append(SweepCase("d%d_b%d_%s" % (d, boxes, order), d, boxes, order, plan,
                                     0.5 if order == "coherent" else 0.25, 1000 * d + boxes))
    return tuple(out)


SWEEP = _sweep()
SWEEP_IDS = [c.name for c in SWEEP]
LIMIT_BOXES = 1365  # the most boxes whose corners fit 64 KiB of LDS; one more is GAPRO_ERR_BAD_ARG


@lru_cache(maxsize=None)
def sweep_scene(case):
    return grid_scene(case.seed, SWEEP_N, case.boxes - 1, case.d, case.cell, case.order)


# ------------------------------------------------------------------------------------------ widths and run tails
# (D, n, cell), D and n paired.  At cell 0.5 a superpoint has at most ~8 points of these scenes: the per-point branch of
# k_pool_lds; the largest sizes again at cell 1.0 (32 superpoints of >= 30 points): the shuffle-reduced branch.
WIDTH_TAILS = ((1, 1, 0.5), (3, 7, 0.5), (7, 8, 0.5), (8, 9, 0.5), (9, 1023, 0.5), (33, 1024, 0.5), (7, 1025, 0.5),
               (33, 2049, 0.5), (1, 1023, 1.0), (3, 1024, 1.0), (9, 1025, 1.0), (8, 2049, 1.0))


def width_tail_scene(d, n, cell):
    return grid_scene(77 * d + n, n, 5, d, cell, "coherent")


# ------------------------------------------------------------------------------------------ the fraction ladder
LADDER_THRESHOLDS = (0.5, 0.6, 0.7, 0.8, 0.999, 1.0 / 3.0, 1.0)


def ladder_pairs():
    """(n, k): a superpoint of n points, k of them inside the one instance box."""
    pairs = [(n, k) for n in range(1, 41) for k in range(n + 1)]
    return pairs + [(1000, 999), (1000, 998), (3, 1), (3, 2)]


@lru_cache(maxsize=None)
def ladder_scene():
    """One instance box [0, 1]^2 x [1, 2]; superpoint j has ladder_pairs()[j][1] points well inside it and the others
    two units away.  Points are shuffled.  (The floor box, the bottom 0.1 of the scene, is a second, random ladder.)"""
    rng = np.random.default_rng(5)
    pairs = ladder_pairs()
    coords, spp = [], []
    for j, (n, k) in enumerate(pairs):
        inside = rng.uniform([0.1, 0.1, 1.0], [0.9, 0.9, 1.9], size=(k, 3))
        outside = rng.uniform([2.5, 0.1, 1.0], [3.5, 0.9, 1.9], size=(n - k, 3))
        coords += [inside, outside]
        spp += [np.full(n, j)]
    coords, spp = np.concatenate(coords), np.concatenate(spp)
    perm = rng.permutation(len(spp))
    feats = rng.standard_normal((len(spp), 6))
    return boxes_kw(coords[perm], feats, spp[perm], [[0, 0, 1, 1, 1, 2]])


# ------------------------------------------------------------------------------------------ faces
FACE_BOX_INDICES = (0, 63, 64, 65)
FACE_N_BOXES = 66  # instance boxes; the floor box is the 67th
# (box, mode): every point its own superpoint (the per-point branch of k_pool_lds) for each box; then the other three
# copies of the interval test: "waves" = every point eight times in a row under one id (the shuffle-reduced branch),
# "crowded" = behind 600 single-point superpoints that fill the table (the global-atomics branch), "k_pool" = 600 boxes
FACE_CASES = tuple((b, "own") for b in FACE_BOX_INDICES) + ((64, "waves"), (64, "crowded"), (63, "k_pool"))


def face_scene(b, mode="own"):
    """18 probe points around instance box b of 66 (corners that are not exact in float32; every other box 100 units
    away): for each of the six faces the point exactly on the widened face float64(float32 corner) -+ 0.005 and its two
    float64 neighbours, the other two coordinates at the box centre.  Returns (kw, expected membership bool[18], the
    superpoint rank of every probe point, points per probe)."""
    assert mode in ("own", "waves", "crowded", "k_pool")
    rng = np.random.default_rng(b)
    n_boxes = 600 if mode == "k_pool" else FACE_N_BOXES
    box = np.zeros((n_boxes, 6), np.float32)
    far = 100.0 + 3.0 * np.arange(n_boxes)
    box[:, 0], box[:, 3] = far, far + 1.0
    box[:, 1:3], box[:, 4:6] = 0.3, 1.3
    box[b] = np.array([1.1, 2.3, 0.7, 2.2, 3.1, 1.9], np.float32) + rng.uniform(0, 0.01, 6).astype(np.float32)
    c = box[b].astype(np.float64)
    centre = 0.5 * (c[:3] + c[3:])
    pts, want = [], []
    for axis in range(3):
        for side in (0, 1):
            face = c[axis] - 0.005 if side == 0 else c[3 + axis] + 0.005  # float64 arithmetic, as the reference does
            inward = np.inf if side == 0 else -np.inf
            for v, inside in ((face, True), (np.nextafter(face, inward), True), (np.nextafter(face, -inward), False)):
                p = centre.copy()
                p[axis] = v
                pts.append(p)
                want.append(inside)
    pts, rep = np.array(pts), 1
    spp = np.arange(len(pts))
    if mode == "waves":
        rep = 8
        pts, spp = np.repeat(pts, 8, axis=0), np.repeat(spp, 8)
    elif mode == "crowded":  # 600 superpoints of one point each, between the boxes, in front of the probe points
        filler = rng.uniform([20, 0, 0.7], [60, 1, 1.9], size=(600, 3))
        pts, spp = np.concatenate([filler, pts]), np.concatenate([1000 + np.arange(600), spp])
    feats = rng.standard_normal((len(pts), 6))
    return boxes_kw(pts, feats, spp, box), np.array(want), np.arange(18), rep
