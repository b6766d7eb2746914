"""A plain NumPy restatement of the training-set assembly of the point-level fits (gapro_amd.gp_train_sets /
fit_gp_batch), for the fit_gp tests: what the device assembly must return, bit for bit.

Written from the stated semantics, not from the kernels: exact int64 sums of fixed-point terms, one float64 division,
distances as (dx dx + dy dy) + dz dz in float64 with every operation rounded on its own (NumPy never fuses them), and
ties ordered by position in the side's list."""
import os

import numpy as np

from oracle.gen_ps_oracle import fixed_point_shift

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NOT_FINITE = -4


def exact_sum(x, k):
    """sum over axis 0 of rint(x * 2**k) in int64"""
    return np.rint(np.ldexp(np.asarray(x, dtype=np.float64), k)).astype(np.int64).sum(axis=0)


def pool_side(feats, spp, inds):
    """(rows f32[U, D], ids i64[U]) of one side: its distinct superpoint ids ascending, each row the exact mean of the
    side's points of that id, duplicates counted as often as they occur."""
    feats = np.asarray(feats, dtype=np.float32)
    n = len(feats)
    k = fixed_point_shift(float(np.max(np.abs(feats))), n)
    inds = np.asarray(inds, dtype=np.int64).reshape(-1)
    ids, inv = np.unique(np.asarray(spp, dtype=np.int64)[inds], return_inverse=True)
    q = np.rint(np.ldexp(feats[inds].astype(np.float64), k)).astype(np.int64)
    sums = np.zeros((len(ids), feats.shape[1]), dtype=np.int64)
    np.add.at(sums, inv.reshape(-1), q)
    cnt = np.bincount(inv.reshape(-1), minlength=len(ids)).astype(np.float64)
    return (np.ldexp(sums.astype(np.float64), -k) / cnt[:, None]).astype(np.float32), ids


def centroid(coords, inter):
    """Exact, order-independent centroid of the intersection's points (float64[3]).  The fixed-point scale comes from
    the largest |coordinate| among the FINITE coordinates of the whole input, so a non-finite coordinate elsewhere does
    not move it (a non-finite term of the intersection itself adds nothing: that problem is NOT_FINITE anyway)."""
    coords = np.asarray(coords, dtype=np.float64)
    finite = np.abs(coords[np.isfinite(coords)])
    kc = fixed_point_shift(float(finite.max()) if finite.size else 0.0, len(coords))
    pts = coords[np.asarray(inter, dtype=np.int64).reshape(-1)]
    pts = np.where(np.isfinite(pts).all(axis=1, keepdims=True), pts, 0.0)
    return np.ldexp(exact_sum(pts, kc).astype(np.float64), -kc) / float(len(pts))


def distances(coords, inds, c):
    """(dx dx + dy dy) + dz dz of the listed points to c, every operation rounded to float64 on its own."""
    d = np.asarray(coords, dtype=np.float64)[np.asarray(inds, dtype=np.int64).reshape(-1)] - c[None, :]
    xx, yy, zz = d[:, 0] * d[:, 0], d[:, 1] * d[:, 1], d[:, 2] * d[:, 2]
    return (xx + yy) + zz


def nearest_side(coords, inds, c, k):
    """The side's chosen point indices in order: all of them as given when there are at most k, else the k smallest
    distances to c ordered by (distance, position in the list)."""
    inds = np.asarray(inds, dtype=np.int64).reshape(-1)
    if len(inds) <= k:
        return inds.copy()
    dist = distances(coords, inds, c)
    order = np.lexsort((np.arange(len(inds)), dist))  # by distance, ties by position
    return inds[order[:k]]


def train_set(coords, feats, spp, problem, npoint_nearest=800, spp_pool=True):
    """(train_x f32[M, D], m1, m2, sel1, sel2, status) of one problem, as gp_train_sets returns it."""
    b1, b2, inter = (np.asarray(x, dtype=np.int64).reshape(-1) for x in problem)
    feats = np.asarray(feats, dtype=np.float32)
    if spp_pool:
        r1, s1 = pool_side(feats, spp, b1)
        r2, s2 = pool_side(feats, spp, b2)
        return np.concatenate([r1, r2]), len(s1), len(s2), s1, s2, 0
    coords = np.asarray(coords, dtype=np.float64)
    need_c = max(len(b1), len(b2)) > npoint_nearest
    c = centroid(coords, inter) if need_c else np.zeros(3)
    s1, s2 = nearest_side(coords, b1, c, npoint_nearest), nearest_side(coords, b2, c, npoint_nearest)
    rows = np.concatenate([feats[s1], feats[s2]])
    used = np.concatenate([b1, b2, inter])
    ok = np.isfinite(coords[used]).all() and np.isfinite(rows).all()
    return rows, len(s1), len(s2), s1, s2, 0 if ok else NOT_FINITE


def golden_scene(name):
    """(coords f64[N,3], feats f32[N,6], spp i64[N], spp_inv, point-level problems) of a golden scene: every recorded
    fit's superpoint index sets turned into the sets of the points of those superpoints."""
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"), allow_pickle=False)
    feats = np.concatenate([z["xyz_raw"], z["rgb"]], axis=-1).astype(np.float32)
    spp = z["spp"].astype(np.int64)
    _, inv = np.unique(spp, return_inverse=True)
    inv = inv.reshape(-1)
    problems = []
    for i in range(int(z["n_fits"])):
        problems.append(tuple(np.nonzero(np.isin(inv, z["fit%03d_%s" % (i, k)]))[0].astype(np.int64)
                              for k in ("b1_inds", "b2_inds", "intersect_inds")))
    return z["xyz_aligned"].astype(np.float64), feats, spp, inv, problems
