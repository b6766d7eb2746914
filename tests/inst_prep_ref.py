"""NumPy restatement of the instance-label preparation (gapro_amd/csrc/inst_prep.hip), the spec the
device results are held to bit for bit, and the loader of the fixtures tests/golden/make_golden_inst_prep.py wrote.

crop      P = distinct ids >= 0, K = |P|; ids of P below K stay, the holes of [0, K) ascending take the ids of P that are
          >= K descending; negative labels stay.
info      per id r in [0, max id + 1): class of the first point (minus label_shift unless -100), box = [min | max] in
          the total order of the float32 keys (-0.0 below +0.0), point count, centroid = exact int64 sum of
          rint(x 2^k), k = fixed_point_shift(largest |coordinate| of the labelled points, V), ldexp(sum, -k) / count in
          float64 rounded once to float32; offsets = one float32 subtraction per component; -100 rows elsewhere.
"""
import os

import numpy as np

from oracle.gen_ps_oracle import fixed_point_shift

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAX_IDS = 1 << 20


class Refused(Exception):
    """What the device reports as a status: .code is the GAPRO_ERR_* value."""

    def __init__(self, code, why):
        super().__init__(why)
        self.code = code


BAD_ARG, NOT_FINITE = -1, -4


def _ids(labels):
    """int64 ids, -1 where the label names no instance (negative or NaN)."""
    labels = np.asarray(labels)
    if labels.dtype.kind == "f":
        named = labels >= 0  # NaN compares false
        if np.any(named & (labels != np.floor(labels))):
            raise Refused(BAD_ARG, "a float label that is no integer")
        ids = np.where(named, np.where(named, labels, 0), -1).astype(np.int64)
    else:
        ids = np.where(labels >= 0, labels, -1).astype(np.int64)
    if ids.size and ids.max() >= MAX_IDS:
        raise Refused(BAD_ARG, "an id at or beyond the bound")
    return ids


def crop_map(present_ids):
    """old id -> new id for the sorted distinct ids >= 0 (the closed form)."""
    p = np.asarray(present_ids, dtype=np.int64)
    K = len(p)
    holes = np.setdiff1d(np.arange(K, dtype=np.int64), p)  # ascending
    high = p[p >= K][::-1]                                 # descending
    assert len(holes) == len(high)
    m = {int(i): int(i) for i in p[p < K]}
    m.update({int(h): int(o) for h, o in zip(high, holes)})
    return m


def get_cropped_instance_label(labels, valid_idxs=None):
    """A cropped COPY in the labels' dtype (the device function works in place)."""
    labels = np.asarray(labels)
    if valid_idxs is not None:
        labels = labels[valid_idxs]
    ids = _ids(labels)
    out = labels.copy()
    present = np.unique(ids[ids >= 0])
    if len(present) == 0:
        return out
    lut = np.full(int(present.max()) + 1, -1, dtype=np.int64)
    for old, new in crop_map(present).items():
        lut[old] = new
    on = ids >= 0
    out[on] = lut[ids[on]].astype(labels.dtype)
    return out


def crop_loop(labels):
    """The hole-filling rule itself, transcribed on a NumPy copy: while j is below the largest id, an empty j takes
    every point of the largest id."""
    lab = np.array(labels).copy()
    j = 0
    while lab.size and j < lab.max():
        if not np.any(lab == j):
            lab[lab == lab.max()] = j
        j += 1
    return lab


def _keys(x):
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def _unkeys(k):
    k = np.asarray(k, dtype=np.uint32)
    return np.where(k >> 31 != 0, k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def get_instance_info(coords, labels, sem, label_shift=0, with_pointnum=False):
    coords = np.ascontiguousarray(coords, dtype=np.float32)
    sem = np.asarray(sem)
    V = coords.shape[0]
    ids = _ids(labels)
    on = np.nonzero(ids >= 0)[0]
    if not np.all(np.isfinite(coords[on])):
        raise Refused(NOT_FINITE, "a non-finite coordinate on a labelled point")
    if len(on) == 0:
        raise Refused(BAD_ARG, "no id >= 0")
    num = int(ids.max()) + 1
    if len(np.unique(ids[on])) != num:
        raise Refused(BAD_ARG, "an empty id below the largest")
    order = on[np.argsort(ids[on], kind="stable")]  # by id, then by point index
    starts = np.nonzero(np.r_[True, ids[order][1:] != ids[order][:-1]])[0]
    count = np.diff(np.r_[starts, len(order)])
    first = order[starts]
    cls = sem[first].astype(np.int64)
    cls[cls != -100] -= int(label_shift)
    keys = _keys(coords[order])
    lo = _unkeys(np.minimum.reduceat(keys, starts, axis=0))
    hi = _unkeys(np.maximum.reduceat(keys, starts, axis=0))
    box = np.concatenate([lo, hi], axis=1)
    k = fixed_point_shift(float(np.abs(coords[on]).max()), V)
    q = np.rint(np.ldexp(coords[order].astype(np.float64), k)).astype(np.int64)
    sums = np.add.reduceat(q, starts, axis=0)
    centroid = (np.ldexp(sums.astype(np.float64), -k) / count[:, None].astype(np.float64)).astype(np.float32)
    cen_off = np.full((V, 3), -100.0, dtype=np.float32)
    cor_off = np.full((V, 6), -100.0, dtype=np.float32)
    cen_off[on] = centroid[ids[on]] - coords[on]
    cor_off[on, :3] = lo[ids[on]] - coords[on]
    cor_off[on, 3:] = hi[ids[on]] - coords[on]
    if with_pointnum:
        return cls, box, count.astype(np.int32), cen_off, cor_off
    return cls, box, cen_off, cor_off


def prepare_instance_labels(coords, labels, sem, label_shift=0):
    """(labels, cls, box, pointnum, centroid offsets, corner offsets)."""
    ids = _ids(labels)
    on = ids >= 0
    if np.any(on) and not np.all(np.isfinite(np.asarray(coords)[on])):
        raise Refused(NOT_FINITE, "a non-finite coordinate on a labelled point")
    new = get_cropped_instance_label(labels)
    return (new,) + get_instance_info(coords, new, sem, label_shift, with_pointnum=True)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


# ---- fixtures --------------------------------------------------------------------------------------------------------
def summary():
    return np.load(os.path.join(GOLDEN_DIR, "inst_prep_summary.npz"), allow_pickle=False)


FIXTURES = ["one", "floats", "mid", "nohole", "blobs", "many"]  # tests/golden/make_golden_inst_prep.py CASES


def fixture(name):
    return np.load(os.path.join(GOLDEN_DIR, "inst_prep_%s.npz" % name), allow_pickle=False)


def centroid_tolerance():
    """4 x the largest |centroid offset of the reference - that of the exact rule| the generator measured."""
    return 4.0 * float(summary()["centroid_max_abs_diff"])
