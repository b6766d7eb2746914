"""NumPy restatement of the per-sample ground-truth masks (gapro_amd/csrc/spp_gt.hip): the RULE, not the
reference's loops -- the spec the device results are held to exactly -- and the loader of the fixtures
tests/golden/make_golden_spp_gt.py wrote.

Sample b holds the points [offsets[b], offsets[b + 1]).  Columns: its distinct superpoint ids, ascending.  Rows: its
distinct labels, ascending, that differ from ignore_label and whose class is >= 0.  c(i, s) = points of s labelled i,
n(s) = all points of s: mask = 1 iff 2 c >= n (strict: 2 c > n).  Without superpoints every point is its own column.
"""
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BAD_ARG, SPP_RANGE = -1, -6
FLAG_OFFSETS, FLAG_GATHER, FLAG_LABEL, FLAG_SPP = 1, 2, 4, 8
FIXTURES = ["two", "four", "second_empty", "shared_spp", "half_splits", "subsample"]  # make_golden_spp_gt.py CASES


class Refused(Exception):
    """What the device reports instead of a result: the status, the winning cause's flag and its lowest sample."""

    def __init__(self, code, flag, sample):
        super().__init__("refused: status %d, flag %d, sample %d" % (code, flag, sample))
        self.code, self.flag, self.sample = code, flag, sample


def rule(c, n, strict=False):
    """The integer rule on counts (any integer arrays that broadcast)."""
    c2 = 2 * np.asarray(c, dtype=np.int64)
    n = np.asarray(n, dtype=np.int64)
    return c2 > n if strict else c2 >= n


def _refusals(labels, gather, spps, n_cls, n_spps, off, ignore):
    """Raises the winning refusal, in the order offsets, gather index, label, superpoint id."""
    B = len(off) - 1
    n = len(gather) if gather is not None else len(labels)
    for b in range(B + 1):
        if off[b] < 0 or off[b] > n or (b < B and off[b + 1] < off[b]):
            raise Refused(BAD_ARG, FLAG_OFFSETS, min(b, B - 1))
    bad = {FLAG_GATHER: None, FLAG_LABEL: None, FLAG_SPP: None}

    def note(flag, b):
        if bad[flag] is None:
            bad[flag] = b

    for b in range(B):
        p = np.arange(off[b], off[b + 1])
        src = gather[p] if gather is not None else p
        ok = (src >= 0) & (src < len(labels))
        if not ok.all():
            note(FLAG_GATHER, b)
        src = src[ok]
        lab = labels[src]
        is_ignore = lab == ignore
        with np.errstate(invalid="ignore"):
            good = (lab >= 0) & (lab < n_cls) & (lab == np.floor(lab))
        if not (good | is_ignore).all():
            note(FLAG_LABEL, b)
        if spps is not None and not ((spps[src] >= 0) & (spps[src] < n_spps)).all():
            note(FLAG_SPP, b)
    for flag in (FLAG_GATHER, FLAG_LABEL, FLAG_SPP):
        if bad[flag] is not None:
            raise Refused(SPP_RANGE if flag == FLAG_SPP else BAD_ARG, flag, bad[flag])


def _rows(lab, cls, ignore):
    ids = np.unique(lab[lab != ignore]).astype(np.int64)
    return ids[cls[ids] >= 0]


def _entry(mask, ids, cls, box):
    return {"mask": mask.astype(np.float32), "cls": cls[ids], "box": box[ids], "ids": ids}


def get_spp_gt(labels, spps, cls, box, offsets, batch_size, ignore=-100, strict=False, n_spps=None):
    labels, spps, off = np.asarray(labels), np.asarray(spps), np.asarray(offsets, dtype=np.int64)
    assert len(off) == batch_size + 1
    n_spps = int(spps.max()) + 1 if n_spps is None else n_spps
    _refusals(labels, None, spps, len(cls), n_spps, off, ignore)
    out = []
    for b in range(batch_size):
        lab, spp = labels[off[b]:off[b + 1]], spps[off[b]:off[b + 1]]
        ids = _rows(lab, cls, ignore)
        if len(ids) == 0:
            out.append(None)
            continue
        cols, inv = np.unique(spp, return_inverse=True)
        n = np.bincount(inv, minlength=len(cols))
        c = np.zeros((len(ids), len(cols)), dtype=np.int64)
        row = np.searchsorted(ids, lab.astype(np.int64))
        row = np.minimum(row, len(ids) - 1)
        kept = (lab != ignore) & (ids[row] == lab)
        np.add.at(c, (row[kept], inv[kept]), 1)
        out.append(_entry(rule(c, n[None, :], strict), ids, cls, box))
    return out


def get_subsample_gt(labels, idxs, cls, box, offsets, batch_size, ignore=-100):
    labels, idxs, off = np.asarray(labels), np.asarray(idxs).astype(np.int64), np.asarray(offsets, dtype=np.int64)
    assert len(off) == batch_size + 1
    _refusals(labels, idxs, None, len(cls), 0, off, ignore)
    out = []
    for b in range(batch_size):
        lab = labels[idxs[off[b]:off[b + 1]]]
        ids = _rows(lab, cls, ignore)
        if len(ids) == 0:
            out.append(None)
            continue
        out.append(_entry(lab[None, :] == ids[:, None], ids, cls, box))
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same(got, want):
    """Two results (lists of None / dicts of arrays) are equal to the bit, in values, dtypes and shapes; ``ids`` is
    compared where both carry it."""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g is None) == (w is None), (g is None, w is None)
        if g is None:
            continue
        for k in ("mask", "cls", "box") + (("ids",) if "ids" in g and "ids" in w else ()):
            a, b = np.asarray(g[k]), np.asarray(w[k])
            assert a.dtype == b.dtype and a.shape == b.shape, (k, a.dtype, b.dtype, a.shape, b.shape)
            assert np.array_equal(bits(a), bits(b)), k
    return True


def fixture(name):
    """The stored case: its inputs and what the reference's function returned, as a list like the functions'."""
    z = np.load(os.path.join(GOLDEN_DIR, "spp_gt_%s.npz" % name), allow_pickle=False)
    want = []
    for b in range(int(z["batch_size"])):
        if bool(z["is_none"][b]):
            want.append(None)
        else:
            want.append({"mask": z["mask_%d" % b], "cls": z["cls_%d" % b], "box": z["box_%d" % b]})
    return z, want
