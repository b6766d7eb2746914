"""NumPy restatement of SPFormer's predicted-instance chain (include/gapro_hip.h, "SPFormer's predicted instances";
DESIGN.md 4.12).  No device.  Floating-point terms are float64 from the float32 inputs, rounded to float32 once;
everything else is integer or a bit copy.

The keyword switches at the end of ``predict_ref`` select the *wrong* conventions the edge cases are built to tell apart
(tests/test_spf_predict_cpu.py); the definition is all of them off.
"""
import os

import numpy as np

OK, ERR_BAD_ARG, ERR_NOT_FINITE, ERR_SPP_RANGE, ERR_WORKSPACE = 0, -1, -4, -6, -7
FLAG_SCORE, FLAG_MASK, FLAG_COORDS, FLAG_SPP = 1, 2, 4, 8


def status_of(flags):
    if flags & (FLAG_SCORE | FLAG_MASK | FLAG_COORDS):
        return ERR_NOT_FINITE
    return ERR_SPP_RANGE if flags & FLAG_SPP else OK


def class_scores64(labels, pred_scores, renorm=False):
    """Step 1 before its rounding: f64[Q, C]."""
    x = np.asarray(labels, np.float32).astype(np.float64)
    if renorm:  # wrong: the softmax over the C kept columns
        x = x[:, :-1]
    e = np.exp(x - x.max(axis=1, keepdims=True))
    den = np.zeros(x.shape[0])
    for c in range(x.shape[1]):  # the sum in ascending c
        den = den + e[:, c]
    e = e if renorm else e[:, :-1]
    return e / den[:, None] * np.asarray(pred_scores, np.float32).astype(np.float64).reshape(-1, 1)


def order_ref(values, k):
    """The k largest float32 values, descending; equal values by ascending index."""
    v = np.asarray(values, np.float32) + np.float32(0)  # -0.0 is +0.0
    return np.lexsort((np.arange(v.shape[0]), -v.astype(np.float64)))[:k]


def order_image(x):
    """float32 -> uint32 of the same order, -0.0 below +0.0."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def order_image_inv(u):
    u = np.asarray(u, np.uint32)
    return np.where(u & np.uint32(0x80000000), u & np.uint32(0x7fffffff), ~u).astype(np.uint32).view(np.float32)


def tables_ref(superpoints, coords_float, S):
    """Step 3: n i64[S], lo / hi as order images u32[S, 3] (all ones / zero for a superpoint without points)."""
    spp = np.asarray(superpoints, np.int64)
    img = order_image(np.asarray(coords_float, np.float32).reshape(-1, 3))
    n = np.bincount(spp, minlength=S).astype(np.int64)
    lo, hi = np.full((S, 3), 0xffffffff, np.uint32), np.zeros((S, 3), np.uint32)
    np.minimum.at(lo, spp, img)
    np.maximum.at(hi, spp, img)
    return n, lo, hi


def rle_ref(mask):
    """Step 6: the counts of one row, int64."""
    m = np.concatenate([[0], np.asarray(mask).astype(np.int8), [0]])
    runs = np.nonzero(m[1:] != m[:-1])[0].astype(np.int64) + 1
    runs[1::2] -= runs[::2]
    return runs


def predict_ref(labels, pred_scores, masks, superpoints, coords_float, *, num_class, topk_insts=100, score_thr=0.0,
                npoint_thr=100, ge_bits=False, ge_score_thr=False, ge_npoint_thr=False, topk_after=False, renorm=False,
                div_c1=False, no_eps=False, label_c=False):
    """All six steps.  Returns a dict: status, flags, conf f32[K'], label_id i32[K'], query i32[K'], box f32[K', 6],
    masks bool[K', N], counts (list of int64 arrays), stages (candidates, rows after score_thr, rows out)."""
    labels, ps = np.asarray(labels, np.float32), np.asarray(pred_scores, np.float32).reshape(-1)
    ml = np.asarray(masks, np.float32)
    spp, xyz = np.asarray(superpoints, np.int64), np.asarray(coords_float, np.float32).reshape(-1, 3)
    C, Q, S = num_class, labels.shape[0], ml.shape[1]
    flags = 0
    if not (np.isfinite(labels).all() and np.isfinite(ps).all()):
        flags |= FLAG_SCORE
    if not np.isfinite(xyz).all():
        flags |= FLAG_COORDS
    if ((spp < 0) | (spp >= S)).any():
        flags |= FLAG_SPP
    with np.errstate(invalid="ignore", over="ignore"):
        s64 = class_scores64(np.nan_to_num(labels, nan=0.0, posinf=0.0, neginf=0.0),
                             np.nan_to_num(ps, nan=0.0, posinf=0.0, neginf=0.0), renorm).reshape(-1)
    if flags & FLAG_SCORE:  # the rows of the bad queries score 0
        badq = ~(np.isfinite(labels).all(axis=1) & np.isfinite(ps))
        s64 = np.where(np.repeat(badq, C), 0.0, s64)
    s32 = s64.astype(np.float32)
    K = min(topk_insts, Q * C)

    def mask_terms(q):
        x = ml[q]
        with np.errstate(invalid="ignore"):
            bit = x >= 0 if ge_bits else x > 0
        with np.errstate(over="ignore", invalid="ignore"):
            sig = 1.0 / (1.0 + np.exp(-x.astype(np.float64)))
        cnt = bit.sum(axis=-1)
        tot = np.where(bit, sig, 0.0).sum(axis=-1)
        return bit, cnt, tot

    def conf_of(idx):
        q = idx // C
        bit, cnt, tot = mask_terms(q)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            c64 = s64[idx] * tot / (cnt + (0.0 if no_eps else 1e-6))
        return bit, np.where(cnt > 0, c64, 0.0).astype(np.float32) + np.float32(0)

    if topk_after:  # wrong: the top-k of the re-weighted scores
        _, conf_all = conf_of(np.arange(Q * C))
        cand = order_ref(conf_all, K)
    else:
        cand = order_ref(s32, K)
    cq = cand // (C + 1) if div_c1 else cand // C
    cq = np.minimum(cq, Q - 1)
    cc = cand % C
    if not np.isfinite(ml[np.unique(cq)]).all():
        flags |= FLAG_MASK
    out = {"status": status_of(flags), "flags": flags}
    if flags:
        return out
    bit, cnt, tot = mask_terms(cq)
    with np.errstate(invalid="ignore", divide="ignore"):
        c64 = s64[cand] * tot / (cnt + (0.0 if no_eps else 1e-6))
    conf = np.where(cnt > 0, c64, 0.0).astype(np.float32) + np.float32(0)
    n, lo, hi = tables_ref(spp, xyz, S)
    npoints = (bit.astype(np.int64) * n[None, :]).sum(axis=1)
    thr = np.float32(score_thr)
    keep1 = conf >= thr if ge_score_thr else conf > thr
    keep2 = keep1 & (npoints >= npoint_thr if ge_npoint_thr else npoints > npoint_thr)
    rows = np.nonzero(keep2)[0]
    rows = rows[np.lexsort((rows, -conf[rows].astype(np.float64)))]
    box = np.zeros((len(rows), 6), np.float32)
    for r, k in enumerate(rows):
        on = bit[k] & (n > 0)
        if on.any():
            box[r, :3] = order_image_inv(lo[on].min(axis=0))
            box[r, 3:] = order_image_inv(hi[on].max(axis=0))
    pmask = bit[rows][:, spp] if len(rows) else np.zeros((0, len(spp)), bool)
    out.update(conf=conf[rows], label_id=(cc[rows] + (0 if label_c else 1)).astype(np.int32),
               query=cq[rows].astype(np.int32), box=box, masks=pmask, counts=[rle_ref(m) for m in pmask],
               stages=(len(cand), int(keep1.sum()), len(rows)), npoints=npoints[rows], cand_scores=s32[cand])
    return out


# ---- the golden fixtures (tests/golden/make_golden_spf_predict.py) -------------------------------------------------
FIXTURES = ["plain", "few_queries", "score_thr", "npoint_negative"]
INPUTS = ("labels", "pred_scores", "masks", "superpoints", "coords_float")


def load_fixture(name):
    """(kwargs of predict_ref, (label_id, conf, list of counts, box) of the reference)."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spf_predict_%s.npz" % name))
    kw = {k: z[k] for k in INPUTS}
    kw.update(num_class=int(z["num_class"]), topk_insts=int(z["topk_insts"]), score_thr=float(z["score_thr"]),
              npoint_thr=int(z["npoint_thr"]))
    off = z["ref_offsets"]
    counts = [z["ref_counts"][off[i]:off[i + 1]] for i in range(len(off) - 1)]
    return kw, (z["ref_label_id"], z["ref_conf"], counts, z["ref_box"])


def _order_free(label, counts):
    return sorted(range(len(label)), key=lambda i: (int(label[i]), np.asarray(counts[i], np.int64).tobytes()))


def compare_with_reference(ours, label, conf, counts, box):
    """The order-free comparison: both sides sorted by (label_id, counts bytes); labels and counts must agree exactly
    and the boxes as float32 values.  Returns the largest relative deviation of conf."""
    assert ours["status"] == OK and len(ours["label_id"]) == len(label), (len(ours.get("label_id", ())), len(label))
    a, b = _order_free(ours["label_id"], ours["counts"]), _order_free(label, counts)
    worst = 0.0
    for i, j in zip(a, b):
        assert int(ours["label_id"][i]) == int(label[j])
        assert np.array_equal(ours["counts"][i], np.asarray(counts[j], np.int64))
        assert np.array_equal(np.asarray(ours["box"][i], np.float32), np.asarray(box[j], np.float32))
        x, y = float(ours["conf"][i]), float(conf[j])
        worst = max(worst, abs(x - y) / max(abs(y), 1e-30))
    return worst
