"""NumPy restatement of the predicted-instance chain (include/gapro_hip.h, "Predicted instances").  No
device.  Floating-point terms are float64 from the float32 inputs, rounded to float32 once; everything else is integer.

The keyword switches at the end of ``get_instance_ref`` / ``nms_ref`` select the *wrong* conventions the edge cases are
built to tell apart (tests/test_proposals_cpu.py); the definition is all of them off.  ``first_pass`` names loops of
csrc/proposals.hip that are cut to their first trip (FIRST_PASS; tests/test_proposals_scale_cpu.py): the definition is
the empty set.
"""
import numpy as np

import proposals_cases as _sizes  # the mirrored kernel constants live with the cases built around them

FIRST_PASS = ("pack_run", "pack_grid", "inter", "score_grid", "points_grid", "tally", "index16", "index8", "nms256",
              "finish_rows")

OK, ERR_BAD_ARG, ERR_NOT_FINITE, ERR_SPP_RANGE = 0, -1, -4, -6
FLAG_SCORE, FLAG_MASK, FLAG_V2P, FLAG_VOXEL_SPP, FLAG_SPP = 1, 2, 4, 8, 16


def status_of(flags):
    if flags & (FLAG_SCORE | FLAG_MASK):
        return ERR_NOT_FINITE
    if flags & (FLAG_V2P | FLAG_VOXEL_SPP):
        return ERR_BAD_ARG
    return ERR_SPP_RANGE if flags & FLAG_SPP else OK


def scores_ref(cls_logits, conf_logits):
    """Stage 1: f32[Q, C]."""
    x = np.asarray(cls_logits, np.float32).astype(np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    den = np.zeros(x.shape[0])
    for c in range(x.shape[1]):  # the sum in ascending c
        den = den + e[:, c]
    cf = np.clip(np.asarray(conf_logits, np.float32).astype(np.float64), 0.0, 1.0)
    s = np.sqrt(e[:, :-1] / den[:, None] * cf[:, None]).astype(np.float32)
    return s + np.float32(0)  # never -0.0


def order_ref(values, k, tie_desc_index=False, index_bits=None):
    """The k largest float32 values, descending; equal values by ascending index.  ``index_bits``: wrong, the tie is
    decided by the low bits of the index only."""
    v = np.asarray(values, np.float32)
    idx = np.arange(v.shape[0])
    tie = -idx if tie_desc_index else idx
    if index_bits is not None:
        tie = idx & ((1 << index_bits) - 1)
    order = np.lexsort((tie, -v.astype(np.float64)))
    return order[:k]


def bits_ref(mask_logits, logit_thresh, voxel_spps=None, wrong_tail=False):
    """Stage 2: bool[Q, V]."""
    ml = np.asarray(mask_logits, np.float32)
    if voxel_spps is not None:
        ml = ml[:, np.asarray(voxel_spps, np.int64)]
    bits = ml >= np.float32(logit_thresh)
    if wrong_tail:  # the last word filled from whatever follows the row in memory
        q, v = bits.shape
        flat = np.concatenate([np.ascontiguousarray(ml).reshape(-1), np.full(64, -np.inf, np.float32)])
        w = (v + 63) // 64 * 64
        bits = np.stack([flat[r * v:r * v + w] >= np.float32(logit_thresh) for r in range(q)])
    return bits


def iou_ref(bits, na=None, inter_voxels=None):
    """Stage 3: f32[n, n] from bool[n, V].  ``inter_voxels``: wrong, the intersections over the first voxels only."""
    b = bits.astype(np.float32 if bits.shape[1] < 1 << 24 else np.float64)  # whole numbers below 2^24 / 2^53: exact
    n = bits.sum(axis=1).astype(np.int64) if na is None else np.asarray(na, np.int64)
    if inter_voxels is not None:
        b = b[:, :inter_voxels]
    inter = (b @ b.T).astype(np.int64)
    uni = n[:, None] + n[None, :] - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = inter.astype(np.float32) / uni.astype(np.float32)
    return np.where(uni > 0, iou, np.float32(0)).astype(np.float32)


def nms_ref(bits, classes, scores, type_nms="matrix", topk=100, nms_threshold=0.2, final_score_thresh=0.1,
            cross_class=False, npoints=None, first_pass=()):
    """Stage 4 on candidates already in stage order.  Returns (positions kept, in output order; their scores f32)."""
    n = len(classes)
    scores = np.asarray(scores, np.float32)
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.float32)
    classes = np.asarray(classes)
    iou = iou_ref(bits, npoints, _sizes.INTER_PASS_WORDS * 64 if "inter" in first_pass else None)
    same = np.ones((n, n), bool) if cross_class else classes[:, None] == classes[None, :]
    upper = np.triu(np.ones((n, n), bool), 1)
    if type_nms == "matrix":
        d = np.where(same & upper, iou, np.float32(0)).astype(np.float64)
        c = d.max(axis=0)
        coef = (np.exp(-2.0 * (d * d)) / np.exp(-2.0 * (c * c))[:, None]).min(axis=0)
        new = (scores.astype(np.float64) * coef).astype(np.float32)
        if topk != -1:
            keep = order_ref(new, min(topk, n))
        else:
            keep = order_ref(new, int((new >= np.float32(final_score_thresh)).sum()))
        return keep, new[keep]
    assert type_nms == "standard"
    supp = np.zeros(n, bool)
    place = np.arange(n)
    for i in range(n):
        if supp[i]:
            continue
        hit = same[i] & upper[i] & (iou[i] > np.float32(nms_threshold))
        if "nms256" in first_pass:  # wrong: a pivot sees the NMS_PASS places behind it only
            hit &= place - i <= _sizes.NMS_PASS
        supp |= hit
    keep = np.nonzero(~supp)[0]
    return keep, scores[keep]


def refine_ref(voxel_bits, v2p_map, spps, n_spps, strict=False, n_from=None, c_from=None):
    """Stage 5: bool[K, N] from bool[K, V].  ``n_from`` / ``c_from``: wrong, n(s) / c(k, s) of the first points only."""
    v2p, spps = np.asarray(v2p_map, np.int64), np.asarray(spps, np.int64)
    pts = voxel_bits[:, v2p]
    n = np.bincount(spps[:n_from], minlength=n_spps)
    out = np.zeros(pts.shape, bool)
    for k in range(pts.shape[0]):
        c = np.bincount(spps[:c_from], weights=pts[k, :c_from].astype(np.float64), minlength=n_spps).astype(np.int64)
        on = 2 * c > n if strict else 2 * c >= n
        out[k] = on[spps]
    return out


def rle_ref(mask):
    """Stage 7: the counts of one row, int64."""
    m = np.concatenate([[0], np.asarray(mask).astype(np.int8), [0]])
    runs = np.nonzero(m[1:] != m[:-1])[0].astype(np.int64) + 1
    runs[1::2] -= runs[::2]
    return runs


def rle_chunked_ref(mask, drop_carry=False, hold_chunk_len=False):
    """The counts of one row by the chunked algorithm of `trans`, `chunks` and `runs`: the transitions of every chunk
    of points, their number before each chunk by a scan over SCAN_CHUNKS chunks a step with a carry, the positions
    written from there.  Equal to ``rle_ref`` with both switches off.  ``drop_carry``: wrong, the carry is lost between
    the steps; ``hold_chunk_len``: wrong, a chunk stays at MIN_CHUNK points beyond MAX_CHUNKS chunks."""
    m = np.asarray(mask).astype(np.int8)
    nchunks, chunk_len = _sizes.chunking(len(m))
    if hold_chunk_len:
        chunk_len = min(chunk_len, _sizes.MIN_CHUNK)
    trans = np.nonzero(np.concatenate([m, [0]]) != np.concatenate([[0], m]))[0].astype(np.int64)  # positions, 0-based
    chunk_of = trans // chunk_len
    trans, chunk_of = trans[chunk_of < nchunks], chunk_of[chunk_of < nchunks]
    cnt = np.bincount(chunk_of, minlength=nchunks).astype(np.int64)
    before, carry = np.zeros(nchunks, np.int64), 0
    for j0 in range(0, nchunks, _sizes.SCAN_CHUNKS):
        step = cnt[j0:j0 + _sizes.SCAN_CHUNKS]
        before[j0:j0 + len(step)] = carry + np.cumsum(step) - step
        carry = 0 if drop_carry else carry + int(step.sum())
        last = int(step.sum())
    total = last if drop_carry else carry
    runs = np.zeros(total + (total & 1), np.int64)
    at = before[chunk_of] + (np.arange(len(trans)) - (np.cumsum(cnt) - cnt)[chunk_of])
    ok = at < len(runs)
    runs[at[ok]] = trans[ok] + 1
    runs[1::2] -= runs[::2]
    return runs


def rle_decode_ref(length, counts):
    """The reference's rle_decode rule (isbnet/util/rle.py:72-89), restated."""
    mask = np.zeros(length, np.uint8)
    for lo, num in zip(counts[0::2], counts[1::2]):
        mask[lo - 1:lo - 1 + num] = 1
    return mask


def get_instance_ref(cls_logits, mask_logits, conf_logits, box_preds, v2p_map, semantic_preds, spps, *,
                     instance_classes, logit_thresh=0.0, npoint_thresh=100, type_nms="matrix", topk=100,
                     nms_threshold=0.2, final_score_thresh=0.1, sem2ins_classes=(), label_shift=1, voxel_spps=None,
                     n_spps=None, pre_topk=300, half_strict=False, wrong_tail=False, tie_desc_index=False,
                     cross_class=False, first_pass=()):
    """All seven stages.  Returns a dict: status, flags, conf f32[K], label_id i32[K], query i32[K], box f32[K, 6],
    masks bool[K, N], counts (list of int64 arrays), stages (candidates after stages 1, 2, 4, 5)."""
    cls_logits, conf_logits = np.asarray(cls_logits, np.float32), np.asarray(conf_logits, np.float32)
    ml = np.asarray(mask_logits, np.float32)
    v2p, spps = np.asarray(v2p_map, np.int64), np.asarray(spps, np.int64)
    C, Q = instance_classes, cls_logits.shape[0]
    V = ml.shape[1] if voxel_spps is None else len(voxel_spps)
    N = len(v2p)
    n_spps = int(spps.max()) + 1 if n_spps is None else n_spps
    flags = 0
    if not (np.isfinite(cls_logits).all() and np.isfinite(conf_logits).all()):
        flags |= FLAG_SCORE
    if ((v2p < 0) | (v2p >= V)).any():
        flags |= FLAG_V2P
    if ((spps < 0) | (spps >= n_spps)).any():
        flags |= FLAG_SPP
    vs = None
    if voxel_spps is not None:
        vs = np.asarray(voxel_spps, np.int64)
        bad = (vs < 0) | (vs >= ml.shape[1])
        if bad.any():
            flags |= FLAG_VOXEL_SPP
            vs = np.where(bad, 0, vs)
    with np.errstate(invalid="ignore", over="ignore"):
        score = scores_ref(np.nan_to_num(cls_logits, nan=0.0, posinf=0.0, neginf=0.0),
                           np.nan_to_num(conf_logits, nan=0.0, posinf=0.0, neginf=0.0)).reshape(-1)
    first_pass = (first_pass,) if isinstance(first_pass, str) else tuple(first_pass)
    assert all(f in FIRST_PASS for f in first_pass)
    if "score_grid" in first_pass:  # the queries beyond one pass of `score` keep the cleared score
        score = score.copy()
        score[_sizes.GRID_PASS_ITEMS * C:] = np.float32(0)
    cand = order_ref(score, min(pre_topk, Q * C), tie_desc_index,
                     16 if "index16" in first_pass else 8 if "index8" in first_pass else None)
    cq, cc = cand // C, cand % C
    read = ml if vs is None else ml[:, vs]
    if not np.isfinite(read[np.unique(cq)]).all():
        flags |= FLAG_MASK
    out = {"status": status_of(flags), "flags": flags}
    if flags:
        return out
    bits = bits_ref(ml, logit_thresh, vs, wrong_tail)
    if "pack_grid" in first_pass:  # the (row, run of words) tasks beyond one pass of `pack` leave their words clear
        run_voxels = _sizes.PACK_WORDS * 64
        run = np.arange(bits.shape[1]) // run_voxels
        task = np.arange(bits.shape[0])[:, None] * (int(run[-1]) + 1) + run
        bits = bits & (task < _sizes.PACK_PASS_WAVES)
    npoints = bits[:, :_sizes.PACK_WORDS * 64].sum(axis=1) if "pack_run" in first_pass else bits.sum(axis=1)
    keep = npoints[cq] >= npoint_thresh
    sq, sc, ss = cq[keep], cc[keep], score[cand][keep]
    kept, conf = nms_ref(bits[sq], sc, ss, type_nms, topk, nms_threshold, final_score_thresh, cross_class,
                         npoints[sq], first_pass)
    vbits = bits[:, :V]
    part = dict(n_from=_sizes.GRID_PASS_ITEMS if "points_grid" in first_pass else None,
                c_from=_sizes.TALLY_PASS_POINTS if "tally" in first_pass else None)
    masks = refine_ref(vbits[sq[kept]], v2p, spps, n_spps, half_strict, **part)
    ok = masks.sum(axis=1) >= npoint_thresh
    n_sem = len(sem2ins_classes)
    sem_bits = np.stack([np.asarray(semantic_preds) == i for i in sem2ins_classes]) if n_sem else np.zeros((0, V), bool)
    sem_masks = refine_ref(sem_bits, v2p, spps, n_spps, half_strict, **part)
    query = sq[kept][ok].astype(np.int32)
    box = np.asarray(box_preds, np.float32)[query] if box_preds is not None else np.zeros((len(query), 6), np.float32)
    masks = np.concatenate([sem_masks, masks[ok]])
    cut = slice(0, _sizes.FINISH_PASS_ROWS if "finish_rows" in first_pass else None)  # wrong: four rows a thread
    out.update(
        conf=np.concatenate([np.ones(n_sem, np.float32), conf[ok]]).astype(np.float32)[cut],
        label_id=np.concatenate([np.asarray(sem2ins_classes, np.int64) + 1,
                                 sc[kept][ok] + label_shift]).astype(np.int32)[cut],
        query=np.concatenate([np.full(n_sem, -1, np.int32), query])[cut],
        box=np.concatenate([np.zeros((n_sem, 6), np.float32), box.reshape(-1, 6)])[cut],
        masks=masks[cut], counts=[rle_ref(m) for m in masks[cut]],
        stages=(len(cand), int(keep.sum()), len(kept), int(ok.sum())))
    return out


# ---- the golden fixtures (tests/golden/make_golden_proposals.py) ---------------------------------------------------
FIXTURES = ["matrix", "matrix_topk", "matrix_thresh", "standard", "s3dis", "few_queries"]
_INPUTS = ("cls_logits", "mask_logits", "conf_logits", "box_preds", "v2p_map", "semantic_preds", "spps", "voxel_spps")


def load_fixture(name):
    """(kwargs of get_instance_ref, (label_id, conf, list of counts) of the reference)."""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "proposals_%s.npz" % name))
    kw = {k: z[k] for k in _INPUTS}
    kw.update(n_spps=int(z["n_spps"]), instance_classes=int(z["instance_classes"]), type_nms=str(z["type_nms"]),
              topk=int(z["topk"]), npoint_thresh=int(z["npoint_thresh"]), logit_thresh=float(z["logit_thresh"]),
              nms_threshold=float(z["nms_threshold"]), sem2ins_classes=tuple(int(i) for i in z["sem2ins_classes"]),
              label_shift=int(z["label_shift"]))
    off = z["ref_offsets"]
    counts = [z["ref_counts"][off[i]:off[i + 1]] for i in range(len(off) - 1)]
    return kw, (z["ref_label_id"], z["ref_conf"], counts)


def _order_free(label, counts):
    return sorted(range(len(label)), key=lambda i: (int(label[i]), np.asarray(counts[i], np.int64).tobytes()))


def compare_with_reference(ours, label, conf, counts):
    """The order-free comparison: both sides sorted by (label_id, counts bytes); labels and counts must agree exactly.
    Returns the largest relative deviation of conf."""
    assert ours["status"] == OK and len(ours["label_id"]) == len(label), (len(ours.get("label_id", ())), len(label))
    a, b = _order_free(ours["label_id"], ours["counts"]), _order_free(label, counts)
    worst = 0.0
    for i, j in zip(a, b):
        assert int(ours["label_id"][i]) == int(label[j])
        assert np.array_equal(ours["counts"][i], np.asarray(counts[j], np.int64))
        x, y = float(ours["conf"][i]), float(conf[j])
        worst = max(worst, abs(x - y) / max(abs(y), 1e-30))
    return worst
