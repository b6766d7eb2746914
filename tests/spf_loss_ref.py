"""NumPy float64 restatement of SPFormer's criterion as gapro_spf_loss_forward / _backward define it
(include/gapro_hip.h, "SPFormer's criterion"): the matcher's cost matrix, the five losses of every head
and their analytic gradients, every term in float64 from the float32 inputs, the level-set membership alone in float32.
Written from the rule, not from the reference's text.  Also the fixtures' loader.  Nothing here is used by the product.
"""
import os

import numpy as np

from loss_ref import members

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ["three", "one", "wide"]
NAMES = ("cls_loss", "mask_bce_loss", "mask_dice_loss", "score_loss", "levelset_loss")  # the table's columns
OUT_NAMES = ("cls_loss", "score_loss", "mask_bce_loss", "mask_dice_loss", "levelset_loss")  # loss_out's order
LOSS_WEIGHT = np.array([1.0, 1.0, 1.0, 1.0, 0.5])  # Criterion.loss_weight, in the order of NAMES


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _terms(x):
    with np.errstate(all="ignore"):
        e = np.exp(-np.abs(x))
        return e, np.where(x >= 0.0, 1.0, e) / (1.0 + e), np.maximum(x, 0.0) + np.log1p(e)


def cost_matrix(labels, mask_logits, gt_labels, gt_masks, cost_weight=(1.0, 1.0, 1.0)):
    """The matcher's cost of one head and sample in float64: [Q, n]."""
    z, x, t = _f64(labels), _f64(mask_logits), _f64(gt_masks)
    m = z.max(1, keepdims=True)
    soft = np.exp(z - m) / np.exp(z - m).sum(1, keepdims=True)
    _, sig, sp = _terms(x)
    S = x.shape[1]
    bce = (sp.sum(1)[:, None] - x @ t.T) / S
    dice = 1.0 - (2.0 * sig @ t.T + 1.0) / (sig.sum(1)[:, None] + t.sum(1)[None, :] + 1.0)
    return cost_weight[0] * -soft[:, np.asarray(gt_labels, dtype=np.int64)] + cost_weight[1] * bce + cost_weight[2] * dice


def iou_kept(inter, union):
    """The score filter as the integer predicate the kernels use."""
    return 2 * inter > union


def _sample(x_all, score_all, w, feats, coords, rows, t, box, up, dice_scale, B, weighted_bce, min_points):
    """One kept sample of one head: (bce, dice, score, levelset) before the divisions by B and, with ``up`` (the head's
    five upstream weights), the gradients by the mask logits [Q, S] and the scores [Q]."""
    n, S = len(rows), x_all.shape[1]
    x, t, w, score, feats = _f64(x_all)[rows], _f64(t), _f64(w), _f64(score_all)[rows], _f64(feats)
    with np.errstate(all="ignore"):
        e, sig, sp = _terms(x)
        ssig, st, sst = sig.sum(1), t.sum(1), (sig * t).sum(1)
        den, num = ssig + st + 1.0, 2.0 * sst + 1.0
        dice = (1.0 - num / den).sum() / n
        sw = w.sum()
        if weighted_bce:
            m_s, scale = w, 1.0 / sw / n
        else:
            m_s, scale = np.ones(S), (sw / sw) / (n * S)
        bce = (m_s[None, :] * (sp - x * t)).sum() * scale
        pos = x >= 0.0
        inter = (pos * t).sum(1)
        union = pos.sum(1) + st - inter
        iou = inter / (union + 1e-6)
        kept = iou_kept(inter.astype(np.int64), union.astype(np.int64))
        n_kept = int(kept.sum())
        score_loss = ((score - iou)[kept] ** 2).sum() / n_kept if n_kept else 0.0
        mem = members(coords, box)
        n_r = mem.sum(1).astype(np.float64)
        v = sig * mem
        a = v.sum(1)
        mu = (v @ feats) / np.maximum(a, 1e-5)[:, None]                     # [n, F]
        dev = ((feats[None, :, :] - mu[:, None, :]) ** 2).sum(2)             # [n, S]
        keep = n_r >= min_points
        l_r = np.where(keep, (v * dev).sum(1) / np.where(keep, n_r, 1.0), 0.0)
        levelset = l_r.sum() / (n + 1e-4)
        vals = np.array([bce, dice, score_loss, levelset])
        if up is None:
            return vals, None
        g_score = np.zeros(x_all.shape[0])
        if n_kept:
            g_score[rows] = np.where(kept, up[3] / B * 2.0 * (score - iou) / n_kept, 0.0)
        sm = e / (1.0 + e)
        dsig = sm / (1.0 + e)
        sig_t = np.where(x >= 0.0, (1.0 - t) - sm, sm - t)
        dv = up[2] * dice_scale / n * (num[:, None] - 2.0 * t * den[:, None]) / (den ** 2)[:, None]
        clamped = a < 1e-5
        rf = np.where(clamped[:, None], 2.0 * mu * ((1e-5 - a) / 1e-5)[:, None], 0.0)      # [n, F]
        k_ls = np.where(keep, up[4] / B / (n + 1e-4) / np.where(keep, n_r, 1.0), 0.0)
        dv = dv + k_ls[:, None] * mem * (dev - rf @ feats.T)
        g_x = np.zeros(x_all.shape)
        g_x[rows] = dsig * dv + up[1] / B * scale * m_s[None, :] * sig_t
        return vals, (g_x, g_score)


def layer_losses(labels, scores, masks, gts, indices, sp_coords, sp_feats, sp_prob, offsets=None, *,
                 non_object_weight=0.1, weighted_bce=False, dice_div_main=False, min_points=100, upstream=None):
    """The table [L1, 5] in float64 (NAMES' order; the main head last) and, with ``upstream`` ([L1, 5]), the gradients
    of sum(upstream * table): ``{"labels": [L1, B, Q, C], "scores": [L1, B, Q], "masks": [L1][B] of [Q, S_b] or None}``.
    ``gts[b]`` is ``None`` or ``(gt_labels, gt_masks, gt_boxes)``; ``indices[h][b]`` is ``(rows, cols)``."""
    L1 = len(labels)
    B, Q, C = np.asarray(labels[0]).shape
    if offsets is None:
        offsets = np.cumsum([0] + [np.asarray(x).shape[1] for x in masks[0]])
    table = np.zeros((L1, 5))
    grads = {"labels": np.zeros((L1, B, Q, C)), "scores": np.zeros((L1, B, Q)), "masks": [[None] * B for _ in range(L1)]}
    weight = np.ones(C)
    weight[-1] = non_object_weight
    for h in range(L1):
        z = _f64(labels[h])
        up = None if upstream is None else _f64(upstream)[h]
        dice_scale = 1.0 if h == L1 - 1 and not dice_div_main else 1.0 / B
        tgt = np.full((B, Q), C - 1, dtype=np.int64)
        for b in range(B):
            if gts[b] is not None:
                rows, cols = (np.asarray(v, dtype=np.int64) for v in indices[h][b])
                tgt[b, rows] = np.asarray(gts[b][0], dtype=np.int64)[cols]
        m = z.max(2, keepdims=True)
        lse = (m + np.log(np.exp(z - m).sum(2, keepdims=True)))[..., 0]
        wq = weight[tgt]
        wsum = wq.sum()
        table[h, 0] = (wq * (lse - np.take_along_axis(z, tgt[..., None], 2)[..., 0])).sum() / wsum
        if up is not None:
            grads["labels"][h] = (up[0] / wsum) * wq[..., None] * np.where(
                np.arange(C)[None, None, :] == tgt[..., None], np.expm1(z - lse[..., None]), np.exp(z - lse[..., None]))
        total = np.zeros(4)
        for b in range(B):
            if gts[b] is None:
                continue
            rows, cols = (np.asarray(v, dtype=np.int64) for v in indices[h][b])
            s0, s1 = int(offsets[b]), int(offsets[b + 1])
            x_all = np.asarray(masks[h][b])
            vals, g = _sample(x_all, np.asarray(scores[h]).reshape(B, Q)[b], np.asarray(sp_prob)[s0:s1],
                              np.asarray(sp_feats)[s0:s1], np.asarray(sp_coords)[s0:s1], rows,
                              np.asarray(gts[b][1])[cols], np.asarray(gts[b][2])[cols], up, dice_scale, B, weighted_bce,
                              min_points)
            total += vals
            if g is not None:
                grads["masks"][h][b], grads["scores"][h, b] = g
        table[h, 1] = total[0] / B
        table[h, 2] = total[1] * dice_scale
        table[h, 3] = total[2] / B
        table[h, 4] = total[3] / B
    return (table, grads) if upstream is not None else table


def fixture(name):
    """A fixture of tests/golden/make_golden_spf_losses.py: the npz and the call's arguments as NumPy arrays, the heads
    in decoder order (the main head last)."""
    z = np.load(os.path.join(GOLDEN, "spf_losses_%s.npz" % name))
    L1, B = int(z["n_heads"]), int(z["batch_size"])
    skipped = [bool(v) for v in z["is_skipped"]]
    gts = [None if skipped[b] else (z["gt_labels_%d" % b], z["gt_spmasks_%d" % b], z["gt_boxes_%d" % b])
           for b in range(B)]
    args = {"labels": [z["labels_%d" % h] for h in range(L1)], "scores": [z["scores_%d" % h] for h in range(L1)],
            "masks": [[z["masks_%d_%d" % (h, b)] for b in range(B)] for h in range(L1)], "gts": gts,
            "indices": [[(z["rows_%d_%d" % (h, b)], z["cols_%d_%d" % (h, b)]) for b in range(B)] for h in range(L1)],
            "sp_coords": z["sp_coords"], "sp_rgb_feats": z["sp_rgb_feats"], "sp_prob_labels": z["sp_prob_labels"],
            "batch_offsets": z["batch_offsets"]}
    return z, args


def table_of(z, key):
    """A run's loss_out as the table [L1, 5] in NAMES' order."""
    return np.asarray(z[key], dtype=np.float64)
