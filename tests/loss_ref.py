"""NumPy float64 restatement of the criterion's seven main losses (ISBNet/isbnet/model/criterion.py:235-331) as
gapro_match_loss_forward / _backward define them (include/gapro_hip.h, "Matched losses"): every term in float64 from the
float32 inputs, the level-set membership alone in float32; losses and their analytic gradients.  Also the fixtures'
loader and the comparisons the tests share.  Nothing here is used by the product.
"""
import os

import numpy as np

from match_ref import ulp32

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ["two", "wide", "long"]
NAMES = ("dice_loss", "bce_loss", "cls_loss", "iou_loss", "box_loss", "giou_loss", "levelset_loss")
UPSTREAM = np.array([1.0, 1.0, 0.5, 0.5, 0.5, 0.5, 0.5])  # Criterion.loss_weight, in the order of NAMES


def default_weight(n_classes):
    w = np.ones(n_classes, dtype=np.float32)
    w[-1] = np.float32(0.1)
    return w


def members(coords, box_label):
    """criterion.py:196-198 in float32: [n, S] bool."""
    c = np.asarray(coords, dtype=np.float32)[None, :, :]
    b = np.asarray(box_label, dtype=np.float32)
    lo = (b[:, None, :3] - np.float32(0.005)).astype(np.float32)
    hi = (b[:, None, 3:] + np.float32(0.005)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        return np.all(c >= lo, axis=-1) & np.all(c <= hi, axis=-1)


def _giou(p, g, want_grad):
    """1 - GIoU of model_utils.py:277-306 per row, and its derivative by p ([n, 6]); NaNs pass as in torch."""
    with np.errstate(all="ignore"):
        a0, a1, b0, b1 = p[:, :3], p[:, 3:], g[:, :3], g[:, 3:]
        d_i, d_p, d_b = np.minimum(a1, b1) - np.maximum(a0, b0), a1 - a0, np.maximum(a1, b1) - np.minimum(a0, b0)
        iw, pw, bw = np.clip(d_i, 0.0, None), np.clip(d_p, 0.0, None), np.clip(d_b, 0.0, None)
        inter, pv, bound = iw.prod(1), pw.prod(1), bw.prod(1)
        gv = np.clip(b1 - b0, 0.0, None).prod(1)
        uni = gv + pv - inter
        loss = 1.0 - (inter / (uni + 1e-6) - (bound - uni) / (bound + 1e-6))
        if not want_grad:
            return loss, None
        d_uni = -inter / (uni + 1e-6) ** 2 + 1.0 / (bound + 1e-6)
        g_inter, g_pv, g_bound = 1.0 / (uni + 1e-6) - d_uni, d_uni, -(uni + 1e-6) / (bound + 1e-6) ** 2
        others = lambda v: np.stack([v[:, 1] * v[:, 2], v[:, 2] * v[:, 0], v[:, 0] * v[:, 1]], 1)  # noqa: E731
        ci = np.where(d_i >= 0.0, g_inter[:, None] * others(iw), 0.0)
        cp = np.where(d_p >= 0.0, g_pv[:, None] * others(pw), 0.0)
        cb = np.where(d_b >= 0.0, g_bound[:, None] * others(bw), 0.0)
        share = lambda first: np.where(first, 1.0, 0.0)  # noqa: E731
        tie1, tie0 = 0.5 * (a1 == b1), 0.5 * (a0 == b0)
        grad = np.empty_like(p)
        grad[:, 3:] = -(ci * (share(a1 < b1) + tie1) + cp + cb * (share(a1 > b1) + tie1))
        grad[:, :3] = ci * (share(a0 > b0) + tie0) + cp + cb * (share(a0 < b0) + tie0)
        return loss, grad


def _sample(z, x_all, conf_all, boxp_all, w, feats, coords, rows, t, cls, boxl, weight, l1_scale, up):
    """One kept sample: its seven values and, with ``up`` (the upstream weights already divided by B), the gradients."""
    Q, C = z.shape
    n = len(rows)
    f64 = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    x, t, w, conf, boxp, boxl = f64(x_all)[rows], f64(t), f64(w), f64(conf_all)[rows], f64(boxp_all)[rows], f64(boxl)
    feats, z, weight = f64(feats), f64(z), f64(weight)
    with np.errstate(all="ignore"):
        e = np.exp(-np.abs(x))
        sig = np.where(x >= 0.0, 1.0, e) / (1.0 + e)
        sp = np.maximum(x, 0.0) + np.log1p(e)
        ssig, st, sst = sig.sum(1), t.sum(1), (sig * t).sum(1)
        den, num = ssig + st + 1.0, 2.0 * sst + 1.0
        dice = (1.0 - num / den).sum() / (n + 1e-6)
        sw = w.sum()
        bce = (w[None, :] * (sp - x * t)).sum() / sw / (n + 1e-6)
        pos = x >= 0.0
        inter = (pos * t).sum(1)
        iou = inter / (pos.sum(1) + st - inter + 1e-6)
        iou_loss = ((conf - iou) ** 2).sum() / n
        tgt = np.full(Q, C - 1, dtype=np.int64)
        tgt[rows] = np.asarray(cls, dtype=np.int64)
        m = z.max(1, keepdims=True)
        lse = (m + np.log(np.exp(z - m).sum(1, keepdims=True)))[:, 0]
        wq = weight[tgt]
        wsum = wq.sum()
        cls_loss = (wq * (lse - z[np.arange(Q), tgt])).sum() / wsum
        box_loss = l1_scale * np.abs(boxp - boxl).sum() / n
        gl, ggrad = _giou(boxp, boxl, up is not None)
        giou_loss = gl.sum() / n
        mem = members(coords, boxl)
        n_r = mem.sum(1).astype(np.float64)
        v = sig * mem
        a = v.sum(1)
        mu = (v @ feats) / np.maximum(a, 1e-5)[:, None]                     # [n, F]
        dev = ((feats[None, :, :] - mu[:, None, :]) ** 2).sum(2)             # [n, S]
        keep = n_r > 0
        l_r = np.where(keep, (v * dev).sum(1) / np.where(keep, n_r, 1.0), 0.0)
        levelset = l_r.sum() / (n + 1e-4)
        vals = np.array([dice, bce, cls_loss, iou_loss, box_loss, giou_loss, levelset])
        if up is None:
            return vals, None
        g_cls = (up[2] / wsum) * wq[:, None] * np.where(np.arange(C)[None, :] == tgt[:, None],
                                                       np.expm1(z - lse[:, None]), np.exp(z - lse[:, None]))
        g_conf = np.zeros(Q)
        g_conf[rows] = up[3] * 2.0 * (conf - iou) / n
        g_box = np.zeros((Q, 6))
        g_box[rows] = up[4] * l1_scale / n * np.sign(boxp - boxl) + up[5] / n * ggrad
        sm = e / (1.0 + e)
        dsig = sm / (1.0 + e)
        sig_t = np.where(x >= 0.0, (1.0 - t) - sm, sm - t)
        dv = up[0] / (n + 1e-6) * (num[:, None] - 2.0 * t * den[:, None]) / (den ** 2)[:, None]
        clamped = a < 1e-5
        rf = np.where(clamped[:, None], 2.0 * mu * ((1e-5 - a) / 1e-5)[:, None], 0.0)      # [n, F]
        k_ls = np.where(keep, up[6] / (n + 1e-4) / np.where(keep, n_r, 1.0), 0.0)
        dv = dv + k_ls[:, None] * mem * (dev - rf @ feats.T)
        g_x = np.zeros((Q, x.shape[1]))
        g_x[rows] = dsig * dv + up[1] / (sw * (n + 1e-6)) * w[None, :] * sig_t
        return vals, (g_cls, g_x, g_conf, g_box)


def losses(cls_logits, mask_logits, conf_logits, box_preds, prob_labels, batch_offsets, levelset_feats,
           levelset_coords, gt, empty_weight=None, voxel_scale=50, upstream=None):
    """The seven losses in float64 (NAMES' order) and, with ``upstream`` (seven weights), the gradients of
    sum_k upstream[k] loss[k]: ``{"cls": [B, Q, C], "mask": list, "conf": [B, Q], "box": [B, Q, 6]}``, ``None`` in the
    list for a skipped sample."""
    B, Q, C = np.asarray(cls_logits).shape
    weight = default_weight(C) if empty_weight is None else np.asarray(empty_weight, dtype=np.float32)
    total = np.zeros(7)
    up = None if upstream is None else np.asarray(upstream, dtype=np.float64) / B
    grads = {"cls": np.zeros((B, Q, C)), "mask": [None] * B, "conf": np.zeros((B, Q)), "box": np.zeros((B, Q, 6))}
    for b in range(B):
        if mask_logits[b] is None or gt["row_indices"][b] is None:
            continue
        s0, s1 = int(batch_offsets[b]), int(batch_offsets[b + 1])
        rows = np.asarray(gt["row_indices"][b], dtype=np.int64)
        vals, g = _sample(np.asarray(cls_logits)[b], mask_logits[b], np.asarray(conf_logits)[b],
                          np.asarray(box_preds)[b], np.asarray(prob_labels)[s0:s1], np.asarray(levelset_feats)[s0:s1],
                          np.asarray(levelset_coords)[s0:s1], rows, gt["inst_labels"][b], gt["cls_labels"][b],
                          gt["box_labels"][b], weight, float(voxel_scale) / 50.0, up)
        total += vals
        if g is not None:
            grads["cls"][b], grads["mask"][b], grads["conf"][b], grads["box"][b] = g
    total /= B
    return (total, grads) if upstream is not None else total


def without_clamp_term(g_row, x_row, mem_row, feats, k_ls):
    """A matched row's mask-logit gradient as it would be with the derivative of the clamped mean left out (the wrong
    form the clamped cases guard against): ``g_row`` of the restatement, minus the term that `rf` adds there.  ``k_ls``
    is the row's level-set coefficient, upstream / B / (n + 1e-4) / members.  Only for a row below the clamp."""
    x, feats = np.asarray(x_row, dtype=np.float64), np.asarray(feats, dtype=np.float64)
    sig = 1.0 / (1.0 + np.exp(-x))
    v = sig * mem_row
    a = v.sum()
    assert a < 1e-5
    rf = 2.0 * ((v @ feats) / 1e-5) * (1e-5 - a) / 1e-5
    return np.asarray(g_row, dtype=np.float64) + sig * (1.0 - sig) * k_ls * mem_row * (feats @ rf)


def close(got, want):
    """Device against the restatement: 1 float32 ulp of the value plus 1e-9 times the array's largest magnitude.  The
    float64 sums of the two differ by their order alone (the argument of match_ref.close), so the rounded results
    differ only where a value sits on a float32 rounding boundary."""
    got, want = np.asarray(got), np.asarray(want, dtype=np.float64)
    assert got.dtype == np.float32 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    if got.size == 0:
        return True
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaNs differ"
    ok = ~np.isnan(want)
    if not ok.any():
        return True
    with np.errstate(all="ignore"):
        want32 = want.astype(np.float32)
    err = np.abs(got.astype(np.float64) - want)[ok]
    bound = (ulp32(want32) + 1e-9 * np.abs(want[ok]).max())[ok]
    assert (err <= bound).all(), "max error %.3g at a bound of %.3g" % (err.max(), bound[err.argmax()])
    return True


def fixture(name):
    """A fixture of tests/golden/make_golden_losses.py: the npz, the call's arguments as NumPy arrays and the gt dict."""
    z = np.load(os.path.join(GOLDEN, "losses_%s.npz" % name))
    B = int(z["batch_size"])
    none = [bool(v) for v in z["is_none"]]
    pick = lambda k: [None if none[b] else z["%s_%d" % (k, b)] for b in range(B)]  # noqa: E731
    gt = {"row_indices": pick("row"), "inst_labels": pick("inst"), "cls_labels": pick("cls"), "box_labels": pick("box")}
    args = {"cls_logits": z["cls_logits"], "mask_logits": pick("mask_logits"), "conf_logits": z["conf_logits"],
            "box_preds": z["box_preds"], "prob_labels": z["prob_labels"], "batch_offsets": z["batch_offsets"],
            "levelset_feats": z["levelset_feats"], "levelset_coords": z["levelset_coords"]}
    return z, args, gt
