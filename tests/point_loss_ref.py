"""NumPy float64 restatement of the criterion's four point-wise losses (ISBNet/isbnet/model/criterion.py:136-191) as
gapro_point_loss_forward / _backward define them (include/gapro_hip.h, "Point-wise losses"): every term in float64 from
the float32 inputs, the two boxes a = c + [x, x] and b = l + [x, x] formed in float64 too; losses and their analytic
gradients.  Also the fixtures' loader.  Nothing here is used by the product.
"""
import os

import numpy as np

from loss_ref import GOLDEN, _giou, close  # noqa: F401  (close: the comparison the tests share)

FIXTURES = ["mixed", "weighted", "nopos"]
NAMES = ("pw_sem_loss", "pw_corners_loss", "pw_giou_loss", "pw_conf_loss")
UPSTREAM = np.array([0.9, 1.3, 0.6, 1.7])
ARGS = ("semantic_scores", "corners_offset", "box_conf", "semantic_labels", "instance_labels", "corners_offset_labels",
        "coords_float")


def boxes(corners_offset, corners_offset_labels, coords_float):
    """The point-wise boxes in float64: predicted and label, [N, 6] each."""
    x2 = np.tile(np.asarray(coords_float, dtype=np.float64), (1, 2))
    return np.asarray(corners_offset, dtype=np.float64) + x2, np.asarray(corners_offset_labels, dtype=np.float64) + x2


def iou_of(p, g):
    """The IoU of model_utils.py:416-444 per row (what _giou folds into its loss)."""
    with np.errstate(all="ignore"):
        a0, a1, b0, b1 = p[:, :3], p[:, 3:], g[:, :3], g[:, 3:]
        inter = np.clip(np.minimum(a1, b1) - np.maximum(a0, b0), 0.0, None).prod(1)
        uni = np.clip(b1 - b0, 0.0, None).prod(1) + np.clip(a1 - a0, 0.0, None).prod(1) - inter
        # np.minimum / np.maximum / np.clip hand a NaN on, as torch's
        return inter / (uni + 1e-6)


def losses(semantic_scores, corners_offset, box_conf, semantic_labels, instance_labels, corners_offset_labels,
           coords_float, semantic_weight=None, ignore_label=-100, voxel_scale=50, upstream=None):
    """The four losses in float64 (NAMES' order) and, with ``upstream`` (four weights), the gradients of
    sum_k upstream[k] loss[k]: ``{"scores": [N, C], "corners": [N, 6], "conf": [N]}``.  A semantic label that is neither
    ``ignore_label`` nor a class is the caller's error."""
    z = np.asarray(semantic_scores, dtype=np.float64)
    N, C = z.shape
    c, l = np.asarray(corners_offset, dtype=np.float64), np.asarray(corners_offset_labels, dtype=np.float64)
    conf = np.asarray(box_conf, dtype=np.float64).reshape(N)
    y, inst = np.asarray(semantic_labels, dtype=np.int64), np.asarray(instance_labels, dtype=np.int64)
    w_all = np.ones(C) if semantic_weight is None else np.asarray(semantic_weight, dtype=np.float32).astype(np.float64)
    keep, pos = y != ignore_label, inst != ignore_label
    assert ((y[keep] >= 0) & (y[keep] < C)).all()
    n = int(pos.sum())
    l1_scale = float(voxel_scale) / 50.0
    with np.errstate(all="ignore"):
        yk = np.where(keep, y, 0)
        m = z.max(1, keepdims=True) if N else np.zeros((0, 1))
        lse = (m + np.log(np.exp(z - m).sum(1, keepdims=True)))[:, 0]
        wt = np.where(keep, w_all[yk], 0.0)
        wsum = wt.sum()
        sem = (wt[keep] * (lse - z[np.arange(N), yk])[keep]).sum() / wsum  # every label ignored: 0 / 0
        a, b = boxes(c, l, coords_float)
        gl, ggrad = _giou(a[pos], b[pos], upstream is not None)
        iou = iou_of(a[pos], b[pos])
        if n:
            vals = np.array([sem, l1_scale * np.abs(c[pos] - l[pos]).sum() / n, gl.sum() / n,
                             ((conf[pos] - iou) ** 2).sum() / n])
        else:
            vals = np.array([sem, 0.0, 0.0, 0.0])
        if upstream is None:
            return vals
        up = np.asarray(upstream, dtype=np.float64)
        g_z = np.zeros((N, C))
        dz = z - lse[:, None]
        soft = np.where(np.arange(C)[None, :] == yk[:, None], np.expm1(dz), np.exp(dz))
        g_z[keep] = ((up[0] / wsum) * wt[:, None] * soft)[keep]
        g_c, g_conf = np.zeros((N, 6)), np.zeros(N)
        if n:
            g_c[pos] = up[1] * l1_scale / n * np.sign(c[pos] - l[pos]) + up[2] / n * ggrad
            g_conf[pos] = up[3] * 2.0 * (conf[pos] - iou) / n
    return vals, {"scores": g_z, "corners": g_c, "conf": g_conf}


def fixture(name):
    """A fixture of tests/golden/make_golden_point_losses.py: the npz and the call's arguments as NumPy arrays."""
    z = np.load(os.path.join(GOLDEN, "point_losses_%s.npz" % name))
    args = {k: z[k] for k in ARGS}
    args["semantic_weight"] = z["semantic_weight"] if "semantic_weight" in z.files else None
    return z, args
