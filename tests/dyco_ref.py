"""NumPy float64 restatement of the dynamic-convolution mask head (include/gapro_hip.h, "Dynamic-convolution mask
head"): the forward and the hand-derived backward, rounded once to float32 by ``head`` /
``head_backward``.  ``variant`` names ONE deliberately wrong convention (tests/test_dyco_cpu.py shows that each fails)."""
import numpy as np

VARIANTS = ("geometry_last", "point_minus_query", "no_abs", "abs_coords", "w1_transposed", "add_b3", "min_minus_max",
            "relu_one_at_zero", "sign_one_at_zero")


def param_count(C):
    H = C // 2
    return (C + 6) * C + C * H + H + C + H + 1


def split_params(theta, C, variant=None):
    """theta [Q, P] -> W1 [Q, C + 6, C], W2 [Q, C, H], W3 [Q, H], b1 [Q, C], b2 [Q, H], b3 [Q]."""
    theta = np.asarray(theta, dtype=np.float64)
    Q, H = theta.shape[0], C // 2
    assert theta.shape[1] == param_count(C)
    sizes = [(C + 6) * C, C * H, H, C, H, 1]
    parts = np.split(theta, np.cumsum(sizes)[:-1], axis=1)
    W1 = parts[0].reshape(Q, C + 6, C)
    if variant == "w1_transposed":
        W1 = parts[0].reshape(Q, C, C + 6).transpose(0, 2, 1)
    return W1, parts[1].reshape(Q, C, H), parts[2], parts[3], parts[4], parts[5][:, 0]


def inputs(feats, locs, box, qloc, qbox, variant=None):
    """x [Q, N, C + 6] and d [Q, N, 3], the box-dimension differences before the abs."""
    feats, locs, box, qloc, qbox = (np.asarray(t, dtype=np.float64) for t in (feats, locs, box, qloc, qbox))
    rel = qloc[:, None, :] - locs[None, :, :]
    if variant == "point_minus_query":
        rel = -rel
    if variant == "abs_coords":
        rel = np.abs(rel)
    qd, pd = qbox[:, 3:] - qbox[:, :3], box[:, 3:] - box[:, :3]
    if variant == "min_minus_max":
        qd, pd = -qd, -pd
    d = qd[:, None, :] - pd[None, :, :]
    ad = d if variant == "no_abs" else np.abs(d)
    f = np.broadcast_to(feats[None], (qloc.shape[0],) + feats.shape)
    x = np.concatenate([f, rel, ad] if variant == "geometry_last" else [rel, ad, f], axis=2)
    return x, d


def forward(theta, feats, locs, box, qloc, qbox, variant=None, full=False):
    """y [Q, N] in float64 (with ``full``: also x, d and the two pre-activations)."""
    C = np.asarray(feats).shape[1]
    W1, W2, W3, b1, b2, b3 = split_params(theta, C, variant)
    x, d = inputs(feats, locs, box, qloc, qbox, variant)
    p1 = np.einsum("qaj,qna->qnj", W1, x) + b1[:, None, :]
    h1 = np.maximum(p1, 0.0)
    p2 = np.einsum("qjk,qnj->qnk", W2, h1) + b2[:, None, :]
    h2 = np.maximum(p2, 0.0)
    y = np.einsum("qk,qnk->qn", W3, h2)
    if variant == "add_b3":
        y = y + b3[:, None]
    return (y, x, d, p1, p2) if full else y


def backward(theta, feats, locs, box, qloc, qbox, gy, variant=None):
    """The hand-derived gradients in float64: d_theta [Q, P], d_feats [N, C], d_box [N, 6], d_qbox [Q, 6]."""
    C = np.asarray(feats).shape[1]
    W1, W2, W3, b1, b2, b3 = split_params(theta, C)
    y, x, d, p1, p2 = forward(theta, feats, locs, box, qloc, qbox, full=True)
    gy = np.asarray(gy, dtype=np.float64)
    on = (lambda p: p >= 0.0) if variant == "relu_one_at_zero" else (lambda p: p > 0.0)
    h1, h2 = np.maximum(p1, 0.0), np.maximum(p2, 0.0)
    dh2 = gy[:, :, None] * W3[:, None, :] * on(p2)
    dW3 = np.einsum("qn,qnk->qk", gy, h2)
    db2 = dh2.sum(axis=1)
    dW2 = np.einsum("qnj,qnk->qjk", h1, dh2)
    dh1 = np.einsum("qjk,qnk->qnj", W2, dh2) * on(p1)
    db1 = dh1.sum(axis=1)
    dW1 = np.einsum("qna,qnj->qaj", x, dh1)
    dx = np.einsum("qaj,qnj->qna", W1, dh1)
    Q = dW1.shape[0]
    d_theta = np.concatenate([dW1.reshape(Q, -1), dW2.reshape(Q, -1), dW3, db1, db2, np.zeros((Q, 1))], axis=1)
    sign = np.sign(d)
    if variant == "sign_one_at_zero":
        sign = np.where(d >= 0.0, 1.0, -1.0)
    dd = dx[:, :, 3:6] * sign            # gradient of d = q_dim - p_dim
    dq, dp = dd.sum(axis=1), -dd.sum(axis=0)
    d_qbox = np.concatenate([-dq, dq], axis=1)
    d_box = np.concatenate([-dp, dp], axis=1)
    return d_theta, dx[:, :, 6:].sum(axis=0), d_box, d_qbox


def head(controllers, feats, locs, box, qlocs, qboxes, off):
    """``dynamic_mask_head``: a list of float32 [Q, N_b], ``None`` for a sample without points."""
    feats = np.asarray(feats).reshape(np.asarray(feats).shape[0], -1)
    out = []
    for b, (lo, hi) in enumerate(zip(off, off[1:])):
        out.append(None if hi == lo else forward(controllers[b], feats[lo:hi], locs[lo:hi], box[lo:hi], qlocs[b],
                                                 qboxes[b]).astype(np.float32))
    return out


def head_backward(controllers, feats, locs, box, qlocs, qboxes, off, grads):
    """The four gradients of ``dynamic_mask_head`` (float32, whole arrays) for the upstream ``grads`` (a list as
    ``head`` returns; ``None`` where the sample has no points or no upstream gradient)."""
    feats = np.asarray(feats).reshape(np.asarray(feats).shape[0], -1)
    g_ctrl = np.zeros(np.asarray(controllers).shape, dtype=np.float64)
    g_feat = np.zeros(feats.shape, dtype=np.float64)
    g_box = np.zeros((feats.shape[0], 6), dtype=np.float64)
    g_qbox = np.zeros(np.asarray(qboxes).shape, dtype=np.float64)
    for b, (lo, hi) in enumerate(zip(off, off[1:])):
        if hi == lo or grads[b] is None:
            continue
        g_ctrl[b], g_feat[lo:hi], g_box[lo:hi], g_qbox[b] = backward(
            controllers[b], feats[lo:hi], locs[lo:hi], box[lo:hi], qlocs[b], qboxes[b], grads[b])
    return {"controllers": g_ctrl.astype(np.float32), "mask_features": g_feat.astype(np.float32),
            "box_preds": g_box.astype(np.float32), "queries_box_preds": g_qbox.astype(np.float32)}
