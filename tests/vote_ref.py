"""NumPy restatement of the superpoint vote (include/gapro_hip.h "Superpoint vote" and gapro_point_refine_vote): the rules
as the header states them, with explicit sequential loops wherever an order is stated.  Written from the header, not
from the kernels; the tests compare the device results with it bit for bit."""
import json
import os

import numpy as np

from oracle.gen_ps_oracle import fixed_point_shift

NAN32 = np.array([0x7fc00000], dtype=np.uint32).view(np.float32)[0]

HERE = os.path.dirname(os.path.abspath(__file__))
SCENES = ("s0_walls", "s1_nowalls", "s2_dense", "s3_bigspp", "s4_dups", "s5_lean")


def fixture(name):
    return np.load(os.path.join(HERE, "golden", "votes_%s.npz" % name))


def prob_tolerance():
    """4 x the largest |reference - restatement| that make_golden_votes.py measured: the reference sums float32 in an
    order that is not specified, the margin covers another order."""
    with open(os.path.join(HERE, "golden", "votes_SUMMARY.json")) as f:
        rec = json.load(f)["max_abs_prob_diff"]
    assert 0 < rec < 1e-6
    return 4 * rec


def _fixed(x32, k):
    """rint(x * 2^k) as int64 for float32 values."""
    return np.rint(np.ldexp(np.asarray(x32, dtype=np.float32).astype(np.float64), k)).astype(np.int64)


def _counts(ids, label, S, C):
    cnt = np.zeros((S, C), dtype=np.int64)
    np.add.at(cnt, (ids, label), 1)
    return cnt


def _prob_sums(ids, label, prob, S, C):
    prob = np.asarray(prob, dtype=np.float32)
    k = fixed_point_shift(float(np.max(np.abs(prob))) if prob.size else 0.0, len(prob))
    P = np.zeros((S, C), dtype=np.int64)
    np.add.at(P, (ids, label), _fixed(prob, k))
    return P, k


def _first_max(m):
    """First maximum of every row over ascending class (an all-zero row gives 0)."""
    out = np.zeros(m.shape[0], dtype=np.int64)
    for s in range(m.shape[0]):
        best, best_m = 0, -1
        for c in range(m.shape[1]):
            if m[s, c] > best_m:
                best, best_m = c, m[s, c]
        out[s] = best
    return out


def spp_align_label(spp, label, n_classes=-1, bb_occupancy_spp=None, prob_label=None):
    _, ids = np.unique(np.asarray(spp), return_inverse=True)
    label = np.asarray(label).astype(np.int64)
    C = int(label.max()) + 1 if n_classes == -1 else int(n_classes)
    S = int(ids.max()) + 1
    cnt = _counts(ids, label, S, C)
    m = cnt.copy()
    if bb_occupancy_spp is not None:
        m[:, 1:] = m[:, 1:] * (np.asarray(bb_occupancy_spp) == 1).T
    lab = _first_max(m)[ids]
    if prob_label is None:
        return lab
    P, k = _prob_sums(ids, label, prob_label, S, C)
    n = cnt.sum(axis=1)
    mean = (np.ldexp(P.sum(axis=1).astype(np.float64), -k) / n.astype(np.float64)).astype(np.float32)
    return lab, mean[ids]


def spp_major_voting(spp, label, prob_label, bb_occupancy, n_classes):
    _, ids = np.unique(np.asarray(spp), return_inverse=True)
    label = np.asarray(label).astype(np.int64)
    C, S = int(n_classes), int(ids.max()) + 1
    cnt = _counts(ids, label, S, C)
    n = cnt.sum(axis=1)
    occn = np.zeros((S, C - 1), dtype=np.int64)
    np.add.at(occn, ids, (np.asarray(bb_occupancy).reshape(len(ids), C - 1) != 0).astype(np.int64))
    m = cnt.copy()
    m[:, 1:] = m[:, 1:] * (occn == n[:, None])
    P, k = _prob_sums(ids, label, prob_label, S, C)
    prob = np.zeros(S, dtype=np.float32)
    for s in range(S):
        acc = np.float64(0.0)
        for c in range(C):  # ascending, every operation rounded on its own
            mean = np.ldexp(np.float64(P[s, c]), -k) / (np.float64(cnt[s, c]) + np.float64(1e-4))
            share = np.float64(m[s, c]) / np.float64(n[s])
            acc = acc + mean * share
        prob[s] = np.float32(acc)
    return _first_max(m)[ids], prob[ids]


def _mean32(vals32, k, count):
    vals32 = np.asarray(vals32, dtype=np.float32)
    if not np.isfinite(vals32).all():
        return NAN32
    total = int(_fixed(vals32, k).sum()) if len(vals32) else 0
    return np.float32(np.ldexp(np.float64(total), -k) / np.float64(count))


def _shift(vals32, n_rows):
    a = np.abs(np.asarray(vals32, dtype=np.float32))
    a = a[np.isfinite(a)]
    return fixed_point_shift(float(a.max()) if a.size else 0.0, n_rows)


def take(p_rows, status_ok):
    """The per-row merge: p_rows f32[n_seg] in tester order -> position of the taking segment or -1, and best."""
    best, took = np.float32(0.0), -1
    for s in range(len(p_rows)):
        if not status_ok[s]:
            continue
        if best < p_rows[s]:  # strict, float32; a NaN never wins
            best, took = p_rows[s], s
    return took, best


def vote_block(n_rows, seg_boxes, seg_ok, p_new, labels, mu, var):
    """One block.  seg_boxes [(b1, b2)] per segment in tester order, seg_ok [bool]; p_new / labels / mu / var are
    [n_seg, n_rows] (row j of segment s).  Returns None (nobody voted) or dict(box, votes, seg, second, prob, mu, var):
    ``seg`` the representative segment, ``second`` whether its voters carry label 1."""
    p_new = np.asarray(p_new, dtype=np.float32).reshape(len(seg_boxes), n_rows)
    voters = []  # (row, segment, label, box)
    for j in range(n_rows):
        s, _ = take(p_new[:, j], seg_ok)
        if s >= 0:
            lb = 1 if labels[s][j] != 0 else 0
            voters.append((j, s, lb, int(seg_boxes[s][lb])))
    if not voters:
        return None
    votes = {}
    for _, _, _, box in voters:
        votes[box] = votes.get(box, 0) + 1
    X, V = -1, 0
    for box in sorted(votes):  # ascending box index, strict >: the lowest box among equals
        if votes[box] > V:
            X, V = box, votes[box]
    per_seg = {}
    for _, s, _, box in voters:
        if box == X:
            per_seg[s] = per_seg.get(s, 0) + 1
    sf, nf = -1, 0
    for s in sorted(per_seg):  # tester order, strict >: the earliest among equals
        if per_seg[s] > nf:
            sf, nf = s, per_seg[s]
    vp = np.array([p_new[s, j] for j, s, _, _ in voters], dtype=np.float32)
    vm = np.array([mu[s][j] for j, s, _, _ in voters], dtype=np.float32)
    vv = np.array([var[s][j] for j, s, _, _ in voters], dtype=np.float32)
    kp, km, kv = _shift(vp, n_rows), _shift(vm, n_rows), _shift(vv, n_rows)
    for_x = np.array([box == X for _, _, _, box in voters])
    by_f = np.array([box == X and s == sf for _, s, _, box in voters])
    second = int(seg_boxes[sf][0]) != X
    return dict(box=X, votes=V, seg=sf, second=second, prob=_mean32(vp[for_x], kp, n_rows),
                mu=_mean32(vm[by_f], km, nf), var=_mean32(vv[by_f], kv, nf))
