"""ScanNet instance AP of pseudo-labels: the reference gapro/eval_ap_ps_labels.py with ISBNet's ScanNetEval
(isbnet/evaluation/instance_eval.py: assign_instances_for_scan :244-336, evaluate_matches :43-218, compute_averages
:220-242, print_results :433-485).

Mean instance IoU (eval_ps_labels) takes the best overlap per GT instance, so a spurious pseudo-instance or a duplicate
of a good one costs it nothing; AP counts both as false positives.  This is the metric of the reference's results table
for the networks trained on the labels.

``ap_tables`` runs the HIP kernels of gapro_amd/csrc/eval_ap.hip (gapro_eval_ap_keys / gapro_eval_ap_tables) over a
batch of scenes and returns per scene the integer tables assign_instances_for_scan builds from the masks: the GT
instances (code (class + 1) * 1000 + inst + 1 after the script's remap, :59-60, with their point counts), the pseudo
instances with a class (label of the first point + 1 in 1..18, :102-127) with their size, void points and confidence,
and the intersections of the same-class pairs.  ``ap_from_tables`` is evaluate_matches and compute_averages over any
number of such tables: AP does not decompose per batch, so the tables of all batches are reduced once, on the host.
``evaluate_ap`` is the two together.  There is no CPU path for the tables.

Probability thresholds: ``ap_tables_rows`` / ``evaluate_ap_rows`` return, beside the unfiltered row 0, one row per
threshold tau: the tables / the AP of the scene restricted, in all four label arrays, to the points with
ps_prob >= float32(tau) (the reference's certain_cond, eval_ps_labels.py:214-220, as eval_ps_labels applies it), and
the share of the points that are kept.  All rows come from the same pass over the points; ``table_from_raw`` (host
only) turns a row of the device arrays into its ApTable.

Confidence: the reference scores every pseudo-instance 1.0 (``"one"``), which makes the precision/recall curve a
single point.  ``"mean_prob"`` scores an instance by the mean per-point probability of gen_ps's label file, computed as
float64(S) / (float64(n) * 2**32) from the kernel's S = sum of rint(float64(prob) * 2**32): exact and independent of
the order of the points.

Not reproduced: the script's lines :65-96 overwrite a random 1/25 of the points with ps_uncertainty < 0.05 by their
GT labels (an unseeded np.random.choice, marked FIXME) and print two counts (:93).  That is an experiment on the
labels, not part of the metric.  The script does not run as released: it imports ``bs3dis``, which does not exist,
and passes start_iou / step_iou / threshold keywords that the ScanNetEval in the reference tree does not take; the
evaluator used here is that ScanNetEval, with its fixed IoU thresholds 0.50, 0.55, .., 0.90 and 0.25.

    python -m gapro_amd.eval_ap_ps_labels [--ps_folder DIR] [--data_root dataset/scannetv2] [--split train|val]
        [--stride 1] [--confidence one|mean_prob] [--min_region_size 100] [--batch_scenes 64] [--device cuda:0]
        [--prob_thresholds 0.6,0.8] [--json PATH]

prints print_results' table and the script's ``AP: x.xxx. AP_50: x.xxx. AP_25: x.xxx`` line, then with
--prob_thresholds one line per threshold (threshold, coverage, AP, AP_50, AP_25; in the JSON the list ``thresholds``).  The scene list,
the file reading and the exit status (0 / 3 / 2) are eval_ps_labels' (``python -m gapro_amd.eval_ps_labels``).
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._lib import Context
from .eval_ps_labels import (_FIELDS, _GT_CODES, _PS_CODES, CLASSES, _as_tensor, _cat, _common_dtype, _device_of,
                             _id_caps, _nan_to_none)

# ScanNetEval.ious: np.append(np.arange(0.5, 0.95, 0.05), 0.25)
IOU_THRESHOLDS = np.append(np.arange(0.5, 0.95, 0.05), 0.25)
N_CLASSES = len(CLASSES)
CONFIDENCE_MODES = ("one", "mean_prob")
_PROB_SCALE = float(2 ** 32)


class ApTable(NamedTuple):
    """One scene's tables.  GT instances in ascending code order; predictions in ascending pseudo id order; pairs
    sorted by (GT index, prediction index), same class, intersection > 0."""
    gt_code: np.ndarray     # int64 [G]: class * 1000 + inst + 1, class in 1..18
    gt_n: np.ndarray        # int64 [G]: points
    pred_id: np.ndarray     # int64 [P]: pseudo instance id
    pred_label: np.ndarray  # int64 [P]: label_id in 1..18
    pred_n: np.ndarray      # int64 [P]: points
    pred_void: np.ndarray   # int64 [P]: points that are in no GT instance
    pred_conf: np.ndarray   # float64 [P]
    pair_gt: np.ndarray     # int64 [Q]: index into the GT arrays
    pair_pred: np.ndarray   # int64 [Q]: index into the prediction arrays
    pair_inter: np.ndarray  # int64 [Q]: points in both


class ApResult(NamedTuple):
    avgs: dict           # compute_averages: all_ap, all_ap_50%, all_ap_25%, all_rc, all_rc_50%, all_rc_25%, classes
    ap: np.ndarray       # float64 [18, 10]: class x IoU threshold (IOU_THRESHOLDS), NaN for a class without GT
    rc: np.ndarray       # float64 [18, 10]
    n_gt: np.ndarray     # int64 [18]: GT instances of at least min_region_size points
    n_pred: np.ndarray   # int64 [18]: predictions of at least min_region_size points


def _mean_prob(s, n):
    return np.asarray(s, dtype=np.int64).astype(np.float64) / (np.asarray(n, dtype=np.int64).astype(np.float64)
                                                             * _PROB_SCALE)


class ApRows(NamedTuple):
    """Result of ``ap_tables_rows``; row 0 = all points, row j = the points with ps_prob >= prob_thresholds[j - 1]."""
    thresholds: tuple   # float32 values of the thresholds, in the caller's order
    tables: list        # [row][scene] ApTable: the tables of the row's points
    kept: np.ndarray    # int64 [scenes, rows]: points of the row


class ApRowsResult(NamedTuple):
    """Result of ``evaluate_ap_rows``, rows as in ApRows."""
    thresholds: tuple
    results: list         # [row] ApResult over all scenes
    kept: np.ndarray      # int64 [rows]: points of the row, summed over the scenes
    coverage: np.ndarray  # float64 [rows]: kept / kept[0] (NaN without a point)


def table_from_raw(key_code, key_n, ps_n, ps_label, ps_void, ps_sum, pair, confidence="one"):
    """One scene's row as the kernels leave it -> its ApTable (host only, NumPy).

    ``key_code`` / ``key_n`` [K]: the keys of the whole scene in ascending code order and their points in this row;
    ``ps_n`` / ``ps_label`` / ``ps_void`` / ``ps_sum`` [P]: per pseudo id the row's points, the label id (1..18, else 0)
    of its first point in the row, its void points and its sum of rint(prob * 2**32); ``pair`` [(K + 1) * (P + 1)]:
    points per (key + 1, id + 1), row 0 = void, column 0 = pseudo id -100.  A key without a point in the row is not a
    GT instance of the row and an id without a class there is no prediction: both are dropped and the pair indices
    count what is left."""
    codes = np.asarray(key_code, dtype=np.int64)
    key_n = np.asarray(key_n, dtype=np.int64)
    K, P = len(codes), len(ps_n)
    lab = np.asarray(ps_label, dtype=np.int64)
    keys = np.flatnonzero(key_n > 0)
    keep = np.flatnonzero(lab > 0)  # ids with points whose first point has a class in 1..18
    n = np.asarray(ps_n, dtype=np.int64)[keep]
    conf = _mean_prob(np.asarray(ps_sum)[keep], n) if confidence == "mean_prob" else np.ones(len(keep))
    codes = codes[keys]
    inter = np.asarray(pair).reshape(K + 1, P + 1)[1:, 1:][keys][:, keep].astype(np.int64)
    same = (codes // 1000)[:, None] == lab[keep][None, :]
    qg, qp = np.nonzero(same & (inter > 0))
    return ApTable(codes, key_n[keys], keep.astype(np.int64), lab[keep], n, np.asarray(ps_void, dtype=np.int64)[keep],
                   conf, qg.astype(np.int64), qp.astype(np.int64), inter[qg, qp])


def _thresholds(prob_thresholds):
    thr = np.asarray([float(t) for t in prob_thresholds], dtype=np.float32)
    if len(thr) > _lib.GAPRO_EVAL_MAX_THRESHOLDS:
        raise ValueError("at most %d probability thresholds" % _lib.GAPRO_EVAL_MAX_THRESHOLDS)
    if np.isnan(thr).any():
        raise ValueError("a probability threshold is NaN")
    return thr


def ap_tables_rows(scenes, prob_thresholds=(), confidence="one", scannet_remap=True, device=None):
    """The AP tables of a batch of scenes, unfiltered and for every probability threshold, in one set of launches (two
    kernel calls and one read of the key counts, one pass over the points).

    ``scenes``: as for eval_ps_labels.evaluate_scenes, mappings with the keys ``semantic_label``, ``instance_label``
    (GT: float64, int32 or int64), ``ps_semantic_label``, ``ps_instance_label`` (int32 or int64), ``ps_prob`` (float32
    per point; needed for ``confidence="mean_prob"`` and with thresholds) and optionally ``max_ps`` (pseudo id table
    size; by default max id + 1), or tuples in that order.  ``scannet_remap`` applies the script's GT remap (:59-60) on
    the device.  A threshold tau keeps the points with ps_prob >= float32(tau) in all four arrays, as
    evaluate_scenes' rows do; a row's tables are the tables of those points alone: a pseudo id takes the label of its
    first kept point, a GT instance without a kept point is not in the row, and mean_prob is over the kept points.
    Thresholds in any order, at most 32.  Returns ApRows.  Raises ValueError before anything runs for a NaN threshold,
    more than 32, or thresholds without ps_prob, and naming the scenes with an instance id >= 999, a pseudo id < 0
    other than -100 or beyond the table, or (with ps_prob in use) a probability that is NaN or outside [0, 1]."""
    if confidence not in CONFIDENCE_MODES:
        raise ValueError("confidence must be one of %s, not %r" % (CONFIDENCE_MODES, confidence))
    thr = _thresholds(prob_thresholds)
    T = len(thr)
    need_prob = confidence == "mean_prob" or T > 0
    cols = {f: [] for f in _FIELDS}
    caps = []
    for i, sc in enumerate(scenes):
        if not isinstance(sc, dict):
            sc = dict(zip(_FIELDS, sc))
        for f in _FIELDS[:4]:
            cols[f].append(_as_tensor(sc[f]))
        n = cols["semantic_label"][-1].numel()
        if any(cols[f][-1].numel() != n for f in _FIELDS[1:4]):
            raise ValueError("scene %d: the label arrays differ in length" % i)
        if need_prob:
            prob = sc.get("ps_prob")
            if prob is None:
                raise ValueError("scene %d: %s ps_prob" % (i, "probability thresholds need" if T else
                                                           "confidence='mean_prob' needs"))
            prob = _as_tensor(prob)
            if prob.numel() != n:
                raise ValueError("scene %d: ps_prob has %d entries for %d points" % (i, prob.numel(), n))
            cols["ps_prob"].append(prob)
        caps.append(sc.get("max_ps"))
    S = len(cols["semantic_label"])
    if S == 0:
        raise ValueError("ap_tables: no scene")
    dev = torch.device(device) if device is not None else _device_of(*[t for f in _FIELDS for t in cols[f]])
    if dev.type != "cuda":
        raise RuntimeError("gapro_amd.eval_ap_ps_labels needs a HIP device; there is no CPU fallback")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    gt_dt = _common_dtype(cols["semantic_label"] + cols["instance_label"], _GT_CODES, torch.int64)
    ps_dt = _common_dtype(cols["ps_semantic_label"] + cols["ps_instance_label"], _PS_CODES, torch.int64)
    ps_caps = _id_caps(cols["ps_instance_label"])
    descs = (_lib.EvalApScene * S)()
    off = 0
    for i, d in enumerate(descs):
        d.point_offset, d.n_points = off, cols["semantic_label"][i].numel()
        d.max_ps = int(caps[i]) if caps[i] is not None else ps_caps[i]
        off += d.n_points
    order = np.argsort(thr, kind="stable")
    h_thr = (C.c_float * T)(*[float(v) for v in thr[order]]) if T else None
    B = T + 1
    ctx = Context.get(dev.index)
    lib = ctx.lib
    ws_bytes = int(lib.gapro_eval_ap_workspace_bytes_rows(descs, S, T))
    if ws_bytes == 0:
        raise ValueError("bad pseudo id table sizes")
    n_ids = int(descs[S - 1].id_offset) + int(descs[S - 1].max_ps)
    stream = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)  # noqa: E731
    with torch.cuda.device(dev):
        sem, ins = (_cat(cols[f], gt_dt, dev) for f in _FIELDS[:2])
        ps_sem, ps_ins = (_cat(cols[f], ps_dt, dev) for f in _FIELDS[2:4])
        prob = _cat(cols["ps_prob"], torch.float32, dev) if need_prob else None
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        d_descs = torch.empty(C.sizeof(descs), dtype=torch.uint8, device=dev)
        n_keys = torch.empty(S, dtype=torch.int32, device=dev)
        status = torch.empty(S, dtype=torch.int32, device=dev)
        remap = 1 if scannet_remap else 0
        ctx.check(lib.gapro_eval_ap_keys(ctx.handle, stream(), S, descs, d_descs.data_ptr(), off, _GT_CODES[sem.dtype],
                                         sem.data_ptr(), _GT_CODES[ins.dtype], ins.data_ptr(), remap, ws.data_ptr(),
                                         ws_bytes, n_keys.data_ptr(), status.data_ptr()))
        for d, k in zip(descs, n_keys.cpu().tolist()):
            d.n_keys = k
        n_cells = int(lib.gapro_eval_ap_pair_cells(descs, S))
        n_key_rows = int(descs[S - 1].key_offset) + int(descs[S - 1].n_keys)
        i32 = lambda m: torch.empty(max(B * m, 1), dtype=torch.int32, device=dev)  # noqa: E731
        key_code, key_n = i32(n_key_rows), i32(n_key_rows)
        ps_n, ps_label, ps_void, pair = i32(n_ids), i32(n_ids), i32(n_ids), i32(n_cells)
        ps_sum = torch.empty(B * n_ids, dtype=torch.int64, device=dev)
        ctx.check(lib.gapro_eval_ap_tables_rows(
            ctx.handle, stream(), S, descs, d_descs.data_ptr(), off, _GT_CODES[sem.dtype], sem.data_ptr(),
            _GT_CODES[ins.dtype], ins.data_ptr(), _PS_CODES[ps_sem.dtype], ps_sem.data_ptr(), _PS_CODES[ps_ins.dtype],
            ps_ins.data_ptr(), None if prob is None else prob.data_ptr(), T, h_thr, remap, ws.data_ptr(), ws_bytes,
            key_code.data_ptr(), key_n.data_ptr(), ps_n.data_ptr(), ps_label.data_ptr(), ps_void.data_ptr(),
            ps_sum.data_ptr(), pair.data_ptr(), status.data_ptr()))
        host = [t.cpu().numpy() for t in (status, key_code, key_n, ps_n, ps_label, ps_void, ps_sum, pair)]
    status = host[0]
    bad = np.flatnonzero(status).tolist()
    if bad:
        raise ValueError("scene(s) %s: a GT instance id >= 999, a pseudo instance id < 0 other than -100 or beyond "
                         "the id table, or a probability that is NaN or outside [0, 1]" % bad)
    # [B, whole batch] each; kernel rows follow the ascending thresholds: the caller's row j + 1 is kernel row
    # 1 + rank of threshold j
    key_code, key_n = (a[:B * n_key_rows].reshape(B, n_key_rows) for a in host[1:3])
    ps_n, ps_label, ps_void, ps_sum = (a[:B * n_ids].reshape(B, n_ids) for a in host[3:7])
    pair = host[7][:B * n_cells].reshape(B, n_cells)
    perm = np.empty(B, dtype=np.int64)
    perm[0] = 0
    perm[1 + order] = 1 + np.arange(T)
    tables = [[] for _ in range(B)]
    kept = np.zeros((S, B), dtype=np.int64)
    for i, d in enumerate(descs):
        k0, K, i0, P, c0 = int(d.key_offset), int(d.n_keys), int(d.id_offset), int(d.max_ps), int(d.pair_offset)
        for j, r in enumerate(perm):
            cells = pair[r, c0:c0 + (K + 1) * (P + 1)]
            kept[i, j] = cells.sum(dtype=np.int64)  # every point of the row is in one pair cell
            tables[j].append(table_from_raw(key_code[r, k0:k0 + K], key_n[r, k0:k0 + K], ps_n[r, i0:i0 + P],
                                            ps_label[r, i0:i0 + P], ps_void[r, i0:i0 + P], ps_sum[r, i0:i0 + P], cells,
                                            confidence))
    return ApRows(tuple(float(v) for v in thr), tables, kept)


def ap_tables(scenes, confidence="one", scannet_remap=True, device=None):
    """The AP tables of a batch of scenes: ap_tables_rows without thresholds, its row 0.

    Returns one ApTable per scene.  Raises ValueError naming the scenes with an instance id >= 999, a pseudo id < 0
    other than -100 or beyond the table, or (mean_prob) a probability that is NaN or outside [0, 1]."""
    return ap_tables_rows(scenes, (), confidence, scannet_remap, device).tables[0]


def _curve(y_true, y_score, hard_false_negatives):
    """evaluate_matches' precision / recall curve and its integration (:154-204) -> (ap, rc)."""
    score_arg_sort = np.argsort(y_score)
    y_score_sorted = y_score[score_arg_sort]
    y_true_sorted = y_true[score_arg_sort]
    if len(y_true_sorted) == 0:
        return 0.0, 0.0
    y_true_sorted_cumsum = np.cumsum(y_true_sorted)
    (thresholds, unique_indices) = np.unique(y_score_sorted, return_index=True)
    num_prec_recall = len(unique_indices) + 1
    num_examples = len(y_score_sorted)
    num_true_examples = y_true_sorted_cumsum[-1]
    precision = np.zeros(num_prec_recall)
    recall = np.zeros(num_prec_recall)
    y_true_sorted_cumsum = np.append(y_true_sorted_cumsum, 0)
    # the reference's loop over the unique scores, elementwise (the same float64 operations)
    cumsum = y_true_sorted_cumsum[unique_indices - 1]
    tp = num_true_examples - cumsum
    fp = num_examples - unique_indices - tp
    fn = cumsum + hard_false_negatives
    precision[:-1] = tp / (tp + fp)
    recall[:-1] = tp / (tp + fn)
    rc_current = recall[0]
    precision[-1] = 1.0
    recall[-1] = 0.0
    recall_for_conv = np.copy(recall)
    recall_for_conv = np.append(recall_for_conv[0], recall_for_conv)
    recall_for_conv = np.append(recall_for_conv, 0.0)
    stepWidths = np.convolve(recall_for_conv, [-0.5, 0, 0.5], "valid")
    return np.dot(precision, stepWidths), rc_current


def _compute_averages(aps, rcs, ious=IOU_THRESHOLDS):
    """compute_averages (:220-242) on [1, classes, thresholds] arrays."""
    import warnings

    d_inf = 0
    o50 = np.where(np.isclose(ious, 0.5))
    o25 = np.where(np.isclose(ious, 0.25))
    oAllBut25 = np.where(np.logical_not(np.isclose(ious, 0.25)))
    avg_dict = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)  # nanmean of all-NaN: NaN, as the reference
        avg_dict["all_ap"] = np.nanmean(aps[d_inf, :, oAllBut25])
        avg_dict["all_ap_50%"] = np.nanmean(aps[d_inf, :, o50])
        avg_dict["all_ap_25%"] = np.nanmean(aps[d_inf, :, o25])
        avg_dict["all_rc"] = np.nanmean(rcs[d_inf, :, oAllBut25])
        avg_dict["all_rc_50%"] = np.nanmean(rcs[d_inf, :, o50])
        avg_dict["all_rc_25%"] = np.nanmean(rcs[d_inf, :, o25])
    avg_dict["classes"] = {}
    for (li, label_name) in enumerate(CLASSES):
        avg_dict["classes"][label_name] = {}
        avg_dict["classes"][label_name]["ap"] = np.average(aps[d_inf, li, oAllBut25])
        avg_dict["classes"][label_name]["ap50%"] = np.average(aps[d_inf, li, o50])
        avg_dict["classes"][label_name]["ap25%"] = np.average(aps[d_inf, li, o25])
        avg_dict["classes"][label_name]["rc"] = np.average(rcs[d_inf, li, oAllBut25])
        avg_dict["classes"][label_name]["rc50%"] = np.average(rcs[d_inf, li, o50])
        avg_dict["classes"][label_name]["rc25%"] = np.average(rcs[d_inf, li, o25])
    return avg_dict


def _greedy(gts, preds, confs):
    """evaluate_matches' greedy assignment (:88-121) over the pairs with IoU > th of GT instances that count, in
    (scene, GT code, pseudo id) order -> (matched GT -> score, false positives' (GT, score))."""
    visited, score, dups = set(), {}, []
    for g, p, c in zip(gts.tolist(), preds.tolist(), confs.tolist()):
        if p in visited:
            continue
        if g in score:
            dups.append((g, min(score[g], c)))
            score[g] = max(score[g], c)
        else:
            score[g] = c
            visited.add(p)
    return score, dups


def ap_from_tables(tables, min_region_size=100):
    """evaluate_matches and compute_averages over the ApTables of any number of scenes (host only) -> ApResult.

    GT instances and predictions of fewer than ``min_region_size`` points do not count (assign_instances_for_scan
    :296-298, evaluate_matches :77); a prediction without a match is a false positive unless its void points plus its
    intersections with same-class GT instances under that size are more than the threshold's share of it (:124-145).
    The result does not depend on the order of the tables."""
    mrs = int(min_region_size)
    tables = list(tables)
    cat = lambda f: np.concatenate([np.asarray(getattr(t, f)) for t in tables]) if tables else np.zeros(0)  # noqa: E731
    g_off = np.cumsum([0] + [len(t.gt_code) for t in tables])
    p_off = np.cumsum([0] + [len(t.pred_id) for t in tables])
    gt_cls = cat("gt_code").astype(np.int64) // 1000
    gt_n = cat("gt_n").astype(np.int64)
    pr_cls = cat("pred_label").astype(np.int64)
    pr_n = cat("pred_n").astype(np.int64)
    pr_void = cat("pred_void").astype(np.int64)
    pr_conf = cat("pred_conf").astype(np.float64)
    q_gt = np.concatenate([np.asarray(t.pair_gt, np.int64) + g_off[i] for i, t in enumerate(tables)]) if tables \
        else np.zeros(0, np.int64)
    q_pr = np.concatenate([np.asarray(t.pair_pred, np.int64) + p_off[i] for i, t in enumerate(tables)]) if tables \
        else np.zeros(0, np.int64)
    q_inter = cat("pair_inter").astype(np.int64)
    gt_ok = gt_n >= mrs
    pr_ok = pr_n >= mrs
    keep = pr_ok[q_pr]  # pairs of the predictions that count, in (GT, prediction) order
    q_gt, q_pr, q_inter = q_gt[keep], q_pr[keep], q_inter[keep]
    iou = q_inter.astype(np.float64) / (gt_n[q_gt] + pr_n[q_pr] - q_inter).astype(np.float64)  # :325
    # unmatched predictions: the best IoU over all same-class GT instances, and the ignored share (:124-145)
    best = np.full(len(pr_n), -np.inf)
    np.maximum.at(best, q_pr, iou)
    small = ~gt_ok[q_gt]
    ignore = pr_void + np.bincount(q_pr[small], weights=q_inter[small], minlength=len(pr_n)).astype(np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        prop_ignore = ignore.astype(np.float64) / pr_n.astype(np.float64)
    n_gt = np.bincount(gt_cls[gt_ok] - 1, minlength=N_CLASSES)[:N_CLASSES].astype(np.int64)
    n_pred = np.bincount(pr_cls[pr_ok] - 1, minlength=N_CLASSES)[:N_CLASSES].astype(np.int64)
    ap = np.zeros((1, N_CLASSES, len(IOU_THRESHOLDS)), np.float64)
    rc = np.zeros((1, N_CLASSES, len(IOU_THRESHOLDS)), np.float64)
    for oi, th in enumerate(IOU_THRESHOLDS):
        m = gt_ok[q_gt] & (iou > th)
        mg, mp = q_gt[m], q_pr[m]
        if len(np.unique(mg)) == len(mg) and len(np.unique(mp)) == len(mp):  # one-to-one: every pair is a match
            tp_gt, tp_score = mg, pr_conf[mp]
            fp_cls, fp_score = np.zeros(0, np.int64), np.zeros(0)
        else:
            score, dups = _greedy(mg, mp, pr_conf[mp])
            tp_gt = np.fromiter(score.keys(), np.int64, len(score))
            tp_score = np.fromiter(score.values(), np.float64, len(score))
            fp_cls = gt_cls[np.asarray([g for g, _ in dups], np.int64)]
            fp_score = np.asarray([s for _, s in dups], np.float64)
        matched = np.zeros(len(gt_n), bool)
        matched[tp_gt] = True
        hard_fn = np.bincount(gt_cls[gt_ok & ~matched] - 1, minlength=N_CLASSES)
        lone = pr_ok & ~(best > th) & (prop_ignore <= th)
        cls_all = np.concatenate([gt_cls[tp_gt], fp_cls, pr_cls[lone]])
        true_all = np.concatenate([np.ones(len(tp_gt)), np.zeros(len(fp_cls) + int(lone.sum()))])
        score_all = np.concatenate([tp_score, fp_score, pr_conf[lone]])
        for li in range(N_CLASSES):
            if n_gt[li] and n_pred[li]:
                sel = cls_all == li + 1
                ap[0, li, oi], rc[0, li, oi] = _curve(true_all[sel], score_all[sel], int(hard_fn[li]))
            elif n_gt[li]:
                ap[0, li, oi] = rc[0, li, oi] = 0.0
            else:
                ap[0, li, oi] = rc[0, li, oi] = float("nan")
    return ApResult(_compute_averages(ap, rc), ap[0], rc[0], n_gt, n_pred)


def evaluate_ap(scenes, confidence="one", scannet_remap=True, min_region_size=100, device=None):
    """ap_from_tables(ap_tables(scenes, ...)) -> ApResult."""
    return ap_from_tables(ap_tables(scenes, confidence, scannet_remap, device), min_region_size)


def ap_from_tables_rows(tables, kept, min_region_size=100):
    """ap_from_tables per row of ap_tables_rows' tables ([row][scene], of any number of batches) and the coverage from
    ``kept`` (int64 [scenes, rows] or already summed [rows]) -> (list of ApResult, kept [rows], coverage [rows])."""
    kept = np.asarray(kept, dtype=np.int64)
    kept = kept.sum(axis=0) if kept.ndim == 2 else kept
    with np.errstate(invalid="ignore", divide="ignore"):
        coverage = kept.astype(np.float64) / np.float64(kept[0])
    return [ap_from_tables(t, min_region_size) for t in tables], kept, coverage


def evaluate_ap_rows(scenes, prob_thresholds=(), confidence="one", scannet_remap=True, min_region_size=100,
                     device=None):
    """ap_from_tables of every row of ap_tables_rows(scenes, prob_thresholds, ...) -> ApRowsResult: the AP of the
    points the generator is at least that sure about, and the share of the points they are."""
    rows = ap_tables_rows(scenes, prob_thresholds, confidence, scannet_remap, device)
    return ApRowsResult(rows.thresholds, *ap_from_tables_rows(rows.tables, rows.kept, min_region_size))


def format_results(avgs):
    """print_results (:433-485): the 64-column table, class rows and the average row."""
    sep, col1, lineLen = "", ":", 64
    lines = ["", "#" * lineLen]
    line = "{:<15}".format("what") + sep + col1
    for h in ("AP", "AP_50%", "AP_25%", "AR", "RC_50%", "RC_25%"):
        line += "{:>8}".format(h) + sep
    lines += [line, "#" * lineLen]
    for label_name in CLASSES:
        c = avgs["classes"][label_name]
        line = "{:<15}".format(label_name) + sep + col1
        for k in ("ap", "ap50%", "ap25%", "rc", "rc50%", "rc25%"):
            line += sep + "{:>8.3f}".format(c[k]) + sep
        lines.append(line)
    lines.append("-" * lineLen)
    line = "{:<15}".format("average") + sep + col1
    for k in ("all_ap", "all_ap_50%", "all_ap_25%", "all_rc", "all_rc_50%", "all_rc_25%"):
        line += "{:>8.3f}".format(avgs[k]) + sep
    lines += [line, "#" * lineLen, ""]
    return "\n".join(lines)


def _json_avgs(avgs):
    out = {k: _nan_to_none(v) for k, v in avgs.items() if k != "classes"}
    out["classes"] = {c: {k: _nan_to_none(v) for k, v in d.items()} for c, d in avgs["classes"].items()}
    return out


def main(argv=None):
    import argparse
    import json
    import os.path as osp
    import sys
    import time

    from .eval_ps_labels import list_scenes, read_scene_batches

    parser = argparse.ArgumentParser("GaPro_EvalApPsLabels")
    parser.add_argument("--ps_folder", type=str, default="dataset/scannetv2/gaussian_process_kl_pseudo_labels")
    parser.add_argument("--data_root", type=str, default="dataset/scannetv2")
    parser.add_argument("--split", type=str, default="train", choices=["train", "val"])
    parser.add_argument("--stride", type=int, default=1)
    parser.add_argument("--confidence", type=str, default="one", choices=list(CONFIDENCE_MODES))
    parser.add_argument("--min_region_size", type=int, default=100)
    parser.add_argument("--prob_thresholds", type=str, default="")
    parser.add_argument("--batch_scenes", type=int, default=64)
    parser.add_argument("--device", type=str, default=None)
    parser.add_argument("--json", type=str, default=None)
    args = parser.parse_args(argv)
    t0 = time.perf_counter()
    try:
        taus = [float(v) for v in args.prob_thresholds.split(",") if v.strip()]
        _thresholds(taus)
    except ValueError as e:
        parser.error("--prob_thresholds: %s" % e)
    scanned = list_scenes(args.data_root, args.split, args.stride)
    present = [s for s in scanned if osp.exists(osp.join(args.ps_folder, s + ".pth"))]
    have = set(present)
    missing = [s for s in scanned if s not in have]
    need_prob = args.confidence == "mean_prob" or bool(taus)
    tables, evaluated, failed = [[] for _ in range(len(taus) + 1)], [], {}
    kept = np.zeros(len(taus) + 1, dtype=np.int64)
    t_eval = 0.0  # upload, kernels, download: the rest of the run is reading and the host reduction
    for names, scenes in read_scene_batches(args, present, need_prob, failed,
                                            "--confidence mean_prob" if args.confidence == "mean_prob"
                                            else "--prob_thresholds"):
        t1 = time.perf_counter()
        rows = ap_tables_rows(scenes, taus, args.confidence, scannet_remap=True, device=args.device)
        t_eval += time.perf_counter() - t1
        for r, per_scene in enumerate(rows.tables):
            tables[r] += per_scene
        kept += rows.kept.sum(axis=0)
        evaluated += names
    t1 = time.perf_counter()
    row_res, _, coverage = ap_from_tables_rows(tables, kept, args.min_region_size) if evaluated else ([None], kept, None)
    res = row_res[0]
    t_ap = time.perf_counter() - t1
    elapsed = time.perf_counter() - t0

    out = dict(data_root=args.data_root, split=args.split, ps_folder=args.ps_folder, stride=args.stride,
               confidence=args.confidence, min_region_size=args.min_region_size, scanned=scanned, evaluated=evaluated,
               missing=missing, failed=failed)
    if res is not None:
        avgs = res.avgs
        print(format_results(avgs))
        print("AP: {:.3f}. AP_50: {:.3f}. AP_25: {:.3f}".format(avgs["all_ap"], avgs["all_ap_50%"],
                                                                 avgs["all_ap_25%"]))
        out.update(avgs=_json_avgs(avgs), n_gt=dict(zip(CLASSES, res.n_gt.tolist())),
                   n_pred=dict(zip(CLASSES, res.n_pred.tolist())))
        if taus:
            print("%-10s %10s %8s %8s %8s" % ("prob >=", "coverage", "AP", "AP_50", "AP_25"))
            out["thresholds"] = []
        for j, tau in enumerate(taus):
            r = row_res[j + 1]
            a = r.avgs
            print("%-10g %10.4f %8.3f %8.3f %8.3f" % (tau, coverage[j + 1], a["all_ap"], a["all_ap_50%"],
                                                        a["all_ap_25%"]))
            out["thresholds"].append(dict(threshold=tau, kept_points=int(kept[j + 1]),
                                          coverage=_nan_to_none(coverage[j + 1]), avgs=_json_avgs(a),
                                          n_gt=dict(zip(CLASSES, r.n_gt.tolist())),
                                          n_pred=dict(zip(CLASSES, r.n_pred.tolist()))))
    print("[eval_ap_ps_labels] %d scene(s) listed, %d evaluated, %d without a label file, %d failed in %.2f s"
          % (len(scanned), len(evaluated), len(missing), len(failed), elapsed), file=sys.stderr)
    if failed:
        print("[eval_ap_ps_labels] %d scene(s) could not be evaluated: %s" % (len(failed), " ".join(sorted(failed))),
              file=sys.stderr)
        for name in sorted(failed):
            print("  %s: %s" % (name, failed[name]), file=sys.stderr)
    out.update(elapsed_s=elapsed, eval_s=t_eval, ap_s=t_ap,
               scenes_per_s=(len(evaluated) / elapsed if elapsed > 0 else None))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)
    if not evaluated:
        print("[eval_ap_ps_labels] nothing was evaluated", file=sys.stderr)
        return 2
    return 3 if failed else 0


if __name__ == "__main__":
    import sys

    sys.exit(main())
