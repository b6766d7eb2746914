"""Pseudo-label quality metrics on the GPU: mirror of reference gapro/eval_ps_labels.py:35-42,100-172 and its main().

SURVEY.md section 8(f) row 1 ("next"): not part of the generator's hot path; wired to ``gen_ps --eval_pslabel``.
Same call signatures as the reference (which runs them on ``.cuda()`` tensors); the work is done by the HIP
kernels of gapro_amd/csrc/eval_batch.hip behind ``gapro_eval_batch``, called for a batch of one scene: one
histogram pass over the points instead of two [I, N] one-hot matrices and their product.  There is no CPU path:
inputs are moved to the device, and without a HIP device the call raises.

``evaluate_scenes`` is the batched form: a batch of scenes in their file dtypes, the unfiltered metrics plus any
number of ``ps_prob >= tau`` filters (the reference's commented-out certain_cond study, :214-220), bit-identical to
the two per-scene functions on the filtered arrays.
``python -m gapro_amd.eval_ps_labels`` is the reference's stand-alone evaluation of a folder of pseudo-labels
(main(), :175-257) on top of it:

    python -m gapro_amd.eval_ps_labels [--ps_folder DIR] [--data_root dataset/scannetv2] [--split train|val]
        [--stride 10] [--prob_thresholds 0.6,0.8] [--batch_scenes 64] [--device cuda:0] [--json PATH]

Every --stride-th scene of the sorted split (taken before the scenes without a label file are skipped, as the
reference does) is read by up to 16 threads and evaluated in batches; the run prints the reference's
``mean inst iou`` / ``sem iou`` / ``sem miou`` lines, a per-class table and, with thresholds, one row per threshold
(coverage = kept / all points, mean instance IoU, semantic mIoU).  Exit status: 0 = every listed scene that has a
label file was evaluated, 3 = some could not be read (named on stderr), 2 = nothing was evaluated.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._lib import Context

_GT_CODES = {torch.float64: _lib.GAPRO_LABEL_F64, torch.int32: _lib.GAPRO_LABEL_I32, torch.int64: _lib.GAPRO_LABEL_I64}
_PS_CODES = {torch.int32: _lib.GAPRO_LABEL_I32, torch.int64: _lib.GAPRO_LABEL_I64}


def _as_tensor(a):
    if isinstance(a, torch.Tensor):
        return a.reshape(-1)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a)).reshape(-1))


def _dev_labels(a, device, codes):
    """The labels on the device, in their own dtype when the kernels have a code for it, else as int64."""
    t = _as_tensor(a)
    return t.to(device=device, dtype=t.dtype if t.dtype in codes else torch.int64).contiguous()


def _device_of(*tensors):
    for t in tensors:
        if isinstance(t, torch.Tensor) and t.is_cuda:
            return t.device
    if not torch.cuda.is_available():
        raise RuntimeError("gapro_amd.eval_ps_labels needs a HIP device; there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def get_miou_scene(semantic_label, instance_label, ps_semantic_label, ps_instance_label):
    """Per GT instance: max IoU over pseudo instances of the same class (eval_ps_labels.py:100-147).

    IoU = inter / (|gt| + |ps| - inter + 1e-4), float32 as in ``cal_iou`` (:35-42).  Returns a float32 device
    tensor with one entry per non-empty GT instance id, in id order."""
    dev = _device_of(semantic_label, instance_label, ps_semantic_label, ps_instance_label)
    sem, ins = (_dev_labels(a, dev, _GT_CODES) for a in (semantic_label, instance_label))
    ps_sem, ps_ins = (_dev_labels(a, dev, _PS_CODES) for a in (ps_semantic_label, ps_instance_label))
    n = int(ins.numel())
    if n == 0:
        return torch.zeros(0, device=dev)
    _, max_iou, gt_cls, _, _ = _eval_batch(dev, [(n, *_id_caps([ins, ps_ins]))], sem, ins, ps_sem, ps_ins)
    return max_iou[gt_cls >= 0]


def get_scene_sem_conf(semantic_label, ps_semantic_label, num_classes=19):
    """Semantic confusion matrix i64[C, C] (eval_ps_labels.py:150-172); the inputs are not modified."""
    dev = _device_of(semantic_label, ps_semantic_label)
    sem, ps_sem = _dev_labels(semantic_label, dev, _GT_CODES), _dev_labels(ps_semantic_label, dev, _PS_CODES)
    n = int(sem.numel())
    if n == 0:
        return torch.zeros((num_classes, num_classes), dtype=torch.int64, device=dev)
    return _eval_batch(dev, [(n, 1, 1)], sem, None, ps_sem, None, num_classes=num_classes)[3][0]


# ---------------------------------------------------------------------------------------------------------------------
# Batched evaluation (gapro_eval_batch) and the stand-alone evaluator (reference main(), :175-257)
# ---------------------------------------------------------------------------------------------------------------------
CLASSES = ("cabinet", "bed", "chair", "sofa", "table", "door", "window", "bookshelf", "picture", "counter", "desk",
           "curtain", "refrigerator", "shower curtain", "toilet", "sink", "bathtub", "otherfurniture")  # :8-27
# class 18 after the GT remap (:196-197) holds the ScanNet classes 0 and 1
CLASS_18 = "wall/floor"

_FIELDS = ("semantic_label", "instance_label", "ps_semantic_label", "ps_instance_label", "ps_prob")


class BatchEval(NamedTuple):
    """Result of ``evaluate_scenes``; row 0 = all points, row j = the points with ps_prob >= prob_thresholds[j - 1]."""
    thresholds: tuple   # float32 values of the thresholds, in the caller's order
    ious: list          # [scene][row] float32 NumPy array: get_miou_scene of the row's points
    conf: np.ndarray    # int64 [rows, C, C]: get_scene_sem_conf of the row's points, summed over the scenes
    kept: np.ndarray    # int64 [scenes, rows]: points of the row


def _common_dtype(ts, allowed, promote):
    dts = {t.dtype for t in ts}
    if len(dts) == 1 and next(iter(dts)) in allowed:
        return next(iter(dts))
    if all(d in allowed for d in dts) or not any(d.is_floating_point for d in dts):
        return promote
    return torch.float64 if torch.float64 in allowed else torch.int64


def _cat(ts, dtype, dev):
    if not ts:
        return torch.empty(0, dtype=dtype, device=dev)
    if all(not t.is_cuda for t in ts):
        return torch.cat([t.to(dtype) for t in ts]).to(dev)
    return torch.cat([t.to(device=dev, dtype=dtype) for t in ts])


def _id_caps(ts):
    """max id + 1 per scene (>= 1): the id-table sizes, from host arrays without a device round trip."""
    caps = [1] * len(ts)
    dev_idx = [i for i, t in enumerate(ts) if t.numel() and t.is_cuda]
    for i, t in enumerate(ts):
        if t.numel() and not t.is_cuda:
            caps[i] = max(1, int(t.max()) + 1)
    if dev_idx:
        m = torch.stack([ts[i].max().to(torch.float64) for i in dev_idx]).cpu().tolist()
        for i, v in zip(dev_idx, m):
            caps[i] = max(1, int(v) + 1)
    return caps


def _eval_batch(dev, sizes, sem, ins, ps_sem, ps_ins, prob=None, thresholds=(), scannet_remap=False, num_classes=19):
    """gapro_eval_batch on label arrays already concatenated on ``dev``, each in a dtype it has a code for.

    ``sizes``: (n_points, max_gt, max_ps) per scene, in array order; ``thresholds``: ascending float32 values, with
    ``prob`` one per point.  ``ins`` and ``ps_ins`` None: the confusion matrix and the counts only, enqueued without a
    host sync.  -> (descriptors, max_iou, gt_cls, conf, kept), device tensors (max_iou / gt_cls None without instance
    arrays).  Raises ValueError for a scene with an instance id beyond its id table."""
    S, K = len(sizes), len(thresholds)
    descs = (_lib.EvalScene * S)()
    off = 0
    for d, (n, max_gt, max_ps) in zip(descs, sizes):
        d.point_offset, d.n_points, d.max_gt, d.max_ps = off, n, max_gt, max_ps
        off += n
    ctx = Context.get(dev.index)
    lib = ctx.lib
    ws_bytes = int(lib.gapro_eval_batch_workspace_bytes(descs, S, K))
    if ws_bytes == 0:
        raise ValueError("bad id-table sizes")
    B, pairs = K + 1, ins is not None
    rows = int(descs[S - 1].row_offset) + B * int(descs[S - 1].max_gt)
    h_thr = (C.c_float * K)(*[float(v) for v in thresholds]) if K else None
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    with torch.cuda.device(dev):
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        max_iou = torch.empty(rows, dtype=torch.float32, device=dev) if pairs else None
        gt_cls = torch.empty(rows, dtype=torch.float32, device=dev) if pairs else None
        conf = torch.empty((B, num_classes, num_classes), dtype=torch.int64, device=dev)
        kept = torch.empty((S, B), dtype=torch.int64, device=dev)
        status = torch.empty(S, dtype=torch.int32, device=dev)
        d_descs = torch.empty(C.sizeof(descs), dtype=torch.uint8, device=dev)
        ctx.check(lib.gapro_eval_batch(
            ctx.handle, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), S, descs, d_descs.data_ptr(), off,
            _GT_CODES[sem.dtype], sem.data_ptr(), _GT_CODES[ins.dtype] if pairs else 0, ptr(ins),
            _PS_CODES[ps_sem.dtype], ps_sem.data_ptr(), _PS_CODES[ps_ins.dtype] if pairs else 0, ptr(ps_ins),
            ptr(prob), K, h_thr, 1 if scannet_remap else 0, int(num_classes), ws.data_ptr(), ws_bytes, ptr(max_iou),
            ptr(gt_cls), conf.data_ptr(), kept.data_ptr(), status.data_ptr()))
        bad = torch.nonzero(status).flatten().tolist() if pairs else []
    if bad:
        raise ValueError("scene(s) %s hold an instance id beyond the id table" % bad)
    return descs, max_iou, gt_cls, conf, kept


def evaluate_scenes(scenes, prob_thresholds=(), scannet_remap=True, num_classes=19, device=None):
    """get_miou_scene and get_scene_sem_conf of a batch of scenes, unfiltered and for every probability threshold, in
    one set of launches.

    ``scenes``: a sequence of mappings with the keys ``semantic_label``, ``instance_label`` (GT: float64 as the ScanNet
    files hold them, int32 or int64), ``ps_semantic_label``, ``ps_instance_label`` (int32 as gen_ps writes them, or
    int64), ``ps_prob`` (float32 per point; needed with thresholds) and optionally ``max_gt`` / ``max_ps`` (id-table
    sizes; by default max id + 1), or tuples in that order.  NumPy arrays or tensors; nothing is modified.
    ``scannet_remap`` applies the reference main()'s GT remap (:196-197) on the device.  A threshold tau keeps the
    points with ps_prob >= float32(tau) in all four arrays.  Every row is bit-identical to the per-scene functions on
    the row's points.  Raises ValueError for a scene with an instance id beyond its id table."""
    thr = np.asarray([float(t) for t in prob_thresholds], dtype=np.float32)
    K = len(thr)
    if K > _lib.GAPRO_EVAL_MAX_THRESHOLDS:
        raise ValueError("at most %d probability thresholds" % _lib.GAPRO_EVAL_MAX_THRESHOLDS)
    if np.isnan(thr).any():
        raise ValueError("a probability threshold is NaN")
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
        prob = sc.get("ps_prob")
        if K:
            if prob is None:
                raise ValueError("scene %d: probability thresholds need ps_prob" % i)
            prob = _as_tensor(prob)
            if prob.numel() != n:
                raise ValueError("scene %d: ps_prob has %d entries for %d points" % (i, prob.numel(), n))
            cols["ps_prob"].append(prob)
        caps.append((sc.get("max_gt"), sc.get("max_ps")))
    S = len(cols["semantic_label"])
    if S == 0:
        raise ValueError("evaluate_scenes: no scene")
    dev = torch.device(device) if device is not None else _device_of(*[t for f in _FIELDS for t in cols[f]])
    if dev.type != "cuda":
        raise RuntimeError("gapro_amd.eval_ps_labels needs a HIP device; there is no CPU fallback")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    gt_dt = _common_dtype(cols["semantic_label"] + cols["instance_label"], _GT_CODES, torch.int64)
    ps_dt = _common_dtype(cols["ps_semantic_label"] + cols["ps_instance_label"], _PS_CODES, torch.int64)
    gt_caps, ps_caps = _id_caps(cols["instance_label"]), _id_caps(cols["ps_instance_label"])
    sizes = [(cols["semantic_label"][i].numel(), int(caps[i][0]) if caps[i][0] is not None else gt_caps[i],
              int(caps[i][1]) if caps[i][1] is not None else ps_caps[i]) for i in range(S)]
    order = np.argsort(thr, kind="stable")
    with torch.cuda.device(dev):
        sem, ins = (_cat(cols[f], gt_dt, dev) for f in _FIELDS[:2])
        ps_sem, ps_ins = (_cat(cols[f], ps_dt, dev) for f in _FIELDS[2:4])
        prob = _cat(cols["ps_prob"], torch.float32, dev) if K else None
    descs, max_iou, gt_cls, conf, kept = _eval_batch(dev, sizes, sem, ins, ps_sem, ps_ins, prob, thr[order],
                                                     scannet_remap, num_classes)
    max_iou, gt_cls, conf, kept = (t.cpu().numpy() for t in (max_iou, gt_cls, conf, kept))
    B = K + 1
    # kernel rows follow the ascending thresholds; the caller's row j + 1 is kernel row 1 + rank of threshold j
    perm = np.empty(B, dtype=np.int64)
    perm[0] = 0
    perm[1 + order] = 1 + np.arange(K)
    ious = []
    for i in range(S):
        g = int(descs[i].max_gt)
        per_row = []
        for r in perm:
            a = int(descs[i].row_offset) + int(r) * g
            per_row.append(max_iou[a:a + g][gt_cls[a:a + g] >= 0])
        ious.append(per_row)
    return BatchEval(tuple(float(v) for v in thr), ious, conf[perm], kept[:, perm])


def list_scenes(data_root, split="train", stride=10):
    """The reference's scene list (:176-179): the sorted scene names of the split, every stride-th one.  The stride
    is applied before the scenes without a label file are skipped (:199-200)."""
    import glob
    import os.path as osp

    names = sorted(osp.basename(f)[:12] for f in glob.glob(osp.join(data_root, split, "*_inst_nostuff.pth")))
    return names[::max(int(stride), 1)]


def _load_tuple(path):
    from . import pth_io

    got = pth_io.load_arrays(path) if pth_io.native_enabled() else None
    if got is None:
        obj = torch.load(path, weights_only=False)
        obj = obj if isinstance(obj, (tuple, list)) else (obj,)
        return [o.numpy() if isinstance(o, torch.Tensor) else np.asarray(o) for o in obj]
    return got[0]


def read_gt_labels(path):
    """(semantic, instance) of a ScanNet *_inst_nostuff.pth file (xyz, rgb, sem, inst), in the file's dtype."""
    arrs = _load_tuple(path)
    if len(arrs) < 4:
        raise ValueError("%s: expected (xyz, rgb, semantic, instance), found %d arrays" % (path, len(arrs)))
    return arrs[2].reshape(-1), arrs[3].reshape(-1)


def read_label_file(path, need_prob=False, what="--prob_thresholds"):
    """(semantic, instance, prob or None) of a pseudo-label file: [0] = semantic, [1] = instance; [2] is the per-point
    probability only when it has one entry per point (gen_ps's 5-tuple; the reference's 2-tuple has none, and an array
    of superpoint length is not a per-point probability).  need_prob: a file without one is an error (naming ``what``
    needs it)."""
    arrs = _load_tuple(path)
    if len(arrs) < 2:
        raise ValueError("%s: expected (semantic, instance, ...), found %d array(s)" % (path, len(arrs)))
    sem, inst = arrs[0].reshape(-1), arrs[1].reshape(-1)
    if len(inst) != len(sem):
        raise ValueError("%s: %d semantic and %d instance labels" % (path, len(sem), len(inst)))
    prob = None
    if len(arrs) > 2 and arrs[2].ndim == 1 and len(arrs[2]) == len(sem) and arrs[2].dtype.kind == "f":
        prob = arrs[2].astype(np.float32, copy=False)
    if need_prob and prob is None:
        raise ValueError("%s: no per-point probability for %s" % (path, what))
    return sem, inst, prob


def sem_iou_from_conf(conf):
    """The reference main()'s reduction of the summed confusion (:243-252): per-class IoU * 100 (float32, NaN for a
    class absent from both sides) and their nanmean.  -> (iou f32[C] NumPy, miou float)."""
    conf_metric = torch.as_tensor(np.asarray(conf), dtype=torch.int64)
    true_positive = torch.diag(conf_metric)
    false_positive = torch.sum(conf_metric, 0) - true_positive
    false_negative = torch.sum(conf_metric, 1) - true_positive
    iou = true_positive / (true_positive + false_positive + false_negative)
    iou = iou * 100
    miou = torch.nanmean(iou)
    return iou.numpy(), float(miou)


def _read_scene(args, name, need_prob, what="--prob_thresholds"):
    import os.path as osp

    sem, inst = read_gt_labels(osp.join(args.data_root, args.split, name + "_inst_nostuff.pth"))
    ps_sem, ps_inst, prob = read_label_file(osp.join(args.ps_folder, name + ".pth"), need_prob, what)
    if len(ps_sem) != len(sem):
        raise ValueError("%d pseudo labels for %d points" % (len(ps_sem), len(sem)))
    return dict(semantic_label=sem, instance_label=inst, ps_semantic_label=ps_sem, ps_instance_label=ps_inst,
                ps_prob=prob)


def read_scene_batches(args, present, need_prob, failed, what="--prob_thresholds"):
    """Yields (names, scenes) per batch of ``args.batch_scenes`` of the scenes ``present`` (GT under
    ``args.data_root`` / ``args.split``, labels in ``args.ps_folder``), read by up to 16 threads one batch ahead.  A
    scene that cannot be read goes to ``failed[name]`` with the reason; a batch left empty is skipped."""
    import concurrent.futures as cf
    import os

    n_threads = max(1, min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 16))
    batch = max(1, int(args.batch_scenes))
    chunks = [present[i:i + batch] for i in range(0, len(present), batch)]
    with cf.ThreadPoolExecutor(max_workers=n_threads) as pool:
        submit = lambda names: [(n, pool.submit(_read_scene, args, n, need_prob, what)) for n in names]  # noqa: E731
        pending = submit(chunks[0]) if chunks else []
        for ci in range(len(chunks)):
            cur, pending = pending, (submit(chunks[ci + 1]) if ci + 1 < len(chunks) else [])  # read one batch ahead
            names, scenes = [], []
            for name, fut in cur:
                try:
                    scenes.append(fut.result())
                    names.append(name)
                except Exception as e:  # noqa: BLE001 - a damaged / unreadable scene is reported, the others go on
                    failed[name] = "%s: %s" % (type(e).__name__, e)
            if scenes:
                yield names, scenes


def _nan_to_none(v):
    return None if v is None or v != v else float(v)


def main(argv=None):
    import argparse
    import json
    import os.path as osp
    import sys
    import time

    from .gen_ps import mean_instance_iou

    parser = argparse.ArgumentParser("GaPro_EvalPsLabels")
    parser.add_argument("--ps_folder", type=str, default="dataset/scannetv2/gaussian_process_kl_pseudo_labels")
    parser.add_argument("--data_root", type=str, default="dataset/scannetv2")
    parser.add_argument("--split", type=str, default="train", choices=["train", "val"])
    parser.add_argument("--stride", type=int, default=10)
    parser.add_argument("--prob_thresholds", type=str, default="")
    parser.add_argument("--batch_scenes", type=int, default=64)
    parser.add_argument("--device", type=str, default=None)
    parser.add_argument("--json", type=str, default=None)
    args = parser.parse_args(argv)
    t0 = time.perf_counter()
    taus = [float(v) for v in args.prob_thresholds.split(",") if v.strip()]
    scanned = list_scenes(args.data_root, args.split, args.stride)
    present = [s for s in scanned if osp.exists(osp.join(args.ps_folder, s + ".pth"))]
    have = set(present)
    missing = [s for s in scanned if s not in have]
    rows = len(taus) + 1
    ious = [dict() for _ in range(rows)]
    conf = np.zeros((rows, 19, 19), dtype=np.int64)
    kept = np.zeros(rows, dtype=np.int64)
    evaluated, failed = [], {}
    t_eval = 0.0  # time in evaluate_scenes (upload, kernels, download): the rest of the run is reading
    for names, scenes in read_scene_batches(args, present, bool(taus), failed):
        t1 = time.perf_counter()
        res = evaluate_scenes(scenes, taus, scannet_remap=True, num_classes=19, device=args.device)
        t_eval += time.perf_counter() - t1
        for name, per_row in zip(names, res.ious):
            for r in range(rows):
                ious[r][name] = per_row[r]
        conf += res.conf
        kept += res.kept.sum(axis=0)
        evaluated += names
    elapsed = time.perf_counter() - t0

    out = dict(data_root=args.data_root, split=args.split, ps_folder=args.ps_folder, stride=args.stride,
               scanned=scanned, evaluated=evaluated, missing=missing, failed=failed, points=int(kept[0]))
    if evaluated:
        mean_iou = mean_instance_iou(ious[0])
        iou, miou = sem_iou_from_conf(conf[0])
        print("mean inst iou", mean_iou)  # :240
        print("sem iou", iou.tolist())    # :250
        print("sem miou", miou)           # :251
        names = list(CLASSES) + [CLASS_18]
        print("%-16s %8s" % ("class", "iou"))
        for c, v in enumerate(iou):
            print("%-16s %8.2f" % (names[c] if c < len(names) else str(c), v))
        out.update(mean_inst_iou=_nan_to_none(mean_iou), sem_iou=[_nan_to_none(v) for v in iou],
                   sem_miou=_nan_to_none(miou),
                   per_class={(names[c] if c < len(names) else str(c)): _nan_to_none(v) for c, v in enumerate(iou)})
        out["thresholds"] = []
        if taus:
            print("%-10s %10s %14s %10s" % ("prob >=", "coverage", "mean inst iou", "sem miou"))
        for j, tau in enumerate(taus):
            r = j + 1
            m = mean_instance_iou(ious[r])
            t_iou, t_miou = sem_iou_from_conf(conf[r])
            cov = float(kept[r]) / float(kept[0]) if kept[0] else float("nan")
            print("%-10g %10.4f %14s %10.4f" % (tau, cov, "%.6f" % m if m is not None else "-", t_miou))
            out["thresholds"].append(dict(threshold=tau, kept_points=int(kept[r]), coverage=_nan_to_none(cov),
                                          mean_inst_iou=_nan_to_none(m), sem_iou=[_nan_to_none(v) for v in t_iou],
                                          sem_miou=_nan_to_none(t_miou)))
    print("[eval_ps_labels] %d scene(s) listed, %d evaluated, %d without a label file, %d failed in %.2f s"
          % (len(scanned), len(evaluated), len(missing), len(failed), elapsed), file=sys.stderr)
    if failed:
        print("[eval_ps_labels] %d scene(s) could not be evaluated: %s" % (len(failed), " ".join(sorted(failed))),
              file=sys.stderr)
        for name in sorted(failed):
            print("  %s: %s" % (name, failed[name]), file=sys.stderr)
    out.update(elapsed_s=elapsed, eval_s=t_eval, scenes_per_s=(len(evaluated) / elapsed if elapsed > 0 else None))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)
    if not evaluated:
        print("[eval_ps_labels] nothing was evaluated", file=sys.stderr)
        return 2
    return 3 if failed else 0


if __name__ == "__main__":
    import sys

    sys.exit(main())
