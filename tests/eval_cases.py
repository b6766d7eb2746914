"""Inputs of the evaluator edge tests (test_eval_edges_cpu.py / test_eval_edges_gpu.py) and plain NumPy references of the
two evaluators to hold gapro_amd/csrc/eval_batch.hip and eval_ap.hip to, bit for bit.

The references are written from the reference's lines and share no code with the package, with oracle/eval_oracle.py or
with tests/ap_tally.py:
* ``miou_reference``       -- gapro/eval_ps_labels.py:35-42,100-147: per GT id with points the largest
  inter / (|gt| + |ps| - inter + 1e-4) over the pseudo ids of the same class, every operation in float32 in that order;
  the class of an id is the label of its first point; ids of a negative class are dropped.
* ``conf_reference``       -- :150-172, a double loop over the classes.
* ``rows_reference``       -- the two above on all points (row 0) and on the points with prob >= float32(tau) per threshold,
  in the caller's order (main()'s certain_cond filter, :214-220), after main()'s .int() and remap (:192-197).
* ``ap_tables_reference``  -- the ten fields of ApTable from assign_instances_for_scan's encoding
  (ISBNet/isbnet/evaluation/instance_eval.py:244-336) as gapro/eval_ap_ps_labels.py:59-60,99-127 drives it.
Everything is integers or float32 / float64 in a fixed order: the GPU comparisons are bit equality.

Each reference takes switches, and each switch restates ONE mistake (MIOU_MISTAKES, AP_MISTAKES);
test_eval_edges_cpu.py uses them to show that a named case can tell the mistake.  Every case is a named entry of
IOU_CASES / CONF_CASES / AP_CASES, a small builder with a comment that says which branch it exists for;
test_eval_edges_cpu.py proves on the CPU that each is what the comment claims.
"""
from collections import OrderedDict, namedtuple
from functools import lru_cache

import numpy as np

F32, F64 = np.float32, np.float64

# structural constants the cases are built around
THREADS = 256           # eval_batch.hip:20, eval_ap.hip:23
PAIR_LDS = 8192         # eval_batch.hip:22,97 (B * (max_gt + 1) * (max_ps + 1)); eval_ap.hip:28,142 ((keys + 1) * (max_ps + 1))
ID_LDS = 512            # eval_batch.hip:21,144,149 (bin * cap + id); eval_ap.hip:29,142 (max_ps)
CONF_LDS = 2048         # eval_batch.hip:23,99 (B * C * C)
AP_INST = 1000          # eval_ap.hip:25: inst + 1 in [0, 1000), inst in -1..998
AP_CLASSES = 18         # eval_ap.hip:24
AP_CODES = AP_CLASSES * AP_INST   # eval_ap.hip:26
AP_WORDS = 563          # eval_ap.hip:27: (18000 + 31) / 32; the last word's bits from 16 on are padding
RANK_WORDS_PER_THREAD = 3         # eval_ap.hip:105: threads from 188 on have no word
MAX_THRESHOLDS = 32     # include/gapro_hip.h GAPRO_EVAL_MAX_THRESHOLDS; eval_batch.hip:24 (33 bins)
EVB_PER_THREAD, EVB_GRID_CAP = 4, 128   # eval_batch.hip:328
AP_PER_THREAD, AP_GRID_CAP = 8, 128     # eval_ap.hip:346,393
EVB_BLOCK2 = THREADS * EVB_PER_THREAD + 1                  # 1025: the grid's second workgroup
EVB_WRAP = THREADS * EVB_PER_THREAD * EVB_GRID_CAP + 1     # 131 073: one point past the capped grid's first sweep...
AP_BLOCK2 = THREADS * AP_PER_THREAD + 1                    # 2049
AP_WRAP = THREADS * AP_PER_THREAD * AP_GRID_CAP + 1        # 262 145
assert (AP_WORDS, EVB_BLOCK2, EVB_WRAP, AP_BLOCK2, AP_WRAP) == ((AP_CODES + 31) // 32, 1025, 131073, 2049, 262145)

FIELDS = ("semantic_label", "instance_label", "ps_semantic_label", "ps_instance_label", "ps_prob")


# ================================================================================================ label conversion
def to_int(a, labels="trunc"):
    """Labels as int64: float64 labels are truncated (the reference's .int()).  labels="round" / "floor": the mistakes."""
    a = np.asarray(a)
    if a.dtype.kind != "f":
        return a.astype(np.int64)
    f = {"trunc": np.trunc, "round": np.rint, "floor": np.floor}[labels]
    return f(a).astype(np.int64)


def remap_sem(sem, times=1):
    """eval_ps_labels.py:196-197 / eval_ap_ps_labels.py:59-60.  times = 0 / 2: the remap left out / applied twice."""
    sem = np.array(sem, dtype=np.int64)
    for _ in range(times):
        sem[sem != -100] -= 2
        sem[(sem == -1) | (sem == -2)] = 18
    return sem


# ================================================================================================ eval_batch references
def _classes(ids, sem, n_ids, how):
    """Per id in [0, n_ids) the class: label of the id's first point, -1 for an id without points.  how="majority" /
    "last": the mistakes."""
    cls = np.full(n_ids, -1, np.int64)
    for i in range(n_ids):
        idx = np.flatnonzero(ids == i)
        if len(idx) == 0:
            continue
        if how == "first":
            cls[i] = sem[idx[0]]
        elif how == "last":
            cls[i] = sem[idx[-1]]
        else:
            vals, cnt = np.unique(sem[idx], return_counts=True)
            cls[i] = vals[np.argmax(cnt)]
    return cls


def miou_reference(sem, ins, ps_sem, ps_ins, cls_from="first", gt_cls=None, ps_cls=None):
    """float32 [ids with points and a class >= 0], in id order.  Integer arrays; gt_cls / ps_cls override the classes (the
    first-point-of-the-unfiltered-scene mistake passes the whole scene's)."""
    sem, ins, ps_sem, ps_ins = (np.asarray(a, np.int64) for a in (sem, ins, ps_sem, ps_ins))
    n_gt = int(ins.max()) + 1 if len(ins) else 0
    n_ps = int(ps_ins.max()) + 1 if len(ins) else 0
    n_gt, n_ps = max(n_gt, 0), max(n_ps, 0)
    cg = _classes(ins, sem, n_gt, cls_from) if gt_cls is None else np.asarray(gt_cls)[:n_gt]
    cp = _classes(ps_ins, ps_sem, n_ps, cls_from) if ps_cls is None else np.asarray(ps_cls)[:n_ps]
    out = []
    for g in range(n_gt):
        in_g = ins == g
        gt_n = int(in_g.sum())
        if gt_n == 0 or cg[g] < 0:
            continue
        best = F32(0.0)
        # a pseudo id without a point in common has IoU 0 and cannot raise the maximum over 0: only the others are visited
        for p in sorted(set(ps_ins[in_g].tolist())):
            if p < 0:
                continue
            in_p = ps_ins == p
            ps_n = int(in_p.sum())
            inter = F32(int((in_g & in_p).sum()))
            union = F32(F32(F32(gt_n) + F32(ps_n)) - inter)
            iou = F32(inter / F32(union + F32(1e-4)))
            v = F32(iou * F32(1.0 if cg[g] == cp[p] else 0.0))
            if v > best:
                best = v
        out.append(best)
    return np.asarray(out, F32)


def conf_reference(sem, ps_sem, C):
    """int64 [C, C], conf[gt, ps]; a pseudo -100 counts as gt + 1 (gt - 1 from 18 on); GT -100 is dropped."""
    sem, ps_sem = np.asarray(sem, np.int64), np.asarray(ps_sem, np.int64)
    keep = sem != -100
    gt, ps = sem[keep], ps_sem[keep].copy()
    none = ps == -100
    ps[none] = np.where(gt[none] < 18, gt[none] + 1, gt[none] - 1)
    conf = np.zeros((C, C), np.int64)
    for g in range(C):
        for p in range(C):
            conf[g, p] = int(((gt == g) & (ps == p)).sum())
    return conf


def conf_in_range(sem, ps_sem, C):
    """Every flat index ps + C * gt inside [0, C * C): outside it the reference's bincount itself fails."""
    sem, ps_sem = np.asarray(sem, np.int64), np.asarray(ps_sem, np.int64)
    keep = sem != -100
    gt, ps = sem[keep], ps_sem[keep].copy()
    none = ps == -100
    ps[none] = np.where(gt[none] < 18, gt[none] + 1, gt[none] - 1)
    x = ps + C * gt
    return bool(((x >= 0) & (x < C * C)).all())


Row = namedtuple("Row", "ious conf kept")

# one switch per mistake: name -> keyword arguments of rows_reference
MIOU_MISTAKES = OrderedDict([
    ("class_majority", dict(cls_from="majority")),
    ("class_last", dict(cls_from="last")),
    ("class_first_unfiltered", dict(cls_from="first_unfiltered")),
    ("strict_compare", dict(compare="gt")),
    ("float64_threshold", dict(compare="f64")),
    ("labels_rounded", dict(labels="round")),
    ("rows_keep_bins_above", dict(bins="above")),
    ("rows_shifted_by_one", dict(bins="shift")),
    ("equal_thresholds_collapsed", dict(bins="collapse")),
    ("remap_left_out", dict(remap_delta=-1)),
    ("remap_twice", dict(remap_delta=1)),
])


def scene_ints(sc, remap, labels="trunc"):
    """(sem, ins, ps_sem, ps_ins) of a scene as int64 after main()'s .int() and ``remap`` applications of the remap."""
    return (remap_sem(to_int(sc["semantic_label"], labels), remap), to_int(sc["instance_label"], labels),
            to_int(sc["ps_semantic_label"]), to_int(sc["ps_instance_label"]))


def keep_mask(prob, tau, compare="ge"):
    """The points of a threshold: prob >= float32(tau).  compare="gt" / "f64": the mistakes."""
    prob = np.asarray(prob, F32)
    if compare == "gt":
        return prob > F32(tau)
    if compare == "f64":
        return prob.astype(F64) >= float(tau)
    return prob >= F32(tau)


def rows_reference(sc, thresholds=(), remap=True, num_classes=19, cls_from="first", compare="ge", labels="trunc",
                   bins=None, remap_delta=0):
    """[Row] of one scene: row 0 = all points, row j + 1 = the points with prob >= float32(thresholds[j])."""
    sem, ins, ps_sem, ps_ins = scene_ints(sc, (1 if remap else 0) + remap_delta, labels)
    n, K = len(sem), len(thresholds)
    masks = [np.ones(n, bool)]
    if bins is None:
        masks += [keep_mask(sc["ps_prob"], t, compare) for t in thresholds]
    else:
        # the mistakes of a bin scheme: bin = thresholds passed (ascending), row t (ascending order) = bins >= t
        thr = np.asarray(thresholds, F32)
        order = np.argsort(thr, kind="stable")
        srt = thr[order]
        prob = np.asarray(sc["ps_prob"], F32) if K else np.zeros(n, F32)
        if bins == "collapse":
            b = np.zeros(n, np.int64)
            for t in np.unique(srt):
                b += prob >= t
        else:
            b = np.zeros(n, np.int64)
            for t in srt:
                b += prob >= t
        by_rank = []
        for t in range(1, K + 1):
            by_rank.append({"above": b > t, "shift": b >= t + 1, "collapse": b >= t}[bins])
        if bins == "above":
            masks[0] = b > 0
        rank = np.empty(K, np.int64)
        rank[order] = np.arange(K)
        masks += [by_rank[rank[j]] for j in range(K)]
    gt_all = ps_all = None
    if cls_from == "first_unfiltered":
        n_gt = max(int(ins.max()) + 1, 0) if n else 0
        n_ps = max(int(ps_ins.max()) + 1, 0) if n else 0
        gt_all, ps_all = _classes(ins, sem, n_gt, "first"), _classes(ps_ins, ps_sem, n_ps, "first")
    out = []
    for m in masks:
        ious = miou_reference(sem[m], ins[m], ps_sem[m], ps_ins[m], "first" if gt_all is not None else cls_from,
                              gt_all, ps_all)
        out.append(Row(ious, conf_reference(sem[m], ps_sem[m], num_classes), int(m.sum())))
    return out


# ================================================================================================ eval_batch cases
EvalCase = namedtuple("EvalCase", "name scenes thresholds remap num_classes meta")


def _freeze(sc):
    for k in FIELDS:
        if sc.get(k) is not None:
            sc[k].setflags(write=False)
    return sc


def writable(sc):
    """A scene with writable copies of its arrays, for the functions under test (the cases themselves stay frozen)."""
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in sc.items()}


def _scene(sem, ins, ps_sem, ps_ins, prob=None, gt_dtype=F64, ps_dtype=np.int32, **caps):
    n = len(sem)
    prob = np.full(n, 0.5, F32) if prob is None else np.asarray(prob, F32)
    sc = dict(semantic_label=np.asarray(sem).astype(gt_dtype), instance_label=np.asarray(ins).astype(gt_dtype),
              ps_semantic_label=np.asarray(ps_sem).astype(ps_dtype), ps_instance_label=np.asarray(ps_ins).astype(ps_dtype),
              ps_prob=prob)
    sc.update(caps)
    return _freeze(sc)


def _random_labels(rng, n, n_gt, n_ps, raw=True):
    """GT id g of class g % 18, pseudo id mostly g % n_ps of class id % 18, some noise and some -100 on every array.  raw:
    ScanNet's raw classes (class + 2; 0 / 1 are wall / floor), for the remap."""
    g = rng.integers(0, n_gt, n)
    p = np.where(rng.random(n) < 0.75, g % n_ps, rng.integers(0, n_ps, n))
    sem = g % 18 + (2 if raw else 0)
    noisy = rng.random(n) < 0.1
    sem[noisy] = rng.integers(0, 21 if raw else 19, int(noisy.sum()))
    ps_sem = p % 18
    noisy = rng.random(n) < 0.1
    ps_sem[noisy] = rng.integers(0, 19, int(noisy.sum()))
    g[rng.random(n) < 0.1] = -100
    sem[rng.random(n) < 0.05] = -100
    none = rng.random(n) < 0.1
    p[none] = -100
    ps_sem[none] = -100
    return sem, g, ps_sem, p


def _cover(ins, ps_ins, n_gt, n_ps):
    """The last points carry the largest ids, so that the last row and column of the tables are used."""
    if len(ins):
        ins[-1], ps_ins[-1] = n_gt - 1, n_ps - 1
    return ins, ps_ins


def _ladder_scene(seed, n, raw=True):
    """A random scene whose last point alone carries a GT id and a pseudo id of their own (one more IoU row that is lost
    with the point)."""
    rng = np.random.default_rng(seed)
    sem, g, ps_sem, p = _random_labels(rng, n, 7, 9, raw)
    if n:
        g[-1], p[-1], sem[-1], ps_sem[-1] = 7, 9, 5 + (2 if raw else 0), 5
    return _scene(sem, g, ps_sem, p, rng.random(n).astype(F32))


EVB_LADDER = (0, 1, THREADS - 1, THREADS, THREADS + 1, EVB_BLOCK2 - 1, EVB_BLOCK2, 0, EVB_WRAP)
AP_LADDER = (0, 1, THREADS - 1, THREADS, THREADS + 1, AP_BLOCK2 - 1, AP_BLOCK2, 0, AP_WRAP)


def _iou_size_ladder():
    # the grid is sized by the largest scene, workgroups of smaller scenes leave early (eval_batch.hip:90); empty scenes in
    # the middle; 1025 = the second workgroup's first point, 131 073 = the first point of the capped grid's second sweep
    scenes = [_ladder_scene(100 + i, n) for i, n in enumerate(EVB_LADDER)]
    return EvalCase("size_ladder", scenes, (0.6, 0.3), True, 19, dict(sizes=EVB_LADDER))


def _pair_scene(seed, n, n_gt, n_ps, taus=()):
    rng = np.random.default_rng(seed)
    sem, g, ps_sem, p = _random_labels(rng, n, n_gt, n_ps)
    g, p = _cover(g, p, n_gt, n_ps)
    prob = rng.random(n).astype(F32)
    prob[-1] = 1.0  # the last cell of the last bin
    return sem, g, ps_sem, p, prob


def _iou_pair(name, max_ps, taus):
    # lds_pair = B * (max_gt + 1) * (max_ps + 1) <= 8192 (eval_batch.hip:97): the same points on both sides of it
    def build():
        sem, g, ps_sem, p, prob = _pair_scene(7 if not taus else 8, 3000, 63, 127 if not taus else 63, taus)
        return EvalCase(name, [_scene(sem, g, ps_sem, p, prob, max_gt=63, max_ps=max_ps)], taus, True, 19,
                        dict(cells=(len(taus) + 1) * 64 * (max_ps + 1)))
    return build


STRADDLE_IDS = (210, 211, 212, 213, 214)
STRADDLE_TAUS = (0.4, 0.8)


def _iou_first_straddle():
    # first points go to LDS or to global memory per entry, f = bin * cap + id < 512 (eval_batch.hip:144,149): with caps
    # of 300 and three bins, bin 1 holds ids 0..211 in LDS and ids from 212 on in global memory.  Ids 210..214 have points
    # in all three bins.  Arrangement A (210, 212, 214): the id's points come in the order bin 2, bin 1, bin 0, so rows 0
    # and 1 must take bin 2's first point; arrangement B (211, 213): bin 1, bin 0, bin 2, so row 0 takes bin 1's and row 1
    # must keep its own.  One side's class is constant, the other side's is that class only at the row's true first point
    # (B: bin 2's first point carries another class, so row 2 is a mismatch and a row 1 that took it would be one too).
    pb = {0: F32(0.1), 1: F32(0.5), 2: F32(0.9)}
    scenes = []
    for varying in ("ps", "gt"):
        rng = np.random.default_rng(31 if varying == "ps" else 32)
        ids, cls_c, cls_v, prob = [], [], [], []

        def add(i, c_const, c_var, b, k=1):
            ids.extend([i] * k), cls_c.extend([c_const] * k), cls_v.extend([c_var] * k), prob.extend([pb[b]] * k)

        # filler in front: ids below 200 in random bins, both sides one class
        for i in rng.integers(0, 200, 300):
            add(int(i), int(i) % 17, int(i) % 17, int(rng.integers(0, 3)))
        for i in STRADDLE_IDS:
            c = i % 17
            if i % 2 == 0:
                add(i, c, c, 2), add(i, c, c + 1, 1), add(i, c, c + 1, 0)
            else:
                add(i, c, c, 1), add(i, c, c + 1, 0), add(i, c, c + 1, 2)
        # the bulk of the edge ids, behind their first points, and more filler up to id 299
        for i in list(STRADDLE_IDS) * 12 + [int(v) for v in rng.integers(200, 300, 600)] + [299]:
            if i in STRADDLE_IDS:
                add(i, i % 17, i % 17 + 1, int(rng.integers(0, 3)))
            else:
                add(i, i % 17, i % 17, int(rng.integers(0, 3)))
        ids, cls_c, cls_v = np.asarray(ids), np.asarray(cls_c), np.asarray(cls_v)
        gt_sem, ps_sem = (cls_c, cls_v) if varying == "ps" else (cls_v, cls_c)
        scenes.append(_scene(gt_sem + 2, ids, ps_sem, ids, np.asarray(prob, F32), max_gt=300, max_ps=300))
    return EvalCase("first_straddle", scenes, STRADDLE_TAUS, True, 19, dict(ids=STRADDLE_IDS, cap=300))


def _iou_first_alone():
    # the class of an id is the label of its first point: id 0's first point is the scene's point 0 (workgroup 0 of three),
    # all its other points lie beyond point 1024 and carry another class; id 1's only point is the scene's last
    rng = np.random.default_rng(41)
    n = 3000
    sem, g, ps_sem, p = _random_labels(rng, n, 12, 12)
    g[g == 0], p[p == 0] = 5, 5
    g[g == 1], p[p == 1] = 6, 6
    far = np.arange(1100, 1400)
    g[0], p[0], sem[0], ps_sem[0] = 0, 0, 5 + 2, 5
    g[far], p[far], sem[far], ps_sem[far] = 0, 0, 6 + 2, 5   # GT majority class 6; the pseudo id is class 5 throughout
    g[-1], p[-1], sem[-1], ps_sem[-1] = 1, 1, 9 + 2, 9
    return EvalCase("first_alone", [_scene(sem, g, ps_sem, p)], (), True, 19, dict(far=(1100, 1400)))


def _iou_first_filtered():
    # the first point in the ROW's filtered points: id 0's first point has a probability under the threshold and another
    # class than the rest, so rows 0 and 1 give the id different classes (GT side: id 0; pseudo side: id 1)
    rng = np.random.default_rng(42)
    n = 1500
    sem, g, ps_sem, p = _random_labels(rng, n, 10, 10)
    for i in (0, 1):
        g[g == i], p[p == i] = 5, 5
    prob = rng.uniform(0.6, 1.0, n).astype(F32)
    prob[rng.random(n) < 0.3] = 0.2
    a, b = np.arange(100, 300), np.arange(400, 600)
    g[a], p[a], sem[a], ps_sem[a], prob[a] = 0, 0, 6 + 2, 6, 0.9
    sem[a[0]], prob[a[0]] = 5 + 2, 0.1
    g[b], p[b], sem[b], ps_sem[b], prob[b] = 1, 1, 7 + 2, 7, 0.9
    ps_sem[b[0]], prob[b[0]] = 8, 0.1
    return EvalCase("first_filtered", [_scene(sem, g, ps_sem, p, prob)], (0.5,), True, 19, dict(first=(100, 400)))


TIE_TAUS = (0.5, 0.9, 0.999)


def tie_values():
    """float32(tau), the float32 below it and the one above it, per tau."""
    out = []
    for t in TIE_TAUS:
        t = F32(t)
        out += [np.nextafter(t, F32(0)), t, np.nextafter(t, F32(2))]
    return np.asarray(out, F32)


def _iou_thr_ties():
    # prob >= float32(tau) at equality and one ulp either side (eval_batch.hip:117): id k's 20 points all carry the k-th of
    # the nine values, so an id enters or leaves a row as a whole
    vals = tie_values()
    ids = np.repeat(np.arange(len(vals)), 20)
    return EvalCase("thr_ties", [_scene(ids % 17 + 2, ids, ids % 17, ids, vals[ids])], TIE_TAUS, True, 19, {})


def _iou_thr(name, seed, taus, n=2000, n_ids=9, special=None):
    def build():
        rng = np.random.default_rng(seed)
        sem, g, ps_sem, p = _random_labels(rng, n, n_ids, n_ids)
        g, p = _cover(g, p, n_ids, n_ids)
        prob = rng.random(n).astype(F32)
        if special is not None:
            special(sem, g, ps_sem, p, prob)
        return EvalCase(name, [_scene(sem, g, ps_sem, p, prob)], taus, True, 19, {})
    return build


def _outside_special(sem, g, ps_sem, p, prob):
    # exact 0 and 1 among the probabilities, and one NaN on a point with ids of its own: it lands in row 0 only
    prob[10:40], prob[50:80] = 0.0, 1.0
    prob[5], g[5], p[5], sem[5], ps_sem[5] = np.nan, 9, 9, 4 + 2, 4


THR_MAX_TAUS = tuple((k + 1) / 34.0 for k in range(MAX_THRESHOLDS))


def _iou_truncation():
    # float64 GT labels are truncated (eval_labels.h label_at, the reference's .int()): 2.9 and 3.999 are 2 and 3, and
    # -0.5 is instance 0 and class 0 (no remap here, so class 0 stays class 0)
    rng = np.random.default_rng(51)
    n = 900
    base = rng.integers(1, 6, n)                                # ids and classes 1..5
    frac = rng.choice([0.0, 0.9, 0.999, 0.5], n)
    ins, sem = base + frac, (base + 3) + rng.choice([0.0, 0.9, 0.999], n)
    zero = rng.random(n) < 0.15
    ins[zero], sem[zero], base[zero] = -0.5, -0.5, 0
    ins[:4], sem[:4] = [2.9, 3.0, 3.999, -0.5], [5.9, 6.0, 6.999, -0.5]
    base[:4] = [2, 3, 3, 0]
    ps_sem = np.where(base == 0, 0, base + 3)
    return EvalCase("truncation", [_scene(sem, ins, ps_sem, base.copy())], (), False, 19, dict(ids=base))


def _iou_no_ids():
    # max_gt = max_ps = 1 with every id negative: no IoU row at all, the confusion still counts
    rng = np.random.default_rng(52)
    sem, g, ps_sem, p = _random_labels(rng, 500, 3, 3)
    g[:], p[:] = -100, -100
    return EvalCase("no_ids", [_scene(sem, g, ps_sem, p)], (0.5,), True, 19, {})


def _iou_one_each():
    # one GT id and one pseudo id: the smallest tables (2 x 2 cells)
    rng = np.random.default_rng(53)
    sem, g, ps_sem, p = _random_labels(rng, 700, 1, 1)
    sem[0], g[0], ps_sem[0], p[0] = 4 + 2, 0, 4, 0
    return EvalCase("one_each", [_scene(sem, g, ps_sem, p, rng.random(700).astype(F32))], (0.5,), True, 19, {})


def _thr_max_special(sem, g, ps_sem, p, prob):
    prob[:] = (np.arange(len(prob)) % 67) / F32(66.0)   # every bin of the 33 is used, 0 and 1 included


IOU_CASES = OrderedDict([
    ("size_ladder", _iou_size_ladder),
    ("pair_8192", _iou_pair("pair_8192", 127, ())),
    ("pair_8256", _iou_pair("pair_8256", 128, ())),
    ("pair_b2_4096", _iou_pair("pair_b2_4096", 63, (0.5,))),
    ("pair_b2_over", _iou_pair("pair_b2_over", 64, (0.5,))),
    ("first_straddle", _iou_first_straddle),
    ("first_alone", _iou_first_alone),
    ("first_filtered", _iou_first_filtered),
    ("thr_ties", _iou_thr_ties),
    # equal thresholds, in the caller's order: equal rows (evaluate_scenes' perm[1 + order])
    ("thr_equal", _iou_thr("thr_equal", 61, (0.7, 0.7, 0.3, 0.7))),
    # thresholds under every probability, above 1 and infinite: rows that keep every point and rows that keep none
    ("thr_outside", _iou_thr("thr_outside", 62, (-1.0, 0.0, 1.0, 1.5, float("inf")), special=_outside_special)),
    # 32 thresholds: 33 bins (s_kept[33]); ids 0..39: ids past 512 / 33 are in global memory from bin 12 on, every id from
    # bin 13 on
    ("thr_max", _iou_thr("thr_max", 63, THR_MAX_TAUS, n=4000, n_ids=40, special=_thr_max_special)),
    ("truncation", _iou_truncation),
    ("no_ids", _iou_no_ids),
    ("one_each", _iou_one_each),
])


def _conf_scene(seed, n, C, raw, void_ps=True):
    rng = np.random.default_rng(seed)
    sem = rng.integers(0, C + (2 if raw else 0), n)
    ps_sem = rng.integers(0, C, n)
    sem[rng.random(n) < 0.1] = -100
    if void_ps:
        ps_sem[rng.random(n) < 0.1] = -100
    sem[-1], ps_sem[-1] = C - 1 + (2 if raw else 0), C - 1   # the last bin of the table
    ins = rng.integers(0, 4, n)
    return sem, ins, ps_sem, ins.copy(), rng.random(n).astype(F32)


CONF_TAUS5 = (0.2, 0.4, 0.6, 0.8, 0.9)


def _conf_c19(name, K):
    # lds_conf = B * C * C <= 2048 (eval_batch.hip:99): with C = 19 five bins fit (1805) and six do not (2166); the same
    # points with the first four and with all five thresholds
    def build():
        return EvalCase(name, [_scene(*_conf_scene(71, 2500, 19, True))], CONF_TAUS5[:K], True, 19,
                        dict(bins=(K + 1) * 361))
    return build


def _conf_classes(C):
    # one bin: the switch is between C = 45 (2025) and C = 46 (2116); 1 and 128 are the ends of the legal range.  C = 1 has
    # no pseudo -100 (gt + 1 would leave the table)
    def build():
        return EvalCase("classes_%d" % C, [_scene(*_conf_scene(72 + C, 1500, C, False, void_ps=C >= 19))], (), False, C,
                        dict(bins=C * C))
    return build


def _conf_gt_void():
    # GT -100 is dropped whatever the pseudo label is
    sem, ins, ps_sem, ps_ins, prob = _conf_scene(75, 800, 19, True)
    sem[::3] = -100
    return EvalCase("gt_void", [_scene(sem, ins, ps_sem, ps_ins, prob)], (0.5,), True, 19, {})


def _conf_ps_void():
    # the reference's +1 / -1 rule (:157-161): pseudo -100 at gt 0, 17 and 18 counts as 1, 18 and 17
    gt = np.repeat([0, 17, 18, 5], [30, 40, 50, 60])
    ps = np.full(len(gt), -100)
    ps[::7] = gt[::7]
    ins = np.zeros(len(gt), np.int64)
    raw = np.where(gt == 18, 1, gt + 2)
    return EvalCase("ps_void", [_scene(raw, ins, ps, ins.copy())], (), True, 19, dict(gt=gt))


CONF_CASES = OrderedDict([
    ("c19_k4", _conf_c19("c19_k4", 4)),
    ("c19_k5", _conf_c19("c19_k5", 5)),
    ("classes_1", _conf_classes(1)),
    ("classes_45", _conf_classes(45)),
    ("classes_46", _conf_classes(46)),
    ("classes_128", _conf_classes(128)),
    ("gt_void", _conf_gt_void),
    ("ps_void", _conf_ps_void),
])


@lru_cache(maxsize=None)
def eval_case(name):
    return (IOU_CASES.get(name) or CONF_CASES[name])()


@lru_cache(maxsize=None)
def eval_expected(name):
    """[scene][row] Row of a case, computed once."""
    case = eval_case(name)
    return [rows_reference(sc, case.thresholds, case.remap, case.num_classes) for sc in case.scenes]


# ================================================================================================ eval_ap reference
ApRef = namedtuple("ApRef", "gt_code gt_n pred_id pred_label pred_n pred_void pred_conf pair_gt pair_pred pair_inter")

AP_MISTAKES = OrderedDict([
    ("inst_minus_one_void", dict(inst_m1_void=True)),
    ("inst_999_legal", dict(inst_999_legal=True)),
    ("class_19_instance", dict(class_19=True)),
    ("remap_left_out", dict(remap_delta=-1)),
    ("remap_twice", dict(remap_delta=1)),
    ("mean_in_float32", dict(mean_f32=True)),
    ("pred_class_majority", dict(cls_from="majority")),
    ("labels_rounded", dict(labels="round")),
])


def ap_tables_reference(sem_gt, inst_gt, ps_sem, ps_inst, prob=None, confidence="one", remap=True, max_ps=None,
                        inst_m1_void=False, inst_999_legal=False, class_19=False, remap_delta=0, mean_f32=False,
                        cls_from="first", labels="trunc"):
    """One scene's ApRef.  Raises ValueError for what ap_tables refuses: a GT instance id >= 999, a pseudo id < 0 other
    than -100 or >= max_ps, and with confidence="mean_prob" a probability that is NaN or outside [0, 1]."""
    sem = remap_sem(to_int(sem_gt, labels), (1 if remap else 0) + remap_delta)
    ins, ps_sem, ps = to_int(inst_gt, labels), to_int(ps_sem), to_int(ps_inst)
    n = len(sem)
    if max_ps is None:
        max_ps = max(int(ps.max()) + 1, 1) if n else 1
    if (ins + 1 >= AP_INST).any() and not inst_999_legal:
        raise ValueError("a GT instance id >= 999")
    if (((ps < 0) & (ps != -100)) | (ps >= max_ps)).any():
        raise ValueError("a pseudo id outside the table")
    if confidence == "mean_prob":
        prob = np.asarray(prob, F32)
        if not ((prob >= 0) & (prob <= 1)).all():
            raise ValueError("a probability outside [0, 1]")
    # assign_instances_for_scan: class = sem + 1 with 19 -> 0 and < 0 -> 0; code = class * 1000 + inst + 1, 0 for
    # inst + 1 < 0; a GT instance has a class in 1..18
    cls = np.where((sem >= 0) & (sem < (19 if class_19 else 18)), sem + 1, 0)
    inst_ok = (cls > 0) & ((ins >= 0) if inst_m1_void else (ins >= -1))
    code = np.where(inst_ok, cls * 1000 + ins + 1, 0)
    gt_code = sorted(set(code[inst_ok].tolist()))
    gt_n = [int((code == c).sum()) for c in gt_code]
    pred_id, pred_label, pred_n, pred_void, pred_conf = [], [], [], [], []
    for u in sorted(set(ps.tolist())):
        if u == -100:
            continue
        idx = np.flatnonzero(ps == u)
        if cls_from == "first":
            label = int(ps_sem[idx[0]]) + 1
        else:
            vals, cnt = np.unique(ps_sem[idx], return_counts=True)
            label = int(vals[np.argmax(cnt)]) + 1
        if not 1 <= label <= AP_CLASSES:
            continue
        pred_id.append(u), pred_label.append(label), pred_n.append(len(idx))
        pred_void.append(int((~inst_ok[idx]).sum()))
        if confidence == "one":
            pred_conf.append(1.0)
        elif mean_f32:
            s = F32(0)
            for v in prob[idx]:
                s = F32(s + v)
            pred_conf.append(float(F32(s / F32(len(idx)))))
        else:
            s = sum(int(np.rint(F64(v) * 2.0 ** 32)) for v in prob[idx])
            pred_conf.append(float(F64(s) / (F64(len(idx)) * 2.0 ** 32)))
    pair_gt, pair_pred, pair_inter = [], [], []
    for gi, c in enumerate(gt_code):
        in_g = code == c
        touched = set(ps[in_g].tolist())
        for pi, u in enumerate(pred_id):
            if c // 1000 != pred_label[pi] or u not in touched:
                continue
            inter = int((in_g & (ps == u)).sum())
            if inter > 0:
                pair_gt.append(gi), pair_pred.append(pi), pair_inter.append(inter)
    i64 = lambda v: np.asarray(v, np.int64).reshape(-1)  # noqa: E731
    return ApRef(i64(gt_code), i64(gt_n), i64(pred_id), i64(pred_label), i64(pred_n), i64(pred_void),
                 np.asarray(pred_conf, F64).reshape(-1), i64(pair_gt), i64(pair_pred), i64(pair_inter))


def tables_equal(a, b):
    """Field by field: shapes, values and dtypes (int64, pred_conf float64)."""
    for f in ApRef._fields:
        x, y = np.asarray(getattr(a, f)), np.asarray(getattr(b, f))
        if x.shape != y.shape or x.dtype != y.dtype or not np.array_equal(x, y):
            return False
    return True


# ================================================================================================ eval_ap cases
ApCase = namedtuple("ApCase", "name scenes confidence remap meta")


def key_index(cls, inst):
    """The bit of a GT instance in the presence bitmap (eval_ap.hip:64): the code cls * 1000 + inst + 1 less 1000."""
    return (cls - 1) * AP_INST + inst + 1


def _ap_random(seed, n, n_gt, n_ps, max_ps=None, gt_dtype=F64, classes=17):
    """GT id g of class 1 + g % classes (raw class + 1), pseudo id mostly g % n_ps; every id from 0 to the largest is
    used, the last points carry the largest."""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, n_gt, n)
    p = np.where(rng.random(n) < 0.75, g % n_ps, rng.integers(0, n_ps, n))
    k = min(n, n_gt)
    g[n - k:] = np.arange(n_gt - k, n_gt)
    k = min(n, n_ps)
    p[n - k:] = np.arange(n_ps - k, n_ps)
    sem = g % classes + 1 + 1                       # class c is raw c + 1
    ps_sem = p % classes
    sem[rng.random(n) < 0.05] = rng.integers(0, 2)  # wall / floor: void
    none = rng.random(n) < 0.1
    none[n - k:] = False
    p[none], ps_sem[none] = -100, -100
    caps = {} if max_ps is None else dict(max_ps=max_ps)
    return _scene(sem, g, ps_sem, p, rng.random(n).astype(F32), gt_dtype=gt_dtype, **caps)


def _ap_size_ladder():
    # as the eval_batch ladder, with AP's 8 points per thread: 2049 and 262 145 (eval_ap.hip:85,138,346,393)
    scenes = []
    for i, n in enumerate(AP_LADDER):
        sc = dict(_ap_random(200 + i, n, 6, 7))
        if n:  # the last point alone carries a GT instance and a prediction of their own
            for k, v in zip(FIELDS[:4], (9, 900, 7, 7)):
                a = sc[k].copy()
                a[-1] = v
                sc[k] = a
        scenes.append(_freeze(sc))
    return ApCase("size_ladder", scenes, "mean_prob", True, dict(sizes=AP_LADDER))


# (n_keys, max_ps): 8192 cells, both tables in LDS | pairs in global memory, ids in LDS | 8193 cells, both in global
# memory | the id split with the pairs in LDS, on either side of 512.  15 ROWS (14 keys and the void row) keep the pairs in
# LDS at 513 and 514 columns (7695 and 7710 cells); 15 keys would make 16 * 513 = 8208 cells and leave it.
MIX4 = ((63, 127), (63, 128), (2, 2730), (14, 512), (14, 513))


def _ap_mix4():
    scenes = []
    for i, (n_keys, max_ps) in enumerate(MIX4):
        n_used = min(max_ps, 200) if max_ps != 2730 else 2730
        sc = dict(_ap_random(300 + i, 6000, n_keys, n_used, max_ps=max_ps, classes=min(n_keys, 17)))
        if max_ps > n_used:  # the largest id is used too
            for k, v in ((FIELDS[3], max_ps - 1), (FIELDS[2], 3)):
                a = sc[k].copy()
                a[0] = v
                sc[k] = a
        scenes.append(_freeze(sc))
    return ApCase("mix4", scenes, "mean_prob", True, dict(tables=MIX4))


KEY_BITS = (0, 31, 32, 63, 40, 41, 999, 1000, 17983, 17999)


def _ap_key_bits(gt_dtype=F64):
    # the key bitmap (eval_ap.hip:92,167,233): bit 0 and bit 31 of word 0, the first and last bit of word 1, two neighbours
    # inside a word, the last instance of class 1 (inst 998) and the first of class 2 (inst -1), bit 31 of word 561 and the
    # last key 17 999 (class 18, inst 998) in word 562, whose bits from 16 on are padding.  Words 2..30 and 32..560 stay
    # empty: k_ap_rank's threads 1..186 sum nothing, and 188..255 have no word.  10 + 3 * j points per key, shuffled.
    rng = np.random.default_rng(81)
    sem, ins = [], []
    for j, k in enumerate(KEY_BITS):
        cls, inst = k // AP_INST + 1, k % AP_INST - 1
        sem += [cls + 1] * (10 + 3 * j)
        ins += [inst] * (10 + 3 * j)
    sem, ins = np.asarray(sem), np.asarray(ins)
    perm = rng.permutation(len(sem))
    sem, ins = sem[perm], ins[perm]
    ps = rng.integers(0, 5, len(sem))
    ps_sem = np.where(rng.random(len(sem)) < 0.5, sem - 2, ps)   # half of the predictions' points in the GT's class
    ps_sem[np.unique(ps, return_index=True)[1]] = [0, 0, 1, 17, 17]  # classes 1, 1, 2, 18, 18: pairs with both ends
    return ApCase("key_bits", [_scene(sem, ins, ps_sem, ps, rng.random(len(sem)).astype(F32), gt_dtype=gt_dtype)],
                  "mean_prob", True, dict(keys=KEY_BITS))


ID_EDGES = (  # (raw class, inst, points, is a GT instance)
    (3, -1, 30, True), (3, 0, 31, True), (3, 998, 32, True), (4, -1, 29, True), (19, 997, 33, True), (19, -1, 34, True),
    (19, 998, 28, True),    # the last key of all
    (20, 5, 35, False),     # class 19: void
    (0, 6, 36, False), (1, 7, 37, False),   # raw 0 / 1 are class 19 after the remap: void
    (3, -2, 38, False), (3, -100, 39, False), (-100, 8, 40, False))


def _ap_id_edges(gt_dtype=F64):
    # the ends of the legal ranges (eval_ap.hip:62-63): inst -1, 0 and 998, class 18 with inst 997, 998 and -1; void: class
    # 19,
    # raw 0 / 1 under the remap, inst -2 and -100, class -100.  Segment j is covered by prediction j of the GT's class.
    rng = np.random.default_rng(82)
    sem, ins, ps, ps_sem = [], [], [], []
    for j, (raw, inst, k, _) in enumerate(ID_EDGES):
        sem += [raw] * k
        ins += [inst] * k
        ps += [j] * k
        ps_sem += [min(max(raw - 2, 0), 17)] * k
    perm = rng.permutation(len(sem))
    arrs = [np.asarray(a)[perm] for a in (sem, ins, ps_sem, ps)]
    return ApCase("id_edges", [_scene(*arrs, rng.random(len(sem)).astype(F32), gt_dtype=gt_dtype)], "mean_prob", True,
                  dict(edges=ID_EDGES))


def _ap_no_remap():
    # scannet_remap=False: labels 0..17 as they are; 18, 19 and -100 are void
    rng = np.random.default_rng(83)
    n = 2000
    g = rng.integers(0, 25, n)
    sem = g % 20
    sem[rng.random(n) < 0.05] = -100
    ps = g % 11
    ps_sem = np.where((sem >= 0) & (rng.random(n) < 0.8), sem, 18)   # 18 and 19 are no class of a prediction either
    return ApCase("no_remap", [_scene(sem, g, ps_sem, ps, rng.random(n).astype(F32))], "mean_prob", False, {})


def _ap_wide_max_ps():
    # an explicit max_ps three times the largest id + 1: ids without points; the tables equal those of the default size
    a, b = dict(_ap_random(84, 3000, 20, 30)), dict(_ap_random(85, 2500, 8, 200))
    wide = [_freeze(dict(a, max_ps=90)), _freeze(dict(b, max_ps=600))]
    return ApCase("wide_max_ps", wide, "mean_prob", True, dict(default=[_freeze(a), _freeze(b)]))


PROB_GRID = (0.0, -0.0, 1.0, 1.0 - 2.0 ** -24, 2.0 ** -33, 3 * 2.0 ** -34, 3 * 2.0 ** -33, 2.0 ** -40, 2.0 ** -149, 0.75)


def _ap_prob_grid():
    # rint(float64(prob) * 2^32) (eval_ap.hip:198): 0, -0.0, 1, 1 - 2^-24, the half-way cases 2^-33 (0.5 -> 0) and
    # 3 * 2^-33 (1.5 -> 2), 3 * 2^-34 (0.75 -> 1), and values under 2^-33 down to the smallest denormal.  Prediction j
    # (j < 10) holds 50 + j points of grid value j alone, predictions 10.. mix all of them.
    rng = np.random.default_rng(86)
    grid = np.asarray(PROB_GRID, F64).astype(F32)
    ps, prob = [], []
    for j in range(len(grid)):
        ps += [j] * (50 + j)
        prob += [grid[j]] * (50 + j)
    k = 1200
    ps += rng.integers(len(grid), len(grid) + 4, k).tolist()
    prob += grid[rng.integers(0, len(grid), k)].tolist()
    ps, prob = np.asarray(ps), np.asarray(prob, F32)
    perm = rng.permutation(len(ps))
    ps, prob = ps[perm], prob[perm]
    g = ps // 2
    return ApCase("prob_grid", [_scene(g % 17 + 2, g, g % 17, ps, prob)], "mean_prob", True, dict(grid=grid))


def _ap_first_class():
    # a prediction's class is the label of its first point: prediction 0's first point carries 18 (gen_ps's background)
    # and the rest 3, so it is dropped; prediction 1's first point carries 3 and the rest 18: kept, as class 4
    n = 400
    ps = np.repeat([0, 1, 2], [150, 150, 100])
    ps_sem = np.repeat([3, 18, 3], [150, 150, 100])
    ps_sem[0], ps_sem[150] = 18, 3
    g = np.repeat([0, 1, 2], [150, 150, 100])
    return ApCase("first_class", [_scene(np.full(n, 3 + 2), g, ps_sem, ps)], "one", True, {})


def _ap_big_int64():
    # int64 labels beyond the int32 range: inst = -2^40 is void (2^40 is refused, see AP_REFUSALS)
    sc = dict(_ap_random(87, 1500, 6, 6, gt_dtype=np.int64))
    ins = sc["instance_label"].copy()
    ins[100:180] = -2 ** 40
    sc["instance_label"] = ins
    return ApCase("big_int64", [_freeze(sc)], "mean_prob", True, dict(void=(100, 180)))


def _ap_truncation():
    # float64 GT labels with fractions are truncated: inst 4.9 is 4, raw class 5.5 is 5
    sc = dict(_ap_random(88, 1200, 9, 9))
    sc["instance_label"] = sc["instance_label"] + 0.9
    sc["semantic_label"] = sc["semantic_label"] + 0.5
    return ApCase("truncation", [_freeze(sc)], "mean_prob", True, {})


AP_CASES = OrderedDict([
    ("size_ladder", _ap_size_ladder),
    ("mix4", _ap_mix4),
    ("key_bits", _ap_key_bits),
    ("id_edges", _ap_id_edges),
    ("no_remap", _ap_no_remap),
    ("wide_max_ps", _ap_wide_max_ps),
    ("prob_grid", _ap_prob_grid),
    ("first_class", _ap_first_class),
    ("big_int64", _ap_big_int64),
    ("truncation", _ap_truncation),
])
AP_DTYPE_CASES = OrderedDict([("key_bits", _ap_key_bits), ("id_edges", _ap_id_edges)])
GT_DTYPES = (np.float64, np.int32, np.int64)


@lru_cache(maxsize=None)
def ap_case(name, gt_dtype=None):
    return AP_CASES[name]() if gt_dtype is None else AP_DTYPE_CASES[name](gt_dtype)


def ap_scene_reference(sc, confidence, remap, **mistake):
    return ap_tables_reference(*(sc[k] for k in FIELDS), confidence=confidence, remap=remap, max_ps=sc.get("max_ps"),
                               **mistake)


@lru_cache(maxsize=None)
def ap_expected(name, gt_dtype=None):
    case = ap_case(name, gt_dtype)
    return [ap_scene_reference(sc, case.confidence, case.remap) for sc in case.scenes]


# refusals: range checks BEFORE any table is addressed (eval_ap.hip:62,177,183).  name -> (field, value, max_ps or None)
AP_REFUSALS = OrderedDict([
    ("inst_999", ("instance_label", 999, None)),
    ("inst_2_pow_40", ("instance_label", 2 ** 40, None)),
    ("ps_minus_one", ("ps_instance_label", -1, None)),
    ("ps_equals_max_ps", ("ps_instance_label", "max_ps", "max_ps")),
    ("prob_above_one", ("ps_prob", np.nextafter(F32(1), F32(2)), None)),
    ("prob_below_zero", ("ps_prob", F32(-1e-45), None)),
    ("prob_nan", ("ps_prob", F32(np.nan), None)),
])


@lru_cache(maxsize=None)
def refusal_scenes(name):
    """(good, bad, good2): ``bad`` is ``good`` with one labelled point's value replaced."""
    field, value, cap = AP_REFUSALS[name]
    good = dict(_ap_random(90, 1200, 5, 6, gt_dtype=np.int64))
    good2 = _ap_random(91, 700, 4, 3, gt_dtype=np.int64)
    max_ps = int(good["ps_instance_label"].max()) + 1
    bad = dict(good)
    a = good[field].copy()
    at = int(np.flatnonzero(good["ps_instance_label"] >= 0)[17])
    a[at] = max_ps if isinstance(value, str) else value
    bad[field] = a
    if cap:
        bad["max_ps"] = max_ps
    return _freeze(good), _freeze(bad), good2
