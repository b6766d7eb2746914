"""Generate tests/golden/ap_eval.npz: the reference's ScanNet instance AP of pseudo-labels on fixed inputs.

Runs the REAL ScanNetEval of the reference checkout (ISBNet/isbnet/evaluation/instance_eval.py) the way
gapro/eval_ap_ps_labels.py drives it: the script's GT remap (:59-60), one prediction per pseudo instance id other than
-100 with label_id = pseudo label of its first point + 1 (:102-127), then assign_instances_for_scan per scene,
evaluate_matches and compute_averages (evaluate() without its 16-process pool).  The script's random GT injection
(:65-96) is not part of the metric and is left out.  Needs the reference checkout; the fixture it writes is plain data.

Stubbed because they are not installed or no longer exist: isbnet.util (only rle_decode is imported; masks are passed
as arrays), plyfile (imported by instance_eval_util) and np.float (removed from NumPy).

Cases (confidence "one" = the reference's 1.0; "mean_prob" = float64(S) / (float64(n) * 2**32) with
S = sum of rint(float64(prob) * 2**32) over the instance's points):
  golden_*: the six golden scenes tests/golden/s0..s5 (sem_gt, inst_gt, out_sem, out_inst, out_prob);
  synth_*:  seeded synthetic scenes built to reach every branch of the matching (see _branch_scene).
A second file, ap_eval_edges.npz, holds the case ``edges``: two scenes that put a value ON every comparison of
evaluate_matches (see _edge_scene), so that ap_from_tables' strict and non-strict comparisons are pinned by the reference.
"""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/ISBNet"
GOLDEN = ["s0_walls", "s1_nowalls", "s2_dense", "s3_bigspp", "s4_dups", "s5_lean"]
CLASSES = ("cabinet", "bed", "chair", "sofa", "table", "door", "window", "bookshelf", "picture", "counter", "desk",
           "curtain", "refrigerator", "shower curtain", "toilet", "sink", "bathtub", "otherfurniture")
AVG_KEYS = ("all_ap", "all_ap_50%", "all_ap_25%", "all_rc", "all_rc_50%", "all_rc_25%")
CLASS_KEYS = ("ap", "ap50%", "ap25%", "rc", "rc50%", "rc25%")


def load_scannet_eval():
    np.float = float  # removed from NumPy; evaluate_matches allocates with it
    util = types.ModuleType("isbnet.util")
    util.rle_decode = lambda rle: (_ for _ in ()).throw(AssertionError("masks are passed as arrays"))
    pkg = types.ModuleType("isbnet")
    pkg.__path__ = [os.path.join(REF, "isbnet")]
    ev = types.ModuleType("isbnet.evaluation")  # the package without its __init__ (s3dis_eval needs scipy)
    ev.__path__ = [os.path.join(REF, "isbnet", "evaluation")]
    sys.modules.update({"isbnet": pkg, "isbnet.util": util, "isbnet.evaluation": ev,
                        "plyfile": types.ModuleType("plyfile")})
    sys.modules["plyfile"].PlyData = None
    return importlib.import_module("isbnet.evaluation.instance_eval").ScanNetEval


def mean_prob(prob, idx):
    s = np.rint(prob[idx].astype(np.float64) * 2.0 ** 32).astype(np.int64).sum()
    return np.float64(s) / (np.float64(len(idx)) * 2.0 ** 32)


def reference_ap(ScanNetEval, scenes, confidence):
    ev = ScanNetEval(CLASSES, dataset_name="scannetv2")
    matches = {}
    for si, (sem_gt, inst_gt, ps_sem, ps_inst, prob) in enumerate(scenes):
        sem = np.array(sem_gt, copy=True)
        sem[sem != -100] -= 2  # :59-60
        sem[(sem == -1) | (sem == -2)] = 18
        preds = []
        for uid in np.unique(ps_inst):  # :99-127
            if uid == -100:
                continue
            ind_ = np.nonzero(ps_inst == uid)[0]
            mask_ = np.zeros(len(ps_inst), dtype=bool)
            mask_[ind_] = 1
            conf = 1.0 if confidence == "one" else mean_prob(prob, ind_)
            preds.append(dict(scan_id="scene%04d_00" % si, conf=conf, label_id=ps_sem[ind_[0]] + 1, pred_mask=mask_))
        gt2pred, pred2gt = ev.assign_instances_for_scan(preds, sem, np.array(inst_gt, copy=True))
        matches["gt_%d" % si] = dict(gt=gt2pred, pred=pred2gt)
    ap, rc = ev.evaluate_matches(matches)
    avgs = ev.compute_averages(ap, rc)
    return (ap[0], rc[0], np.array([avgs[k] for k in AVG_KEYS], np.float64),
            np.array([[avgs["classes"][c][k] for k in CLASS_KEYS] for c in CLASSES], np.float64))


class _Builder:
    """A scene as segments of points: (count, raw GT semantic, GT instance, pseudo semantic, pseudo instance, prob)."""

    def __init__(self):
        self.cols = [[] for _ in range(5)]

    def add(self, n, sem, inst, ps_sem, ps_inst, prob):
        for c, v in zip(self.cols, (sem, inst, ps_sem, ps_inst, prob)):
            c.append(np.full(n, v) if np.isscalar(v) else np.asarray(v))

    def build(self, rng, gt_dtype):
        sem, inst, ps_sem, ps_inst, prob = (np.concatenate(c) for c in self.cols)
        perm = rng.permutation(len(sem))
        return [sem[perm].astype(gt_dtype), inst[perm].astype(gt_dtype), ps_sem[perm].astype(np.int32),
                ps_inst[perm].astype(np.int32), prob[perm].astype(np.float32)]


def _branch_scene(seed):
    """Every branch: raw GT semantic r is class id r - 1 after the remap (r = 2..19), 0 / 1 and -100 are void; a
    pseudo label l is class id l + 1 (18 = background and -100 have none).  Class 15 has GT and no prediction, class
    17 neither."""
    rng = np.random.default_rng(seed)
    b = _Builder()
    u = lambda n, lo=0.5, hi=1.0: rng.uniform(lo, hi, n).astype(np.float32)  # noqa: E731
    # a clean match: GT (class 3) 300 points, pseudo 0 on 280 of them and 20 void points
    b.add(280, 4, 0, 2, 0, u(280))
    b.add(20, 4, 0, 2, -100, u(20))
    b.add(20, 0, -100, 2, 0, u(20))
    # two predictions over one GT (class 5, 400 points): pseudo 1 on 220 (IoU 0.55), pseudo 2 on 150 (0.375)
    b.add(220, 6, 1, 4, 1, 0.75)
    b.add(150, 6, 1, 4, 2, 0.75)
    b.add(30, 6, 1, -100, -100, 0.6)
    # class 7: GT 2 (400) and GT 3 (150); pseudo 3 on 200 of GT 2, pseudo 4 on 150 of GT 2 and 100 of GT 3: above 0.25
    # with both, a duplicate of GT 2 at 0.25, then GT 3's match
    b.add(200, 8, 2, 6, 3, u(200))
    b.add(150, 8, 2, 6, 4, 0.75)
    b.add(50, 8, 2, 6, -100, 0.9)
    b.add(100, 8, 3, 6, 4, 0.75)
    b.add(50, 8, 3, 18, 5, u(50))  # pseudo class 18: not a prediction
    # small GT (class 2, 90 points) under a 120-point pseudo 6 (80 of it): ignored or a false positive by threshold;
    # pseudo 7 is under 100 points
    b.add(80, 3, 9, 1, 6, u(80))
    b.add(40, 0, -100, 1, 6, u(40))
    b.add(10, 3, 9, 1, 7, u(10))
    b.add(60, 5, 20, 1, 7, u(60))
    # void overlap: pseudo 8 (class 4) 150 void + 50 of GT 10 (class 4, 400 points)
    b.add(150, 1, 4, 3, 8, u(150))
    b.add(50, 5, 10, 3, 8, u(50))
    b.add(350, 5, 10, 3, 11, u(350))
    # GT instance -1 on an object class (class 11) is an instance; pseudo 9 covers it, most of it labelled class 12
    b.add(200, 12, -1, 11, 9, u(200))
    # GT instance < -1 on an object class: void
    b.add(120, 12, -100, 11, 10, u(120))
    # one GT id on two classes (13 and 14): two GT instances; pseudo 12 on the first, pseudo 13 on the second
    b.add(150, 14, 11, 12, 12, u(150))
    b.add(150, 15, 11, 13, 13, u(150))
    # class 15: GT and no prediction; wall / floor and -100 GT under a -100 pseudo
    b.add(200, 16, 12, -100, -100, u(200))
    b.add(300, 0, 7, -100, -100, u(300))
    b.add(100, -100, -100, -100, -100, u(100))
    scene = b.build(rng, np.float64)
    # pseudo 9's first point carries class 10: the instance's class is that of its first point, not its majority
    first = np.flatnonzero(scene[3] == 9)[0]
    scene[2][first] = 9
    return scene


def _random_scene(seed, n_gt, gt_dtype):
    """GT instances of random classes and sizes; pseudo instances that keep, split, merge, shrink or relabel them, with
    probabilities in coarse steps (tied confidences)."""
    rng = np.random.default_rng(seed)
    b = _Builder()
    pid = 0
    for g in range(n_gt):
        n = int(rng.integers(40, 700))
        raw = int(rng.integers(2, 16))  # classes 1..14: class 15 keeps GT without prediction, 17 keeps neither
        fate = rng.integers(0, 5)
        ps_cls = raw - 2 if rng.random() < 0.85 else int(rng.choice([*range(14), 18]))
        p = np.round(rng.uniform(0.5, 1.0, n) * 4).astype(np.float32) / 4
        if fate == 0:    # kept
            b.add(n, raw, g, ps_cls, pid, p)
        elif fate == 1:  # split
            k = int(rng.integers(1, n))
            b.add(k, raw, g, ps_cls, pid, p[:k])
            pid += 1
            b.add(n - k, raw, g, ps_cls, pid, p[k:])
        elif fate == 2:  # merged with the next one
            b.add(n, raw, g, ps_cls, pid if g % 2 == 0 else max(pid - 1, 0), p)
        elif fate == 3:  # shrunk, rest unlabelled
            k = int(rng.integers(1, n))
            b.add(k, raw, g, ps_cls, pid, p[:k])
            b.add(n - k, raw, g, -100, -100, p[k:])
        else:            # spills into void
            b.add(n, raw, g, ps_cls, pid, p)
            b.add(int(rng.integers(10, 300)), int(rng.integers(0, 2)), -100, ps_cls, pid, 0.5)
        pid += 1
    b.add(500, 0, -100, -100, -100, 0.5)
    return b.build(rng, gt_dtype)


def _edge_scene(seed, gt_dtype):
    """Values on the comparisons of evaluate_matches (iou > th, prop_ignore <= th, >= min_region_size):"""
    rng = np.random.default_rng(seed)
    b = _Builder()
    # an IoU of exactly 0.5 (class 3): GT 0 of 300 points, pseudo 0 on 200 of them and 100 void points
    b.add(200, 4, 0, 2, 0, 0.75)
    b.add(100, 4, 0, 2, -100, 0.5)
    b.add(100, 0, -100, 2, 0, 0.75)
    # an IoU of exactly 0.25 with a prediction of exactly 100 points, all inside GT 1 of 400 points (class 4)
    b.add(100, 5, 1, 3, 1, 0.75)
    b.add(300, 5, 1, -100, -100, 0.5)
    # instances of 99 and of 100 points, GT and prediction alike (class 5): either side of min_region_size
    b.add(99, 6, 2, 4, 2, 0.5)
    b.add(100, 6, 3, 4, 3, 1.0)
    # prop_ignore exactly 0.5 (150 void + 150 on a 1000-point GT) and exactly 0.25 (100 void + 300 on a 2000-point GT)
    b.add(150, 0, -100, 5, 4, 0.75)
    b.add(150, 7, 4, 5, 4, 0.75)
    b.add(850, 7, 4, -100, -100, 0.5)
    b.add(100, 1, -100, 5, 5, 0.5)
    b.add(300, 7, 5, 5, 5, 0.5)
    b.add(1700, 7, 5, -100, -100, 0.5)
    # a prediction ignored through a same-class GT of 60 points (class 7): pseudo 6 = all of GT 6 + 60 of GT 7 (500 points)
    b.add(60, 8, 6, 6, 6, 0.75)
    b.add(60, 8, 7, 6, 6, 0.75)
    b.add(440, 8, 7, 6, 7, 1.0)
    # one prediction over two GTs at IoU 0.5 each (class 8): GT 8 and GT 9 of 200 points, pseudo 8 covers both
    b.add(200, 9, 8, 7, 8, 0.75)
    b.add(200, 9, 9, 7, 8, 0.75)
    # two predictions of equal IoU (0.5) and equal confidence on one GT of 600 points (class 9)
    b.add(300, 10, 10, 8, 9, 0.75)
    b.add(300, 10, 10, 8, 10, 0.75)
    # class 18 with inst 998, and with inst -1
    b.add(150, 19, 998, 17, 11, 1.0)
    b.add(150, 19, -1, 17, 12, 0.25)
    # wall / floor and unlabelled GT under no prediction
    b.add(600, 0, -100, -100, -100, 0.5)
    b.add(291, -100, -100, -100, -100, 0.5)
    return b.build(rng, gt_dtype)


def edge_scenes():
    return [_edge_scene(11, np.float64), _edge_scene(12, np.int64)]


def synthetic_scenes():
    return [_branch_scene(1), _random_scene(2, 25, np.int64), _random_scene(3, 40, np.float64),
            _random_scene(4, 12, np.int32)]


def golden_scenes():
    out = []
    for name in GOLDEN:
        z = np.load(os.path.join(HERE, name + ".npz"))
        out.append([z["sem_gt"], z["inst_gt"], z["out_sem"], z["out_inst"], z["out_prob"]])
    return out


def main():
    ScanNetEval = load_scannet_eval()
    synth = synthetic_scenes()
    out = dict(golden=np.array(GOLDEN), n_synth=np.int64(len(synth)))
    for i, sc in enumerate(synth):
        for k, a in zip(("sem_gt", "inst_gt", "ps_sem", "ps_inst", "prob"), sc):
            out["synth%d_%s" % (i, k)] = a
    for case, scenes in (("golden", golden_scenes()), ("synth", synth)):
        for conf in ("one", "mean_prob"):
            ap, rc, avg, cls = reference_ap(ScanNetEval, scenes, conf)
            key = "%s_%s" % (case, conf)
            out[key + "_ap"], out[key + "_rc"], out[key + "_avg"], out[key + "_cls"] = ap, rc, avg, cls
            print("%-16s AP %.4f AP50 %.4f AP25 %.4f" % (key, avg[0], avg[1], avg[2]))
    path = os.path.join(HERE, "ap_eval.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    edges = edge_scenes()
    out = dict(n_edges=np.int64(len(edges)))
    for i, sc in enumerate(edges):
        for k, a in zip(("sem_gt", "inst_gt", "ps_sem", "ps_inst", "prob"), sc):
            out["edges%d_%s" % (i, k)] = a
    for conf in ("one", "mean_prob"):
        ap, rc, avg, cls = reference_ap(ScanNetEval, edges, conf)
        key = "edges_%s" % conf
        out[key + "_ap"], out[key + "_rc"], out[key + "_avg"], out[key + "_cls"] = ap, rc, avg, cls
        print("%-16s AP %.4f AP50 %.4f AP25 %.4f" % (key, avg[0], avg[1], avg[2]))
    path = os.path.join(HERE, "ap_eval_edges.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
