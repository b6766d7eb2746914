"""A plain NumPy restatement of the per-scene AP tables (assign_instances_for_scan of ISBNet's ScanNetEval, driven as
the reference's eval_ap_ps_labels.py does), for the AP tests: what gapro_amd.eval_ap_ps_labels.ap_tables must return,
bit for bit."""
import os

import numpy as np

from gapro_amd.eval_ap_ps_labels import ApTable

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def tally(sem_gt, inst_gt, ps_sem, ps_inst, prob=None, confidence="one", remap=True):
    sem = np.asarray(sem_gt).astype(np.int64)  # float64 labels: truncation
    ins = np.asarray(inst_gt).astype(np.int64)
    ps_sem = np.asarray(ps_sem).astype(np.int64)
    ps = np.asarray(ps_inst).astype(np.int64)
    if remap:  # eval_ap_ps_labels.py:59-60
        sem = np.where(sem != -100, sem - 2, sem)
        sem[(sem == -1) | (sem == -2)] = 18
    assert not (ins >= 999).any() and not ((ps < 0) & (ps != -100)).any()
    # assign_instances_for_scan's encoding: class (sem + 1) in 1..18, inst + 1 >= 0, else void
    inst_ok = (sem >= 0) & (sem < 18) & (ins >= -1)
    code = (sem + 1) * 1000 + ins + 1
    gt_code, gt_of_point = np.unique(code[inst_ok], return_inverse=True)
    gt_n = np.bincount(gt_of_point, minlength=len(gt_code))
    ids, first, n = np.unique(ps, return_index=True, return_counts=True)
    label = ps_sem[first] + 1
    keep = (ids != -100) & (label >= 1) & (label <= 18)
    ids, first, n, label = ids[keep], first[keep], n[keep], label[keep]
    pred_of_point = np.full(len(ps), -1)
    pred_of_point[np.isin(ps, ids)] = np.searchsorted(ids, ps[np.isin(ps, ids)])
    has = pred_of_point >= 0
    void = np.bincount(pred_of_point[has & ~inst_ok], minlength=len(ids))
    if confidence == "one":
        conf = np.ones(len(ids))
    else:
        q = np.rint(np.asarray(prob)[has].astype(np.float64) * 2.0 ** 32).astype(np.int64)
        s = np.zeros(len(ids), np.int64)
        np.add.at(s, pred_of_point[has], q)
        conf = s.astype(np.float64) / (n.astype(np.float64) * 2.0 ** 32)
    both = inst_ok & has
    gt_all = np.full(len(ps), -1)
    gt_all[inst_ok] = gt_of_point
    inter = np.bincount(gt_all[both] * len(ids) + pred_of_point[both],
                        minlength=len(gt_code) * len(ids)).reshape(len(gt_code), len(ids))
    inter[(gt_code // 1000)[:, None] != label[None, :]] = 0  # only GT instances of the prediction's class
    qg, qp = np.nonzero(inter)
    i64 = lambda v: np.asarray(v, dtype=np.int64)  # noqa: E731
    return ApTable(i64(gt_code), i64(gt_n), i64(ids), i64(label), i64(n), i64(void), np.asarray(conf, np.float64),
                   i64(qg), i64(qp), i64(inter[qg, qp]))


def fixture():
    return np.load(os.path.join(GOLDEN_DIR, "ap_eval.npz"))


def fixture_scenes(case):
    """The scenes of a fixture case ("golden" or "synth") as (sem_gt, inst_gt, ps_sem, ps_inst, prob) lists."""
    z = fixture()
    if case == "golden":
        out = []
        for name in z["golden"]:
            g = np.load(os.path.join(GOLDEN_DIR, str(name) + ".npz"))
            out.append([g["sem_gt"], g["inst_gt"], g["out_sem"], g["out_inst"], g["out_prob"]])
        return out
    return [[z["synth%d_%s" % (i, k)] for k in ("sem_gt", "inst_gt", "ps_sem", "ps_inst", "prob")]
            for i in range(int(z["n_synth"]))]


def assert_tables_equal(a, b):
    for f in ApTable._fields:
        x, y = np.asarray(getattr(a, f)), np.asarray(getattr(b, f))
        assert x.shape == y.shape and np.array_equal(x, y), f
        if f == "pred_conf":
            assert x.dtype == y.dtype == np.float64
