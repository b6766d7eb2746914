"""The inputs of test_eval_edges_gpu.py really are what eval_cases.py claims (no device), and its references restate the
reference:
1. every case has the property its builder names, so that nothing in the GPU file passes vacuously;
2. on every case the NumPy references equal oracle/eval_oracle.py bit for bit (row 0, and each threshold on the points
   filtered beforehand) and ap_tally.tally field by field;
3. each mistake switch makes the case built for it fail;
4. evaluate_scenes' row permutation for duplicate and unsorted thresholds against a direct computation."""
import contextlib
import types

import numpy as np
import pytest
import torch

import eval_cases as ec
from ap_tally import tally
from oracle import eval_oracle as E

ALL_EVAL = list(ec.IOU_CASES) + list(ec.CONF_CASES)


def _bins(prob, taus):
    """Thresholds passed per point: the kernel's bin."""
    b = np.zeros(len(prob), np.int64)
    for t in taus:
        b += np.asarray(prob, np.float32) >= np.float32(t)
    return b


def _first(mask):
    idx = np.flatnonzero(mask)
    return int(idx[0]) if len(idx) else None


def _rows_equal(a, b):
    return len(a) == len(b) and all(
        x.ious.dtype == y.ious.dtype and x.ious.shape == y.ious.shape
        and np.array_equal(x.ious.view(np.uint32), y.ious.view(np.uint32)) and np.array_equal(x.conf, y.conf)
        and x.kept == y.kept for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------ 1. eval_batch cases
def test_constants_sit_where_the_kernels_put_them():
    assert ec.AP_CODES == 18000 and ec.AP_WORDS * 32 - ec.AP_CODES == 16   # the last word's bits from 16 on are padding
    assert -(-ec.AP_WORDS // ec.THREADS) == ec.RANK_WORDS_PER_THREAD
    assert -(-ec.AP_WORDS // ec.RANK_WORDS_PER_THREAD) == 188      # k_ap_rank's threads from 188 on have no word
    assert ec.EVB_LADDER == (0, 1, 255, 256, 257, 1024, 1025, 0, 131073)
    assert ec.AP_LADDER == (0, 1, 255, 256, 257, 2048, 2049, 0, 262145)


@pytest.mark.parametrize("name", ALL_EVAL)
def test_eval_cases_are_what_they_claim(name):
    case = ec.eval_case(name)
    C, K = case.num_classes, len(case.thresholds)
    B = K + 1
    assert K <= ec.MAX_THRESHOLDS
    for sc in case.scenes:
        n = len(sc["semantic_label"])
        assert all(len(sc[f]) == n for f in ec.FIELDS) and sc["ps_prob"].dtype == np.float32
        sem, ins, ps_sem, ps_ins = ec.scene_ints(sc, 1 if case.remap else 0)
        assert ec.conf_in_range(sem, ps_sem, C)                     # the reference itself is defined on every point
        if n:
            assert ins.max() < sc.get("max_gt", 1 << 30) and ps_ins.max() < sc.get("max_ps", 1 << 30)
    sc = case.scenes[-1]
    sem, ins, ps_sem, ps_ins = ec.scene_ints(sc, 1 if case.remap else 0)
    prob = sc["ps_prob"]
    rows = ec.eval_expected(name)[-1]
    b = _bins(prob, case.thresholds)
    if name == "size_ladder":
        assert tuple(len(s["semantic_label"]) for s in case.scenes) == ec.EVB_LADDER
        per_wg = ec.THREADS * ec.EVB_PER_THREAD
        assert -(-1024 // per_wg) == 1 and -(-1025 // per_wg) == 2 and -(-131073 // per_wg) == ec.EVB_GRID_CAP + 1
        for s, r in zip(case.scenes, ec.eval_expected(name)):
            if len(s["semantic_label"]):  # the last point alone holds ids of its own, and they give one IoU row
                gi, pi = ec.to_int(s["instance_label"]), ec.to_int(s["ps_instance_label"])
                assert (gi == 7).sum() == 1 and gi[-1] == 7 and (pi == 9).sum() == 1 and pi[-1] == 9
                assert r[0].ious[-1] == np.float32(1.0) / np.float32(np.float32(1.0) + np.float32(1e-4))
            else:
                assert all(len(x.ious) == 0 and x.kept == 0 and not x.conf.any() for x in r)
    if name.startswith("pair_"):
        cells = B * (sc["max_gt"] + 1) * (sc["max_ps"] + 1)
        want = {"pair_8192": 8192, "pair_8256": 8256, "pair_b2_4096": 8192, "pair_b2_over": 8320}[name]
        assert cells == want == case.meta["cells"] and (cells <= ec.PAIR_LDS) == (name in ("pair_8192", "pair_b2_4096"))
        other = ec.eval_case({"pair_8192": "pair_8256", "pair_8256": "pair_8192", "pair_b2_4096": "pair_b2_over",
                              "pair_b2_over": "pair_b2_4096"}[name]).scenes[0]
        assert all(np.array_equal(sc[f], other[f]) for f in ec.FIELDS)     # the same points on both sides
        # the last cell of the last bin is used: the largest ids at a point of the last bin
        last = (ins == sc["max_gt"] - 1) & (b == K)
        assert (ps_ins[last] == min(sc["max_ps"], 127 if K == 0 else 63) - 1).any()
    if name == "first_straddle":
        cap = case.meta["cap"]
        assert B == 3 and all(s["max_gt"] == s["max_ps"] == cap for s in case.scenes)
        assert 0 * cap + cap - 1 < ec.ID_LDS and 2 * cap >= ec.ID_LDS           # bin 0 in LDS, bin 2 in global memory
        assert [i for i in ec.STRADDLE_IDS if 1 * cap + i < ec.ID_LDS] == [210, 211]
        assert [i for i in ec.STRADDLE_IDS if 1 * cap + i >= ec.ID_LDS] == [212, 213, 214]
        for s, r in zip(case.scenes, ec.eval_expected(name)):
            gi, pi = ec.to_int(s["instance_label"]), ec.to_int(s["ps_instance_label"])
            bb = _bins(s["ps_prob"], case.thresholds)
            assert np.array_equal(gi, pi) and gi.max() == cap - 1
            gt_sem, _, pss, _ = ec.scene_ints(s, 1)
            present = sorted(set(gi.tolist()))
            for i in ec.STRADDLE_IDS:
                f = [_first((gi == i) & (bb == k)) for k in range(3)]
                assert None not in f                                            # points in all three bins
                if i % 2 == 0:   # rows 0 and 1 must take bin 2's first point
                    assert f[2] < f[1] < f[0]
                    want = [True, True, True]
                else:            # row 0 takes bin 1's, row 1 keeps its own, row 2 is another class
                    assert f[1] < f[0] < f[2]
                    want = [True, True, False]
                for t in range(3):
                    first = min(f[t:])
                    assert (gt_sem[first] == pss[first]) == want[t]
                    others = np.flatnonzero((gi == i) & (bb >= t))
                    assert (gt_sem[others[others != first]] != pss[others[others != first]]).all()
                    kept_ids = sorted(set(gi[bb >= t].tolist()))
                    assert (r[t].ious[kept_ids.index(i)] > 0) == want[t]
            assert len(r[0].ious) == len(present)
    if name == "first_alone":
        idx0 = np.flatnonzero(ins == 0)
        assert idx0[0] == 0 and idx0[1] > ec.THREADS * ec.EVB_PER_THREAD and len(idx0) > 100
        assert sem[0] != sem[idx0[1]] and (sem[idx0[1:]] == sem[idx0[1]]).all()
        assert np.array_equal(np.flatnonzero(ps_ins == 0), idx0) and (ps_sem[idx0] == sem[0]).all()
        assert np.flatnonzero(ins == 1).tolist() == [len(ins) - 1] == np.flatnonzero(ps_ins == 1).tolist()
        assert rows[0].ious[0] > 0.99 and rows[0].ious[1] > 0.99
    if name == "first_filtered":
        for i, at in zip((0, 1), case.meta["first"]):
            idx = np.flatnonzero(ins == i)
            assert idx[0] == at and prob[at] < np.float32(0.5) and (prob[idx[1:]] >= np.float32(0.5)).all()
            assert rows[0].ious[i] == 0 and rows[1].ious[i] > 0.99
        assert sem[100] != sem[101] and ps_sem[400] != ps_sem[401]
    if name == "thr_ties":
        vals = ec.tie_values()
        for j, t in enumerate(ec.TIE_TAUS):
            lo, at, hi = vals[3 * j:3 * j + 3]
            assert lo < at < hi and at == np.float32(t)
            assert np.nextafter(lo, np.float32(1)) == at and np.nextafter(at, np.float32(2)) == hi
            for v in (lo, at, hi):
                assert (prob == v).sum() == 20
            assert rows[j + 1].kept == int((vals >= np.float32(t)).sum()) * 20
        assert float(np.float32(0.9)) < 0.9                                # the float64 comparison drops the tie
    if name == "thr_equal":
        assert case.thresholds == (0.7, 0.7, 0.3, 0.7)
        assert _rows_equal([rows[1]] * 3, [rows[1], rows[2], rows[4]]) and rows[3].kept > rows[1].kept > 0
    if name == "thr_outside":
        assert case.thresholds == (-1.0, 0.0, 1.0, 1.5, float("inf"))
        n = len(prob)
        assert np.isnan(prob).sum() == 1 and (prob == 0).sum() >= 30 and (prob == 1).sum() == 30
        assert [r.kept for r in rows] == [n, n - 1, n - 1, 30, 0, 0]
        assert len(rows[0].ious) == len(rows[1].ious) + 1                  # the NaN point's id is in row 0 only
        assert len(rows[4].ious) == len(rows[5].ious) == 0 and not rows[5].conf.any()
    if name == "thr_max":
        assert K == ec.MAX_THRESHOLDS and len(set(np.float32(case.thresholds).tolist())) == K
        assert sorted(set(b.tolist())) == list(range(K + 1))               # every one of the 33 bins holds points
        assert ins.max() + 1 == 40 and 12 * 40 + 39 >= ec.ID_LDS > 12 * 40 and ins.max() > ec.ID_LDS // B
        assert len({r.kept for r in rows}) == B
    if name == "truncation":
        raw = sc["instance_label"]
        assert raw.dtype == np.float64 and raw[:4].tolist() == [2.9, 3.0, 3.999, -0.5]
        assert ins[:4].tolist() == [2, 3, 3, 0] and sem[3] == 0 and not case.remap
        assert (raw != np.trunc(raw)).any() and (sc["semantic_label"] != np.trunc(sc["semantic_label"])).any()
        assert np.array_equal(ins, case.meta["ids"]) and (rows[0].ious > 0.99).all() and len(rows[0].ious) == 6
    if name == "no_ids":
        assert (ins < 0).all() and (ps_ins < 0).all() and all(len(r.ious) == 0 for r in rows) and rows[0].conf.any()
    if name == "one_each":
        assert set(ins.tolist()) == {0, -100} == set(ps_ins.tolist()) and len(rows[0].ious) == 1
    if name in ("c19_k4", "c19_k5"):
        assert C == 19 and case.meta["bins"] == B * C * C
        assert (B * C * C <= ec.CONF_LDS) == (name == "c19_k4") and 5 * 361 <= ec.CONF_LDS < 6 * 361
        a, c5 = ec.eval_case("c19_k4"), ec.eval_case("c19_k5")
        assert all(np.array_equal(a.scenes[0][f], c5.scenes[0][f]) for f in ec.FIELDS)
        assert c5.thresholds[:4] == a.thresholds
        assert rows[0].conf[18, 18] > 0 and all(r.kept > 0 for r in rows)
    if name.startswith("classes_"):
        assert B == 1 and case.meta["bins"] == C * C and (C * C <= ec.CONF_LDS) == (C <= 45)
        assert rows[0].conf[C - 1, C - 1] > 0 and rows[0].conf.sum() == (sem != -100).sum()
    if name == "gt_void":
        assert (sem == -100).sum() >= len(sem) // 3 and rows[0].conf.sum() == (sem != -100).sum()
    if name == "ps_void":
        none = ps_sem == -100
        for g, want in ((0, 1), (17, 18), (18, 17)):
            assert rows[0].conf[g, want] == (none & (sem == g)).sum() > 0
        assert np.array_equal(sem, case.meta["gt"])


def test_a_33rd_threshold_is_refused_before_any_device_work():
    from gapro_amd.eval_ps_labels import evaluate_scenes

    sc = ec.writable(ec.eval_case("thr_max").scenes[0])
    with pytest.raises(ValueError, match="at most 32"):
        evaluate_scenes([sc], prob_thresholds=ec.THR_MAX_TAUS + (0.99,))


# ------------------------------------------------------------------------------------------ 2. references = oracle
def _oracle_row(sc, mask, remap, C):
    """oracle/eval_oracle.py on the points filtered beforehand, labels cast as the reference's main() casts them."""
    sem = torch.from_numpy(np.asarray(sc["semantic_label"])[mask]).int()
    if remap:
        sem[sem != -100] -= 2
        sem[(sem == -1) | (sem == -2)] = 18
    ins = torch.from_numpy(np.asarray(sc["instance_label"])[mask]).int()
    ps_sem = torch.from_numpy(np.asarray(sc["ps_semantic_label"])[mask]).int()
    ps_ins = torch.from_numpy(np.asarray(sc["ps_instance_label"])[mask]).int()
    if len(sem) == 0:
        return None
    return (E.get_miou_scene(sem.long(), ins.long(), ps_sem.long(), ps_ins.long()).numpy(),
            E.get_scene_sem_conf(sem.long(), ps_sem.long(), C).numpy())


@pytest.mark.parametrize("name", ALL_EVAL)
def test_eval_references_equal_the_oracle(name):
    case = ec.eval_case(name)
    for sc, rows in zip(case.scenes, ec.eval_expected(name)):
        n = len(sc["semantic_label"])
        masks = [np.ones(n, bool)] + [np.asarray(sc["ps_prob"]) >= np.float32(t) for t in case.thresholds]
        assert len(rows) == len(masks)
        for row, m in zip(rows, masks):
            assert row.kept == m.sum() and row.ious.dtype == np.float32 and row.conf.dtype == np.int64
            got = _oracle_row(sc, m, case.remap, case.num_classes)
            if got is None:
                assert len(row.ious) == 0 and not row.conf.any()
                continue
            assert got[0].dtype == np.float32
            np.testing.assert_array_equal(row.ious.view(np.uint32), got[0].view(np.uint32))
            np.testing.assert_array_equal(row.conf, got[1])


# ------------------------------------------------------------------------------------------ 3. the mistakes
# the named case built for each mistake (others may see it too)
MIOU_DETECTORS = {
    "class_majority": ("first_alone", "first_straddle"), "class_last": ("first_alone", "first_straddle"),
    "class_first_unfiltered": ("first_filtered", "first_straddle"),
    "strict_compare": ("thr_ties",), "float64_threshold": ("thr_ties",), "labels_rounded": ("truncation",),
    "rows_keep_bins_above": ("thr_equal", "c19_k5"), "rows_shifted_by_one": ("thr_equal", "thr_outside"),
    "equal_thresholds_collapsed": ("thr_equal",), "remap_left_out": ("ps_void", "one_each"),
    "remap_twice": ("ps_void", "one_each"),
}


def test_every_eval_mistake_has_a_detector():
    assert set(MIOU_DETECTORS) == set(ec.MIOU_MISTAKES)


@pytest.mark.parametrize("mistake", list(ec.MIOU_MISTAKES))
def test_eval_cases_detect_their_mistake(mistake):
    for name in MIOU_DETECTORS[mistake]:
        case = ec.eval_case(name)
        wrong = [ec.rows_reference(sc, case.thresholds, case.remap, case.num_classes, **ec.MIOU_MISTAKES[mistake])
                 for sc in case.scenes]
        right = ec.eval_expected(name)
        assert not all(_rows_equal(a, b) for a, b in zip(wrong, right)), name


def test_floor_is_told_from_truncation_too():
    case = ec.eval_case("truncation")
    wrong = ec.rows_reference(case.scenes[0], (), False, 19, labels="floor")
    assert not _rows_equal(wrong, ec.eval_expected("truncation")[0])


# ------------------------------------------------------------------------------------------ 4. the row permutation
@pytest.mark.parametrize("taus", [(0.7, 0.7, 0.3, 0.7), (0.9, 0.1, 0.9, 0.5, 0.1), (0.2,), ()])
def test_evaluate_scenes_row_permutation(monkeypatch, taus):
    """evaluate_scenes hands the kernel ascending thresholds and maps its rows back to the caller's order: with the
    launch replaced by the NumPy reference in the kernel's row layout, every row must be the direct computation."""
    from gapro_amd import eval_ps_labels as P

    scenes = [ec.writable(ec.eval_case(n).scenes[0]) for n in ("thr_equal", "one_each")]
    seen = {}

    def fake(dev, sizes, sem, ins, ps_sem, ps_ins, prob=None, thresholds=(), scannet_remap=False, num_classes=19):
        thr = [float(t) for t in thresholds]
        assert thr == sorted(thr) and np.asarray(thresholds).dtype == np.float32
        seen["thr"] = thr
        B = len(thr) + 1
        descs, iou, cls, off, row_off = [], [], [], 0, 0
        conf = np.zeros((B, num_classes, num_classes), np.int64)
        kept = np.zeros((len(sizes), B), np.int64)
        for i, (n, max_gt, _) in enumerate(sizes):
            sc = dict(zip(ec.FIELDS, (t[off:off + n].numpy() for t in (sem, ins, ps_sem, ps_ins))))
            sc["ps_prob"] = prob[off:off + n].numpy() if prob is not None else None
            rows = ec.rows_reference(sc, thr, scannet_remap, num_classes)
            for r, row in enumerate(rows):
                a, c = np.zeros(max_gt, np.float32), np.full(max_gt, -1.0, np.float32)
                a[:len(row.ious)], c[:len(row.ious)] = row.ious, 0.0
                iou.append(a), cls.append(c)
                conf[r] += row.conf
                kept[i, r] = row.kept
            descs.append(types.SimpleNamespace(max_gt=max_gt, row_offset=row_off))
            off, row_off = off + n, row_off + B * max_gt
        return (descs, torch.from_numpy(np.concatenate(iou)), torch.from_numpy(np.concatenate(cls)),
                torch.from_numpy(conf), torch.from_numpy(kept))

    monkeypatch.setattr(P, "_eval_batch", fake)
    monkeypatch.setattr(P, "_cat", lambda ts, dtype, dev: torch.cat([t.to(dtype) for t in ts]))
    monkeypatch.setattr(P.torch.cuda, "device", lambda dev: contextlib.nullcontext())
    res = P.evaluate_scenes(scenes, prob_thresholds=taus, device="cuda:0")
    assert seen["thr"] == sorted(float(np.float32(t)) for t in taus)
    assert res.thresholds == tuple(float(np.float32(t)) for t in taus)
    conf = np.zeros((len(taus) + 1, 19, 19), np.int64)
    for i, sc in enumerate(scenes):
        want = ec.rows_reference(sc, taus)           # in the caller's order, each row filtered directly
        for r, row in enumerate(want):
            np.testing.assert_array_equal(res.ious[i][r].view(np.uint32), row.ious.view(np.uint32))
            assert res.kept[i, r] == row.kept
            conf[r] += row.conf
    np.testing.assert_array_equal(res.conf, conf)


# ------------------------------------------------------------------------------------------ 1. eval_ap cases
def _n_keys(table):
    return len(table.gt_code)


@pytest.mark.parametrize("name", list(ec.AP_CASES))
def test_ap_cases_are_what_they_claim(name):
    case, want = ec.ap_case(name), ec.ap_expected(name)
    for sc in case.scenes:
        assert all(len(sc[f]) == len(sc["semantic_label"]) for f in ec.FIELDS) and sc["ps_prob"].dtype == np.float32
    t = want[-1]
    sc = case.scenes[-1]
    if name == "size_ladder":
        assert tuple(len(s["semantic_label"]) for s in case.scenes) == ec.AP_LADDER
        per_wg = ec.THREADS * ec.AP_PER_THREAD
        assert -(-2048 // per_wg) == 1 and -(-2049 // per_wg) == 2 and -(-262145 // per_wg) == ec.AP_GRID_CAP + 1
        for s, w in zip(case.scenes, want):
            if len(s["semantic_label"]):  # the last point alone: GT instance 8901 and prediction 7, one pair of one point
                assert w.gt_code[-1] == 8901 and w.gt_n[-1] == 1 and w.pred_id[-1] == 7 and w.pred_n[-1] == 1
                assert (w.pair_gt[-1], w.pair_pred[-1], w.pair_inter[-1]) == (len(w.gt_code) - 1, len(w.pred_id) - 1, 1)
            else:
                assert all(len(getattr(w, f)) == 0 for f in ec.ApRef._fields)
    if name == "mix4":
        got = []
        for s, w, (n_keys, max_ps) in zip(case.scenes, want, ec.MIX4):
            assert _n_keys(w) == n_keys and s["max_ps"] == max_ps and s["ps_instance_label"].max() == max_ps - 1
            cells = (n_keys + 1) * (max_ps + 1)
            got.append((cells, cells <= ec.PAIR_LDS, max_ps <= ec.ID_LDS))
        assert got == [(8192, True, True), (8256, False, True), (8193, False, False), (7695, True, True),
                       (7710, True, False)]
        assert 16 * 513 > ec.PAIR_LDS   # why the id split is taken with 14 keys: 15 would leave the LDS pair table
    if name == "key_bits":
        idx = [ec.key_index(c // 1000, c % 1000 - 1) for c in t.gt_code.tolist()]
        assert idx == sorted(ec.KEY_BITS) and np.all(np.diff(t.gt_code) > 0)
        where = [(k >> 5, k & 31) for k in idx]
        assert where[:6] == [(0, 0), (0, 31), (1, 8), (1, 9), (1, 0), (1, 31)] or \
            where[:6] == [(0, 0), (0, 31), (1, 0), (1, 8), (1, 9), (1, 31)]
        assert (561, 31) in where and where[-1] == (ec.AP_WORDS - 1, 15) and idx[-1] == ec.AP_CODES - 1
        assert t.gt_code[-1] == 18999 and t.gt_code[idx.index(999)] == 1999 and t.gt_code[idx.index(1000)] == 2000
        assert sorted(t.gt_n.tolist()) == [10 + 3 * j for j in range(10)]
        assert {1, 2, 18} <= set(t.pred_label.tolist()) and {0, len(idx) - 1} <= set(t.pair_gt.tolist())
    if name == "id_edges":
        legal = sorted((raw - 1) * 1000 + inst + 1 for raw, inst, _, ok in ec.ID_EDGES if ok)
        assert t.gt_code.tolist() == legal == [2000, 2001, 2999, 3000, 18000, 18998, 18999]
        assert t.gt_n.tolist() == [30, 31, 32, 29, 34, 33, 28]   # class 2's inst 998 and class 3's inst -1 are neighbours
        assert t.pred_void.sum() == sum(k for _, _, k, ok in ec.ID_EDGES if not ok) and len(t.pred_id) == len(ec.ID_EDGES)
    if name == "no_remap":
        sem = ec.to_int(sc["semantic_label"])
        assert not case.remap and {18, 19, -100} <= set(sem.tolist()) and len(t.pair_gt) >= 5
        assert set((t.gt_code // 1000).tolist()) == set(range(1, 19))
    if name == "wide_max_ps":
        for s, d, w in zip(case.scenes, case.meta["default"], want):
            assert s["max_ps"] >= 3 * (int(s["ps_instance_label"].max()) + 1) and "max_ps" not in d
            assert ec.tables_equal(w, ec.ap_scene_reference(d, case.confidence, case.remap))
        assert want[1].pred_id.max() < ec.ID_LDS < case.scenes[1]["max_ps"]
    if name == "prob_grid":
        grid = case.meta["grid"]
        assert grid.dtype == np.float32 and np.signbit(grid[1]) and grid[1] == 0 and grid[8] > 0
        assert grid[3] == np.nextafter(np.float32(1), np.float32(0)) and grid[4] * 2.0 ** 32 == 0.5
        assert grid[5] * 2.0 ** 32 == 0.75 and grid[6] * 2.0 ** 32 == 1.5
        exact = [0.0, 0.0, 1.0, 1.0 - 2.0 ** -24, 0.0, 2.0 ** -32, 2.0 ** -31, 0.0, 0.0, 0.75]
        assert t.pred_id[:10].tolist() == list(range(10)) and t.pred_conf[:10].tolist() == exact
        assert t.pred_n[:10].tolist() == [50 + j for j in range(10)] and len(t.pred_id) == 14
    if name == "first_class":
        ps_sem = sc["ps_semantic_label"]
        assert ps_sem[0] == 18 and (ps_sem[1:150] == 3).all() and ps_sem[150] == 3 and (ps_sem[151:300] == 18).all()
        assert t.pred_id.tolist() == [1, 2] and t.pred_label.tolist() == [4, 4]
    if name == "big_int64":
        ins = sc["instance_label"]
        assert ins.dtype == np.int64 and (ins[100:180] == -2 ** 40).all() and ins.min() < np.iinfo(np.int32).min
        assert t.pred_void.sum() >= 60
    if name == "truncation":
        assert sc["instance_label"].dtype == np.float64 and (sc["instance_label"] % 1 != 0).all()
        assert (sc["semantic_label"] % 1 != 0).all() and len(t.pair_gt) > 5


@pytest.mark.parametrize("name", list(ec.AP_DTYPE_CASES))
def test_ap_dtype_variants_hold_the_same_labels(name):
    base = ec.ap_expected(name)
    for dt in ec.GT_DTYPES:
        case = ec.ap_case(name, dt)
        assert case.scenes[0]["instance_label"].dtype == dt == case.scenes[0]["semantic_label"].dtype
        assert all(ec.tables_equal(a, b) for a, b in zip(ec.ap_expected(name, dt), base))


@pytest.mark.parametrize("name", list(ec.AP_REFUSALS))
def test_ap_refusal_inputs_are_refused_for_one_point(name):
    good, bad, good2 = ec.refusal_scenes(name)
    field = ec.AP_REFUSALS[name][0]
    differ = [f for f in ec.FIELDS if not np.array_equal(good[f], bad[f], equal_nan=True)]
    assert differ == [field] and (good[field] != bad[field]).sum() == 1
    at = int(np.flatnonzero(good[field] != bad[field])[0])
    assert good["ps_instance_label"][at] >= 0                       # a labelled point
    for sc in (good, good2):
        ec.ap_scene_reference(sc, "mean_prob", True)
    with pytest.raises(ValueError):
        ec.ap_scene_reference(bad, "mean_prob", True)
    if name == "prob_above_one":
        assert bad[field][at] == np.float32(1) + np.float32(2.0 ** -23)
    if name == "prob_below_zero":
        assert bad[field][at] < 0 and bad[field][at] == -np.float32(2.0 ** -149)
    if name == "ps_equals_max_ps":
        assert bad[field][at] == bad["max_ps"] == good[field].max() + 1


# ------------------------------------------------------------------------------------------ 2. AP reference = ap_tally
@pytest.mark.parametrize("name", list(ec.AP_CASES))
def test_ap_reference_equals_the_tally(name):
    case = ec.ap_case(name)
    for sc, want in zip(case.scenes, ec.ap_expected(name)):
        got = tally(*(sc[f] for f in ec.FIELDS), confidence=case.confidence, remap=case.remap)
        for f in ec.ApRef._fields:
            x, y = np.asarray(getattr(got, f)), np.asarray(getattr(want, f))
            assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y), (name, f)


# ------------------------------------------------------------------------------------------ 3. the AP mistakes
AP_DETECTORS = {
    "inst_minus_one_void": ("id_edges", "key_bits"), "class_19_instance": ("id_edges",),
    "remap_left_out": ("id_edges",), "remap_twice": ("id_edges",), "mean_in_float32": ("prob_grid",),
    "pred_class_majority": ("first_class",), "labels_rounded": ("truncation",),
}


@pytest.mark.parametrize("mistake", list(ec.AP_MISTAKES))
def test_ap_cases_detect_their_mistake(mistake):
    kw = ec.AP_MISTAKES[mistake]
    if mistake == "inst_999_legal":   # told by the refusal: with the mistake nothing is raised
        _, bad, _ = ec.refusal_scenes("inst_999")
        wrong = ec.ap_scene_reference(bad, "mean_prob", True, **kw)
        assert 1000 in (wrong.gt_code % 1000).tolist() or len(wrong.gt_code)   # the id has carried into the class digit
        with pytest.raises(ValueError):
            ec.ap_scene_reference(bad, "mean_prob", True)
        return
    for name in AP_DETECTORS[mistake]:
        case = ec.ap_case(name)
        wrong = [ec.ap_scene_reference(sc, case.confidence, case.remap, **kw) for sc in case.scenes]
        assert not all(ec.tables_equal(a, b) for a, b in zip(wrong, ec.ap_expected(name))), name
