"""Probability-threshold rows of the AP tables on the device (gapro_eval_ap_tables_rows behind
eval_ap_ps_labels.ap_tables_rows / evaluate_ap_rows) and the CLI's --prob_thresholds.  Row t of a scene equals
ap_tally.tally of the arrays filtered with NumPy's float32 ``prob >= tau``, bit for bit; pred_conf as equal float64.
No tolerances."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from ap_rows_cases import F32, filtered, kept_mask, own_thresholds, random_scene
from ap_tally import assert_tables_equal, fixture_scenes, tally

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("semantic_label", "instance_label", "ps_semantic_label", "ps_instance_label", "ps_prob")
BAD_ARG, WORKSPACE = -1, -7


def _check_rows(scenes, taus, conf="mean_prob", max_ps=None):
    """ap_tables_rows of the batch against the tally of every filtered scene -> the ApRows."""
    from gapro_amd.eval_ap_ps_labels import ap_tables_rows

    batch = scenes if max_ps is None else [dict(zip(FIELDS, sc), max_ps=m) for sc, m in zip(scenes, max_ps)]
    rows = ap_tables_rows(batch, taus, conf)
    assert rows.thresholds == tuple(float(F32(t)) for t in taus) and len(rows.tables) == len(taus) + 1
    assert rows.kept.shape == (len(scenes), len(taus) + 1) and rows.kept.dtype == np.int64
    for i, sc in enumerate(scenes):
        assert_tables_equal(rows.tables[0][i], tally(*sc, confidence=conf))
        assert rows.kept[i, 0] == len(sc[4])
        for j, tau in enumerate(taus, 1):
            assert_tables_equal(rows.tables[j][i], tally(*filtered(sc, tau), confidence=conf))
            assert rows.kept[i, j] == int(kept_mask(sc[4], tau).sum())
    return rows


# ------------------------------------------------------------------------------------------------ 1. fixture scenes
@pytest.mark.parametrize("gt_dt", [np.float64, np.int32, np.int64])
@pytest.mark.parametrize("ps_dt", [np.int32, np.int64])
def test_every_row_equals_the_tally_of_the_filtered_scene(gt_dt, ps_dt):
    scenes = [[sc[0].astype(gt_dt), sc[1].astype(gt_dt), sc[2].astype(ps_dt), sc[3].astype(ps_dt), sc[4]]
              for sc in fixture_scenes("golden") + fixture_scenes("synth")]
    taus = own_thresholds(scenes)
    taus = [taus[2], taus[0], taus[1]]  # in the caller's order, not ascending
    for conf in ("one", "mean_prob"):
        _check_rows(scenes, taus, conf)


# ------------------------------------------------------------------------------------------------ 2. row 0, batches
def _raw_call(scenes, taus, entry):
    """The C calls as ap_tables_rows makes them, through ``entry`` ("tables": gapro_eval_ap_workspace_bytes and
    gapro_eval_ap_tables; "rows": the _rows pair) -> (rc of pass 2, error text, [status, key_code, key_n, ps_n,
    ps_label, ps_void, ps_sum, pair] host arrays)."""
    import torch
    from gapro_amd import _lib

    ctx = _lib.Context.get(0)
    lib = ctx.lib
    S, T = len(scenes), len(taus)
    B = T + 1 if entry == "rows" else 1
    d = (_lib.EvalApScene * S)()
    off = 0
    for x, sc in zip(d, scenes):
        x.point_offset, x.n_points, x.max_ps = off, len(sc[0]), max(1, int(np.max(sc[3], initial=-1)) + 1)
        off += len(sc[0])
    dev = torch.device("cuda", 0)
    up = lambda k, dt: torch.as_tensor(np.concatenate([np.asarray(sc[k]).astype(dt) for sc in scenes])).to(dev)  # noqa: E731
    sem, ins, ps_sem, ps_ins, prob = up(0, np.float64), up(1, np.float64), up(2, np.int32), up(3, np.int32), up(4, F32)
    ws_bytes = int(lib.gapro_eval_ap_workspace_bytes_rows(d, S, T) if entry == "rows" else
                   lib.gapro_eval_ap_workspace_bytes(d, S))
    assert ws_bytes > 0
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    d_d = torch.empty(C.sizeof(d), dtype=torch.uint8, device=dev)
    n_keys = torch.empty(S, dtype=torch.int32, device=dev)
    status = torch.empty(S, dtype=torch.int32, device=dev)
    ctx.check(lib.gapro_eval_ap_keys(ctx.handle, stream, S, d, d_d.data_ptr(), off, 1, sem.data_ptr(), 1, ins.data_ptr(),
                                     1, ws.data_ptr(), ws_bytes, n_keys.data_ptr(), status.data_ptr()))
    for x, k in zip(d, n_keys.cpu().tolist()):
        x.n_keys = k
    n_cells = int(lib.gapro_eval_ap_pair_cells(d, S))
    n_k = int(d[S - 1].key_offset) + int(d[S - 1].n_keys)
    n_i = int(d[S - 1].id_offset) + int(d[S - 1].max_ps)
    i32 = lambda m: torch.full((max(B * m, 1),), -7, dtype=torch.int32, device=dev)  # noqa: E731
    outs = [i32(n_k), i32(n_k), i32(n_i), i32(n_i), i32(n_i),
            torch.full((max(B * n_i, 1),), -7, dtype=torch.int64, device=dev), i32(n_cells)]
    head = [ctx.handle, stream, S, d, d_d.data_ptr(), off, 1, sem.data_ptr(), 1, ins.data_ptr(), 2, ps_sem.data_ptr(), 2,
            ps_ins.data_ptr(), prob.data_ptr()]
    tail = [1, ws.data_ptr(), ws_bytes] + [t.data_ptr() for t in outs] + [status.data_ptr()]
    if entry == "rows":
        rc = lib.gapro_eval_ap_tables_rows(*head, T, (C.c_float * max(T, 1))(*taus), *tail)
    else:
        rc = lib.gapro_eval_ap_tables(*head, *tail)
    err = (lib.gapro_last_error(ctx.handle) or b"").decode() if rc else ""
    torch.cuda.synchronize()
    return rc, err, [t.cpu().numpy() for t in [status] + outs]


def test_row_0_and_the_zero_threshold_call_are_the_plain_tables_bit_for_bit():
    from gapro_amd.eval_ap_ps_labels import ap_tables, ap_tables_rows

    scenes = fixture_scenes("synth") + [random_scene(21, 3000, 40, 30), random_scene(22, 257, 5, 600)]
    taus = sorted(own_thresholds(scenes))
    rc0, _, plain = _raw_call(scenes, [], "tables")
    rc1, _, zero = _raw_call(scenes, [], "rows")
    rc2, _, rows = _raw_call(scenes, taus, "rows")
    assert rc0 == rc1 == rc2 == 0
    for a, b, c in zip(plain, zero, rows):
        assert a.dtype == b.dtype == c.dtype and np.array_equal(a, b)
        assert np.array_equal(a, c[:len(a)])  # row 0's block is laid out as the plain output
    assert not plain[0].any()
    # the same through the Python layer, for both confidences
    for conf in ("one", "mean_prob"):
        ref = ap_tables(scenes, conf)
        for other in (ap_tables_rows(scenes, (), conf), ap_tables_rows(scenes, taus, conf)):
            for got, want, sc in zip(other.tables[0], ref, scenes):
                assert_tables_equal(got, want)
                assert_tables_equal(got, tally(*sc, confidence=conf))


def test_a_scene_alone_equals_the_scene_in_a_batch_of_three():
    from gapro_amd.eval_ap_ps_labels import ap_tables_rows

    a, b, c = random_scene(31, 700, 12, 9), random_scene(32, 2500, 30, 40), random_scene(33, 300, 3, 700)
    taus = [0.7, 0.2, 0.5]
    batch = ap_tables_rows([a, b, c], taus, "mean_prob")
    for i, sc in enumerate((a, b, c)):
        alone = ap_tables_rows([sc], taus, "mean_prob")
        assert np.array_equal(alone.kept[0], batch.kept[i])
        for r in range(4):
            assert_tables_equal(alone.tables[r][0], batch.tables[r][i])
    _check_rows([c, a, b], taus)


# ------------------------------------------------------------------------------------------------ 3. threshold edges
def test_threshold_edges():
    from gapro_amd.eval_ap_ps_labels import evaluate_ap_rows

    below = float(np.nextafter(F32(0.5), F32(0)))
    sc = random_scene(41, 600, 8, 9, prob_levels=(0.25, below, 0.5, 1.0))
    assert all((sc[4] == F32(v)).sum() > 50 for v in (below, 0.5, 1.0))
    taus = [0.5, 0.0, 1.5, 1.0, 0.5, below]
    rows = _check_rows([sc], taus)
    n = {v: int((sc[4] == F32(v)).sum()) for v in (0.25, below, 0.5, 1.0)}
    # a probability equal to tau is kept, the float32 just below it is dropped
    assert rows.kept[0].tolist() == [600, n[0.5] + n[1.0], 600, 0, n[1.0], n[0.5] + n[1.0], 600 - n[0.25]]
    for f, x in zip(rows.tables[2][0], rows.tables[0][0]):  # tau = 0 is row 0 again
        assert np.array_equal(f, x)
    for f, x in zip(rows.tables[1][0], rows.tables[5][0]):  # equal thresholds, equal rows
        assert np.array_equal(f, x)
    assert all(len(v) == 0 for v in rows.tables[3][0])      # above every probability: zero-length tables
    assert len(rows.tables[4][0].pred_id) > 0               # tau = 1.0 keeps the probabilities that are 1.0f
    res = evaluate_ap_rows([sc], taus, "mean_prob", min_region_size=10)
    assert np.isnan(res.results[3].ap).all() and np.isnan(res.results[3].avgs["all_ap"])  # no GT instance: NaN
    assert res.results[3].n_gt.sum() == 0 and res.results[0].n_gt.sum() > 0
    assert res.kept.tolist() == rows.kept[0].tolist() and res.coverage[3] == 0.0 and res.coverage[2] == 1.0
    assert res.coverage[1] == (n[0.5] + n[1.0]) / 600


def test_32_thresholds_are_accepted_and_bad_ones_refused():
    from gapro_amd.eval_ap_ps_labels import ap_tables_rows

    sc = random_scene(42, 400, 5, 6)
    _check_rows([sc], [(k + 1) / 34.0 for k in range(32)][::-1], "one")
    with pytest.raises(ValueError, match="at most 32"):
        ap_tables_rows([sc], [(k + 1) / 35.0 for k in range(33)])
    with pytest.raises(ValueError, match="NaN"):
        ap_tables_rows([sc], [0.5, float("nan")])
    # the library itself: 33 thresholds, a descending pair, a NaN, and a workspace without the rows' first points
    rc, err, _ = _raw_call([sc], [0.5, 0.25], "rows")
    assert rc == BAD_ARG and "ascending" in err
    rc, err, _ = _raw_call([sc], [0.5, float("nan")], "rows")
    assert rc == BAD_ARG and "ascending" in err
    import torch
    from gapro_amd import _lib

    ctx = _lib.Context.get(0)
    d = (_lib.EvalApScene * 1)()
    d[0].n_points, d[0].max_ps = 4, 2
    assert ctx.lib.gapro_eval_ap_workspace_bytes_rows(d, 1, 33) == 0
    small = int(ctx.lib.gapro_eval_ap_workspace_bytes(d, 1))
    assert ctx.lib.gapro_eval_ap_pair_cells(d, 1) == 3
    t = torch.zeros(64, dtype=torch.int64, device="cuda:0")
    ws = torch.zeros(small + 64, dtype=torch.uint8, device="cuda:0")
    thr = (C.c_float * 33)(*[k / 40.0 for k in range(33)])
    p = t.data_ptr()
    call = lambda T, prob, ws_bytes: ctx.lib.gapro_eval_ap_tables_rows(  # noqa: E731
        ctx.handle, None, 1, d, p, 4, 3, p, 3, p, 3, p, 3, p, prob, T, thr, 1, ws.data_ptr(), ws_bytes, p, p, p, p, p, p, p,
        p)
    assert call(33, p, small + 64) == BAD_ARG
    assert call(-1, p, small + 64) == BAD_ARG
    assert call(1, None, small + 64) == BAD_ARG   # thresholds need d_prob
    assert call(2, p, small + 8) == WORKSPACE     # two rows of two ids need 32 bytes behind the scene's block
    torch.cuda.synchronize()
    _check_rows([sc], [0.5])                      # the context is as usable as before


# ------------------------------------------------------------------------------------------------ 4. first-point rule
def _first_point_scene():
    # (points, raw GT class, GT inst, pseudo class, pseudo id, prob); GT class c is raw c + 1, pseudo class c is c - 1
    seg = [(1, 4, 0, 2, 0, 0.1),     # id 0's first point: class 3, on GT 3001
           (20, 4, 0, 4, 0, 0.9),    # id 0 on GT 3001 with class 5 points
           (40, 6, 1, 4, 0, 0.9),    # id 0 on GT 5002
           (1, 6, 1, 4, 1, 0.1),     # id 1's first point: class 5
           (30, 6, 1, 18, 1, 0.5),   # id 1's first point from 0.3 on: 19, not a class
           (30, 6, 1, 4, 1, 0.9),    # id 1's first point from 0.7 on: class 5 again
           (25, 3, 2, 1, 2, 0.1),    # GT 2003 and id 2: gone from 0.3 on; the lowest code, so the GT indices move
           (10, 0, -100, -100, -100, 0.9)]
    cols = [np.concatenate([np.full(s[0], s[k]) for s in seg]) for k in range(1, 6)]
    return [cols[0].astype(np.float64), cols[1].astype(np.float64), cols[2].astype(np.int32), cols[3].astype(np.int32),
            cols[4].astype(F32)]


def test_a_rows_label_is_that_of_the_first_kept_point():
    sc = _first_point_scene()
    rows = _check_rows([sc], [0.3, 0.7])
    r0, r1, r2 = (rows.tables[r][0] for r in range(3))
    assert r0.gt_code.tolist() == [2003, 3001, 5002] and r0.pred_id.tolist() == [0, 1, 2]
    assert r0.pred_label.tolist() == [3, 5, 2]
    assert (r0.pair_gt.tolist(), r0.pair_pred.tolist(), r0.pair_inter.tolist()) == ([0, 1, 2], [2, 0, 1], [25, 21, 61])
    # 0.3: id 0 is class 5 now and pairs with GT 5002, not 3001; id 1 has no class; GT 2003 and id 2 have no point
    assert r1.gt_code.tolist() == [3001, 5002] and r1.gt_n.tolist() == [20, 100]
    assert r1.pred_id.tolist() == [0] and r1.pred_label.tolist() == [5] and r1.pred_n.tolist() == [60]
    assert (r1.pair_gt.tolist(), r1.pair_pred.tolist(), r1.pair_inter.tolist()) == ([1], [0], [40])
    # 0.7: id 1 is back, with the class of its first point there
    assert r2.gt_code.tolist() == [3001, 5002] and r2.gt_n.tolist() == [20, 70]
    assert r2.pred_id.tolist() == [0, 1] and r2.pred_label.tolist() == [5, 5] and r2.pred_n.tolist() == [60, 30]
    assert (r2.pair_gt.tolist(), r2.pair_pred.tolist(), r2.pair_inter.tolist()) == ([1, 1], [0, 1], [40, 30])
    assert r2.pred_conf.tolist() == [float(F32(0.9))] * 2
    # min_region_size applies to the kept counts: GT 3001 (21 -> 20 points) counts at 21 in row 0 only
    from gapro_amd.eval_ap_ps_labels import ap_from_tables

    assert [int(ap_from_tables([t], 21).n_gt[2]) for t in (r0, r1, r2)] == [1, 0, 0]


# ------------------------------------------------------------------------------------------------ 5. kernel edges
def test_point_counts_around_a_workgroup():
    scenes = [random_scene(50 + i, n, 3, 4) for i, n in enumerate((0, 1, 255, 256, 257))]
    rows = _check_rows(scenes, [0.6, 0.3])
    assert rows.kept[:, 0].tolist() == [0, 1, 255, 256, 257]
    assert all(len(v) == 0 for r in range(3) for v in rows.tables[r][0])
    _check_rows(scenes[:1], [0.5])  # a batch of nothing but an empty scene


def test_tables_on_both_sides_of_the_lds_switches_with_several_workgroups():
    """5000 points: three workgroups of 8 points per thread tally a scene, so the LDS partials merge.  15 keys x 15 ids
    are 256 pair cells: 32 bins fill the 8192 LDS cells, 33 go to global memory.  16 ids: 32 bins fill the 512 LDS
    first-point / sum entries, 33 do not (3 keys keep that scene's pairs in LDS either way)."""
    pairs, ids = random_scene(61, 5000, 15, 15), random_scene(62, 5000, 3, 16)
    assert len(tally(*pairs).gt_code) == 15 and pairs[3].max() == 14 and ids[3].max() == 15
    t32 = [(k + 1) / 33.0 for k in range(32)]
    in_lds = _check_rows([pairs, ids], t32[:31])
    in_global = _check_rows([pairs, ids], t32)
    for r in range(32):
        for a, b in zip(in_lds.tables[r], in_global.tables[r]):
            assert_tables_equal(a, b)
    assert np.array_equal(in_lds.kept, in_global.kept[:, :32])
    # max_ps beyond the ids in use: the table size, not the largest id, places the tables
    _check_rows([ids], t32[:31], max_ps=[17])


# ------------------------------------------------------------------------------------------------ 6. bad probabilities
@pytest.mark.parametrize("value", [np.nan, 1.5, -0.25])
def test_a_bad_probability_names_its_scene(value):
    from gapro_amd.eval_ap_ps_labels import ap_tables_rows

    good = random_scene(71, 300, 4, 5)
    bad = [a.copy() for a in good]
    bad[4][17] = value
    with pytest.raises(ValueError, match=r"scene\(s\) \[1\]"):
        ap_tables_rows([good, bad, good], [0.5], "one")
    _check_rows([good], [0.5], "one")


# ------------------------------------------------------------------------------------------------ 7. CLI
def _write_layout(tmp_path, names):
    import torch
    from gapro_amd.gen_ps import write_label_file  # pth_io's writer

    root, ps = tmp_path / "scannetv2", tmp_path / "labels"
    (root / "train").mkdir(parents=True)
    ps.mkdir()
    scenes = []
    for i, g in enumerate(names):
        z = np.load(os.path.join(ROOT, "tests", "golden", g + ".npz"))
        scan = "scene%04d_00" % i
        torch.save((z["xyz_raw"], z["rgb"], z["sem_gt"], z["inst_gt"]), str(root / "train" / (scan + "_inst_nostuff.pth")))
        write_label_file(str(ps / (scan + ".pth")), (z["out_sem"], z["out_inst"], z["out_prob"], z["out_mu"], z["out_var"]))
        scenes.append([z["sem_gt"], z["inst_gt"], z["out_sem"], z["out_inst"], z["out_prob"]])
    return str(root), str(ps), scenes


def _run_cli(args):
    return subprocess.run([sys.executable, "-m", "gapro_amd.eval_ap_ps_labels"] + args, cwd=ROOT, capture_output=True,
                          text=True, timeout=300)


def test_cli_prints_and_writes_the_threshold_rows(tmp_path):
    from gapro_amd.eval_ap_ps_labels import evaluate_ap_rows
    from gapro_amd.eval_ps_labels import _nan_to_none

    root, ps, scenes = _write_layout(tmp_path, ("s0_walls", "s2_dense", "s5_lean"))
    out = str(tmp_path / "ap.json")
    taus = [0.8, 0.6]
    want = evaluate_ap_rows(scenes, taus, "mean_prob")
    p = _run_cli(["--ps_folder", ps, "--data_root", root, "--json", out, "--batch_scenes", "2", "--confidence",
                  "mean_prob", "--prob_thresholds", "0.8,0.6"])
    assert p.returncode == 0, p.stdout + p.stderr
    got = json.load(open(out))
    lines = p.stdout.split("\n")
    a0 = want.results[0].avgs
    k = lines.index("AP: {:.3f}. AP_50: {:.3f}. AP_25: {:.3f}".format(a0["all_ap"], a0["all_ap_50%"], a0["all_ap_25%"]))
    assert lines[k + 1] == "%-10s %10s %8s %8s %8s" % ("prob >=", "coverage", "AP", "AP_50", "AP_25")
    assert len(got["thresholds"]) == 2
    for j, tau in enumerate(taus):
        a = want.results[j + 1].avgs
        assert lines[k + 2 + j] == "%-10g %10.4f %8.3f %8.3f %8.3f" % (tau, want.coverage[j + 1], a["all_ap"],
                                                                       a["all_ap_50%"], a["all_ap_25%"])
        e = got["thresholds"][j]
        assert e["threshold"] == tau and e["kept_points"] == int(want.kept[j + 1])
        assert e["coverage"] == float(want.coverage[j + 1])
        for key in ("all_ap", "all_ap_50%", "all_ap_25%", "all_rc", "all_rc_50%", "all_rc_25%"):
            assert e["avgs"][key] == _nan_to_none(a[key]), key
        assert list(e["n_gt"].values()) == want.results[j + 1].n_gt.tolist()
        assert list(e["n_pred"].values()) == want.results[j + 1].n_pred.tolist()
    assert got["avgs"]["all_ap"] == _nan_to_none(a0["all_ap"]) and 0 < want.coverage[1] < want.coverage[2] < 1

    # without the flag: today's output, no new key, no extra line
    q = _run_cli(["--ps_folder", ps, "--data_root", root, "--json", out, "--confidence", "mean_prob"])
    assert q.returncode == 0, q.stdout + q.stderr
    plain = json.load(open(out))
    assert "thresholds" not in plain and sorted(plain) == sorted(set(got) - {"thresholds"})
    assert plain["avgs"] == got["avgs"] and plain["n_gt"] == got["n_gt"]
    assert q.stdout.split("\n") == lines[:k + 1] + lines[k + 4:] and "prob >=" not in q.stdout
