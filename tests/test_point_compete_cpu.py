"""Host side of point_level="compete" (no GPU needed): gapro_schedule_export_testers against a CSR built from the exported
events, the fact that a refined superpoint is listed by no containment event, the host plan of the expanded predict
launch on the golden scenes, and the ABI of the two new device entry points."""
import ctypes as C

import numpy as np
import pytest

from gapro_amd import _lib
from gapro_amd.pipeline import BLOCK_DTYPE, SEGMENT_DTYPE, Pipeline, plan_point_compete, point_mode
from oracle import gen_ps_oracle as O

# golden -> refined superpoints, their points R, (superpoints, points) tested by >= 2 fits, max testers, rows R2:
# counted on the CPU from oracle.gen_ps_oracle.enumerate_schedule and the recorded reference fit outputs
TABLE = {
    "s0_walls": (13, 316, 0, 0, 1, 316),
    "s1_nowalls": (4, 78, 0, 0, 1, 78),
    "s2_dense": (44, 712, 3, 39, 3, 790),
    "s3_bigspp": (0, 0, 0, 0, 0, 0),
    "s4_dups": (7, 99, 0, 0, 1, 99),
    "s5_lean": (92, 1769, 28, 525, 6, 3302),
}


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p(0)


def _occ_bits(occ_spp):
    S, B = occ_spp.shape
    bits = np.zeros((S, (B + 63) // 64), dtype=np.uint64)
    for b in range(B):
        bits[:, b // 64] |= occ_spp[:, b].astype(np.uint64) << np.uint64(b % 64)
    return bits


def _events(lib, sched):
    cnt = _lib.ScheduleCounts()
    assert lib.gapro_schedule_get_counts(sched, C.byref(cnt)) == 0
    n = max(cnt.n_events, 1)
    kind, b1, b2, aux = np.zeros(n, np.uint8), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    offs = np.zeros(cnt.n_events + 1, np.int64)
    eidx = np.zeros(max(cnt.n_event_idx, 1), np.int32)
    assert lib.gapro_schedule_export_events(sched, _p(kind), _p(b1), _p(b2), _p(aux), _p(offs), _p(eidx)) == 0
    return cnt, [(int(kind[i]), int(b1[i]), int(b2[i]), int(aux[i]), eidx[offs[i]:offs[i + 1]].copy())
                 for i in range(cnt.n_events)]


def _testers(lib, sched, S, cnt):
    """gapro_schedule_export_testers into canary-framed arrays: (offsets, fit, pos)."""
    n = int(cnt.n_fit_out)
    off = np.full(S + 2, -7, np.int64)
    fit, pos = np.full(n + 1, -7, np.int32), np.full(n + 1, -7, np.int32)
    assert lib.gapro_schedule_export_testers(sched, _p(off), _p(fit), _p(pos)) == 0
    assert off[S + 1] == -7 and fit[n] == -7 and pos[n] == -7  # nothing beyond S + 1 offsets and n entries
    assert off[0] == 0 and off[S] == n and (np.diff(off[:S + 1]) >= 0).all()
    return off[:S + 1].copy(), fit[:n].copy(), pos[:n].copy()


def _testers_from_events(events, S):
    """The CSR the issue defines, from the exported events alone: per superpoint the (fit, position) pairs of the fit
    events that list it, in event order."""
    per = [[] for _ in range(S)]
    for kind, _, _, aux, inter in events:
        if kind == 1:
            for j, sp in enumerate(inter):
                per[sp].append((aux, j))
    return per


def _check_testers(off, fit, pos, per):
    assert len(off) == len(per) + 1
    for sp, want in enumerate(per):
        got = list(zip(fit[off[sp]:off[sp + 1]].tolist(), pos[off[sp]:off[sp + 1]].tolist()))
        assert got == want, (sp, got, want)


def _contained(events, S):
    m = np.zeros(S, dtype=bool)
    for kind, _, _, _, inter in events:
        if kind == 0:
            m[inter] = True
    return m


def _merge_winner(lib, sched, S, fit_out, cls64, vol64, n_fg):
    tabs = [np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros(S, np.float32), np.zeros(S, np.float32),
            np.zeros(S, np.float32)]
    winner = np.full(S, 77, np.int32)
    pn, lb, mu, var = fit_out
    assert lib.gapro_schedule_merge_ex(sched, _p(pn), _p(lb), _p(mu), _p(var), _p(cls64), _p(vol64), n_fg, 18,
                                       *[_p(t) for t in tabs], _p(winner)) == 0
    return winner


_CACHE = {}


def _golden_scene(name):
    """Schedule of a golden scene, once per session: events, testers, the winners the recorded reference fit outputs
    give, and the superpoints' point counts."""
    if name in _CACHE:
        return _CACHE[name]
    from conftest import Golden

    golden = Golden(name)
    lib = _lib.load()
    kw = golden.api_inputs()
    boxes, cls, vol = O.assemble_boxes(kw["coords_float"], kw["instance_cls"], kw["instance_box"],
                                       kw["instance_box_volume"], kw["wall_box"], kw["wall_box_volume"])
    part = O.partition(kw["coords_float"], kw["mask_feats"], kw["spp"], boxes, cls, vol, 0.999)
    bits = np.ascontiguousarray(_occ_bits(part.occ_spp))
    n_bbs = np.ascontiguousarray(part.n_bbs_per_spp.astype(np.int32))
    boxes = np.ascontiguousarray(boxes)
    S = part.n_spps
    sched = C.c_void_p()
    assert lib.gapro_schedule_build(S, len(boxes), _p(boxes), _p(bits), _p(n_bbs), C.byref(sched)) == 0
    try:
        cnt, events = _events(lib, sched)
        fits = golden.fits
        assert cnt.n_fits == len(fits)
        if fits:
            fit_out = tuple(np.ascontiguousarray(np.concatenate([f[k] for f in fits]).astype(dt))
                            for k, dt in (("probs_new", np.float32), ("labels", np.uint8), ("mu", np.float32),
                                          ("var", np.float32)))
        else:
            fit_out = (None, None, None, None)
        winner = _merge_winner(lib, sched, S, fit_out, np.ascontiguousarray(cls.astype(np.int64)),
                               np.ascontiguousarray(vol.astype(np.float64)), len(kw["instance_box"]))
        testers = _testers(lib, sched, S, cnt)
        descs = (_lib.FitDesc * max(cnt.n_fits, 1))()
        h_idx = np.zeros(max(int(cnt.n_fit_idx), 1), np.int32)
        assert lib.gapro_schedule_export_fits(sched, 0, 0, 0, 0, C.cast(descs, C.c_void_p), _p(h_idx)) == 0
    finally:
        lib.gapro_schedule_free(sched)
    r = dict(S=S, events=events, n_fits=int(cnt.n_fits), winner=winner, testers=testers, n_bbs=n_bbs,
             point_count=part.point_count.astype(np.int32), descs=descs, oracle_events=O.enumerate_schedule(
                 boxes, part.occ_spp, part.n_bbs_per_spp))
    _CACHE[name] = r
    return r


def _check_plan(plan, scenes):
    """What every plan must satisfy, whatever the scenes: blocks ascending, disjoint and covering [0, R), one per refined
    superpoint with its point count, in (scene, superpoint) order; every block's segments are its testers in order; the
    segments of a model are contiguous in the row list, ascending in superpoint, and tile [0, R2)."""
    blocks, segs, models = plan["blocks"], plan["segments"], plan["models"]
    assert blocks.dtype == BLOCK_DTYPE and segs.dtype == SEGMENT_DTYPE
    R, R2 = plan["rows"], plan["expanded_rows"]
    end, base, nb, seg_end = 0, 0, 0, 0
    pieces = []  # (out_start, rows, model) of every segment
    for si, sc in enumerate(scenes):
        off, fit, _ = sc["testers"]
        ref = np.nonzero(sc["winner"] >= 0)[0]
        assert plan["scene_rows"][si] == (end, int(sc["point_count"][ref].sum()))
        for sp in range(sc["S"]):
            row = plan["sp_row"][base + sp]
            if sc["winner"][sp] < 0:
                assert row == -1
                continue
            b = blocks[nb]
            nb += 1
            assert (b["row_start"], b["n_rows"], b["scene"]) == (end, sc["point_count"][sp], si) and row == end
            end += int(b["n_rows"])
            assert b["seg_start"] == seg_end and b["n_seg"] == off[sp + 1] - off[sp] >= 1
            seg_end += int(b["n_seg"])
            for s, k in zip(segs[b["seg_start"]:b["seg_start"] + b["n_seg"]], fit[off[sp]:off[sp + 1]]):
                f, msi = models[s["model"]][:2]
                assert msi == si and f == sc["fit_base"] + k and s["reserved"] == 0
                pieces.append((int(s["out_start"]), int(b["n_rows"]), int(s["model"])))
            assert sc["winner"][sp] in fit[off[sp]:off[sp + 1]]
        base += sc["S"]
    assert nb == len(blocks) and end == R and seg_end == len(segs) and base == len(plan["sp_row"])
    pieces.sort()
    at, seen = 0, []
    for o, n, m in pieces:  # the row list is tiled without gap or overlap, one run per model, models ascending
        assert o == at
        at += n
        if not seen or seen[-1] != m:
            seen.append(m)
    assert at == R2 and seen == list(range(len(models)))
    for m, (f, si, row0, t, b1, b2) in enumerate(models):
        mine = [(o, n) for o, n, k in pieces if k == m]
        assert mine and mine[0][0] == row0 and sum(n for _, n in mine) == t
        d = scenes[si]["descs"][f - scenes[si]["fit_base"]]
        assert (b1, b2) == (d.b1, d.b2)
    assert [m[:2] for m in models] == sorted(m[:2] for m in models)


def _plan(scenes):
    fb = 0
    for sc in scenes:
        sc["fit_base"] = fb
        fb += sc["n_fits"]
    descs = (_lib.FitDesc * max(fb, 1))()
    for sc in scenes:
        for k in range(sc["n_fits"]):
            descs[sc["fit_base"] + k] = sc["descs"][k]
    return plan_point_compete([sc["winner"] for sc in scenes], [sc["point_count"] for sc in scenes],
                              [sc["testers"] for sc in scenes], [sc["fit_base"] for sc in scenes], descs)


def test_testers_and_plan_on_the_golden_scenes(golden):
    sc = _golden_scene(golden.name)
    S, (off, fit, pos) = sc["S"], sc["testers"]
    per = _testers_from_events(sc["events"], S)
    _check_testers(off, fit, pos, per)
    # the same lists from the oracle's own enumeration: fits numbered in the order of its fit events
    k, per_o = 0, [[] for _ in range(S)]
    for e in sc["oracle_events"]:
        if e.kind == "fit":
            for j, sp in enumerate(e.intersect_inds):
                per_o[int(sp)].append((k, j))
            k += 1
    assert per_o == per and k == sc["n_fits"]
    # rule 1: a refined superpoint is listed by no containment event, lies in several boxes, and its winner tested it
    refined = sc["winner"] >= 0
    assert not (refined & _contained(sc["events"], S)).any()
    assert (sc["n_bbs"][refined] > 1).all()
    plan = _plan([sc])
    _check_plan(plan, [sc])
    n_test = np.diff(off)[refined]
    pts = sc["point_count"][refined]
    multi = n_test >= 2
    got = (int(refined.sum()), plan["rows"], int(multi.sum()), int(pts[multi].sum()), int(n_test.max(initial=0)),
           plan["expanded_rows"])
    assert got == TABLE[golden.name], (golden.name, got)
    assert plan["refined_spps"] == got[0] and plan["multi_spps"] == got[2]
    assert plan["expanded_rows"] == int((pts.astype(np.int64) * n_test).sum())
    assert len(plan["models"]) == len(np.unique(np.concatenate([fit[off[sp]:off[sp + 1]]
                                                                for sp in np.nonzero(refined)[0]] + [fit[:0]])))


def test_plan_of_a_batch_and_of_scenes_that_take_no_part():
    """All six goldens as one batch, the fit-less scene first: scene offsets of superpoints, rows, fits and models.  A
    scene whose winners are None (it failed before the plan) contributes nothing and moves nobody else's rows."""
    from conftest import GOLDEN_NAMES

    names = ["s3_bigspp"] + [n for n in GOLDEN_NAMES if n != "s3_bigspp"]
    scenes = [dict(_golden_scene(n)) for n in names]
    plan = _plan(scenes)
    _check_plan(plan, scenes)
    assert plan["rows"] == sum(TABLE[n][1] for n in names) and plan["expanded_rows"] == sum(TABLE[n][5] for n in names)
    assert plan["refined_spps"] == sum(TABLE[n][0] for n in names) and plan["multi_spps"] == 31
    out = [dict(sc) for sc in scenes]
    lost = names.index("s2_dense")
    winners = [None if i == lost else sc["winner"] for i, sc in enumerate(out)]
    p2 = plan_point_compete(winners, [sc["point_count"] for sc in out], [sc["testers"] for sc in out],
                            [sc["fit_base"] for sc in out])
    out[lost]["winner"] = np.full(out[lost]["S"], -1, np.int32)
    p3 = _plan(out)
    _check_plan(p3, out)
    for k in ("sp_row", "blocks", "segments"):
        assert np.array_equal(p2[k], p3[k]), k
    assert p2["rows"] == plan["rows"] - TABLE["s2_dense"][1] and [m[:4] for m in p2["models"]] == [m[:4] for m in p3["models"]]
    assert all(m[4:] == (-1, -1) for m in p2["models"])  # without descriptors the models carry no boxes
    empty = plan_point_compete([], [], [], [])
    assert (empty["rows"], empty["expanded_rows"], len(empty["blocks"]), len(empty["sp_row"])) == (0, 0, 0, 0)


def test_testers_on_a_hand_built_schedule():
    """The four-box schedule of tests/test_point_refine_cpu.py: fit 0 (boxes 0, 1) on superpoints [6 7 8 9 10], fit 1
    (0, 2) on [6 12], fit 2 (0, 3) on [8 9 10], and the containment verdict (1, 2) -> 2 on [6 13]."""
    lib = _lib.load()
    boxes = np.array([[0.0, 0.0, 0.0, 2.0, 2.0, 2.0],
                      [1.5, 0.0, 0.0, 4.0, 2.0, 2.0],
                      [1.6, 0.5, 0.5, 3.0, 1.5, 1.5],
                      [-1.5, 0.0, 0.0, 0.5, 2.0, 2.0]])
    member = [{0}, {0}, {1}, {2}, {3}, {1}, {0, 1, 2}, {0, 1}, {0, 1, 3}, {0, 1, 3}, {0, 1, 3}, set(), {0, 2}, {1, 2}]
    S, B = len(member), len(boxes)
    occ = np.zeros((S, B), dtype=bool)
    for sp, bs in enumerate(member):
        occ[sp, list(bs)] = True
    bits = np.ascontiguousarray(_occ_bits(occ))
    n_bbs = np.ascontiguousarray(occ.sum(1).astype(np.int32))
    sched = C.c_void_p()
    assert lib.gapro_schedule_build(S, B, _p(boxes), _p(bits), _p(n_bbs), C.byref(sched)) == 0
    try:
        cnt, events = _events(lib, sched)
        assert [list(e[4]) for e in events] == [[6, 7, 8, 9, 10], [6, 12], [8, 9, 10], [6, 13]]
        off, fit, pos = _testers(lib, sched, S, cnt)
        _check_testers(off, fit, pos, _testers_from_events(events, S))
        lists = [list(zip(fit[off[sp]:off[sp + 1]].tolist(), pos[off[sp]:off[sp + 1]].tolist())) for sp in range(S)]
        assert lists[8] == [(0, 2), (2, 0)] and lists[9] == [(0, 3), (2, 1)] and lists[10] == [(0, 4), (2, 2)]
        assert lists[6] == [(0, 0), (1, 0)] and lists[7] == [(0, 1)] and lists[12] == [(1, 1)]
        assert [sp for sp in range(S) if not lists[sp]] == [0, 1, 2, 3, 4, 5, 11, 13]  # 13: a containment is no tester
        # the winners of the outputs that test chose: superpoint 6 is reset by the containment event, so no refined
        # superpoint is listed by one
        pn = np.array([0.9, 0.8, 0.6, 0.7, 0.75, 0.95, 0.85, 0.65, 0.7, 0.5], dtype=np.float32)
        lb = np.array([0, 1, 0, 1, 0, 1, 0, 1, 0, 1], dtype=np.uint8)
        mu, var = np.arange(10, dtype=np.float32) - 4.5, np.arange(10, dtype=np.float32) + 1.0
        winner = _merge_winner(lib, sched, S, (pn, lb, mu, var), np.array([3, 5, 7, 18], dtype=np.int64),
                               np.array([8.0, 10.0, 1.4, 8.0]), 3)
        np.testing.assert_array_equal(winner, [-1, -1, -1, -1, -1, -1, -1, 0, 2, 0, 0, -1, 1, -1])
        assert not ((winner >= 0) & _contained(events, S)).any() and _contained(events, S)[6]
        # its plan: blocks 7, 8, 9, 10, 12 with 3, 1, 4, 2, 5 points; fit 0 tests four of them, fit 1 one, fit 2 three
        pc = np.zeros(S, np.int32)
        pc[[7, 8, 9, 10, 12]] = [3, 1, 4, 2, 5]
        pc[pc == 0] = 9
        descs = (_lib.FitDesc * 3)()
        for d, (b1, b2) in zip(descs, [(0, 1), (0, 2), (0, 3)]):
            d.b1, d.b2 = b1, b2
        sc = dict(S=S, winner=winner, point_count=pc, testers=(off, fit, pos), fit_base=0, descs=descs)
        plan = plan_point_compete([winner], [pc], [(off, fit, pos)], [0], descs)
        _check_plan(plan, [sc])
        assert plan["blocks"]["row_start"].tolist() == [0, 3, 4, 8, 10] and plan["rows"] == 15
        assert plan["blocks"]["n_seg"].tolist() == [1, 2, 2, 2, 1] and plan["multi_spps"] == 3
        assert plan["models"] == [(0, 0, 0, 10, 0, 1), (1, 0, 10, 5, 0, 2), (2, 0, 15, 7, 0, 3)]
        assert plan["expanded_rows"] == 22
        # segments in block order: 7:[fit 0]  8:[fit 0, fit 2]  9:[fit 0, fit 2]  10:[fit 0, fit 2]  12:[fit 1]
        assert plan["segments"]["model"].tolist() == [0, 0, 2, 0, 2, 0, 2, 1]
        assert plan["segments"]["out_start"].tolist() == [0, 3, 15, 4, 16, 8, 20, 10]
    finally:
        lib.gapro_schedule_free(sched)


def test_point_compete_abi():
    # sizes and offsets follow the C declarations: i64 | 4 x i32;  i64 | 2 x i32 -- and the NumPy images the plan fills
    B, G = _lib.PointRefineBlock, _lib.PointRefineSegment
    assert C.sizeof(B) == 24 and C.sizeof(G) == 16
    assert [getattr(B, f).offset for f in ("row_start", "n_rows", "scene", "seg_start", "n_seg")] == [0, 8, 12, 16, 20]
    assert [getattr(G, f).offset for f in ("out_start", "model", "reserved")] == [0, 8, 12]
    for dt, st in ((BLOCK_DTYPE, B), (SEGMENT_DTYPE, G)):
        assert dt.itemsize == C.sizeof(st)
        assert [(n, dt.fields[n][1]) for n in dt.names] == [(n, getattr(st, n).offset) for n, _ in st._fields_]
    lib = _lib.load()
    for name in ("gapro_schedule_export_testers", "gapro_point_refine_expand", "gapro_point_refine_compete"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.gapro_version() == 200
    # without a device there is no context: every call is refused before it looks at anything else
    blocks, segs = (B * 1)(), (G * 1)()
    scenes, models = (_lib.PointRefineScene * 1)(), (_lib.PointRefineModel * 1)()
    bp, gp, sp, mp = (C.cast(x, C.c_void_p) for x in (blocks, segs, scenes, models))
    assert lib.gapro_point_refine_expand(None, None, 1, bp, bp, 1, gp, gp, 10, 10, bp) == -1
    assert lib.gapro_point_refine_expand(None, None, 0, None, None, 0, None, None, 0, 0, None) == -1
    assert lib.gapro_point_refine_expand(None, None, 1, bp, bp, 1, gp, gp, 10, 2 ** 31, bp) == -1
    assert lib.gapro_point_refine_expand(None, None, -1, bp, bp, -1, gp, gp, -1, -1, bp) == -1
    args = (1, sp, sp, 1, mp, mp, 1, bp, bp, 1, gp, gp)
    assert lib.gapro_point_refine_compete(None, None, *args, 10, 10, sp, sp, sp, sp, sp, None, None) == -1
    assert lib.gapro_point_refine_compete(None, None, *args, 10, 2 ** 31, sp, sp, sp, sp, sp, None, None) == -1
    assert lib.gapro_point_refine_compete(None, None, 0, None, None, 0, None, None, 0, None, None, 0, None, None, 0, 0,
                                          None, None, None, None, None, None, None) == -1
    z = np.zeros(4, np.int64)
    assert lib.gapro_schedule_export_testers(None, _p(z), _p(z), _p(z)) == -1


def test_point_level_values():
    assert [point_mode(v) for v in (False, True, "winner", "compete", np.bool_(True))] == [None, "winner", "winner",
                                                                                           "compete", "winner"]
    for bad in ("nonsense", "Compete", 1, 0, None, 2.0, ["compete"]):
        with pytest.raises(ValueError):
            point_mode(bad)
    # refused before a context is made: this needs no device
    with pytest.raises(ValueError):
        Pipeline(point_level="nonsense")
    with pytest.raises(ValueError):
        Pipeline(point_level="nonsense", backend="native")
