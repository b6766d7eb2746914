"""Host side of the point-level labels (no GPU needed): gapro_schedule_merge_ex's winner table against a NumPy replay of
the exported events, on the golden scenes and on a hand-built schedule, and the ABI of the point-refine entry points."""
import ctypes as C

import numpy as np

from gapro_amd import _lib
from oracle import gen_ps_oracle as O


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


def _replay_winner(events, n_bbs, probs_new):
    """The rule of the issue, from the exported events alone: winner starts at -1; a fit event that overwrites a
    superpoint (strict float32 <) sets it to the fit's index; a containment event that writes it sets it back to -1.
    Returns the winners and, per superpoint, the list of what happened to it ('fit k' taken / 'tested k' / 'contain')."""
    S = len(n_bbs)
    prob = np.where(n_bbs <= 1, np.float32(1), np.float32(0)).astype(np.float32)  # single-box / no-box superpoints
    winner = np.full(S, -1, dtype=np.int32)
    hist = [[] for _ in range(S)]
    o = 0
    for kind, _, _, aux, inter in events:
        if kind == 0:
            for sp in inter:
                winner[sp], prob[sp] = -1, np.float32(1)
                hist[sp].append("contain")
            continue
        pn = probs_new[o:o + len(inter)]
        o += len(inter)
        for sp, v in zip(inter, pn):
            if prob[sp] < np.float32(v):
                prob[sp], winner[sp] = np.float32(v), aux
                hist[sp].append("fit %d" % aux)
            else:
                hist[sp].append("tested %d" % aux)
    return winner, hist


def _merge_both(lib, sched, S, fit_out, cls64, vol64, n_fg, classes=18):
    """gapro_schedule_merge and gapro_schedule_merge_ex on the same inputs: (five tables of each, winner)."""
    pn, lb, mu, var = fit_out
    res = []
    for ex in (False, True):
        tabs = [np.full(S, 77, np.int32), np.full(S, 77, np.int32), np.full(S, 77, np.float32),
                np.full(S, 77, np.float32), np.full(S, 77, np.float32)]
        args = [sched, _p(pn), _p(lb), _p(mu), _p(var), _p(cls64), _p(vol64), n_fg, classes] + [_p(t) for t in tabs]
        if ex:
            winner = np.full(S, 77, np.int32)
            assert lib.gapro_schedule_merge_ex(*args, _p(winner)) == 0
            res += [tabs, winner]
            # NULL winner: the plain merge
            tabs0 = [np.full(S, 77, t.dtype) for t in tabs]
            assert lib.gapro_schedule_merge_ex(*(args[:9] + [_p(t) for t in tabs0]), None) == 0
            for a, b in zip(tabs, tabs0):
                assert a.tobytes() == b.tobytes()
        else:
            assert lib.gapro_schedule_merge(*args) == 0
            res.append(tabs)
    return res


def test_merge_ex_on_the_golden_scenes(golden):
    lib = _lib.load()
    kw = golden.api_inputs()
    boxes, cls, vol = O.assemble_boxes(kw["coords_float"], kw["instance_cls"], kw["instance_box"],
                                       kw["instance_box_volume"], kw["wall_box"], kw["wall_box_volume"])
    part = O.partition(kw["coords_float"], kw["mask_feats"], kw["spp"], boxes, cls, vol, 0.999)
    bits = np.ascontiguousarray(_occ_bits(part.occ_spp))
    n_bbs = np.ascontiguousarray(part.n_bbs_per_spp.astype(np.int32))
    boxes = np.ascontiguousarray(boxes)
    sched = C.c_void_p()
    assert lib.gapro_schedule_build(part.n_spps, len(boxes), _p(boxes), _p(bits), _p(n_bbs), C.byref(sched)) == 0
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
        S = part.n_spps
        plain, ex, winner = _merge_both(lib, sched, S, fit_out, np.ascontiguousarray(cls.astype(np.int64)),
                                        np.ascontiguousarray(vol.astype(np.float64)), len(kw["instance_box"]))
        for a, b in zip(plain, ex):
            assert a.dtype == b.dtype
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(ex[3], golden["out_mu"])  # and they are the reference's
        want, _ = _replay_winner(events, n_bbs, fit_out[0])
        assert winner.dtype == np.int32
        np.testing.assert_array_equal(winner, want)
        # a superpoint with a winner holds that fit's mu / var; one that was reset keeps stale values (mu != -100)
        n_gp = int((golden["out_mu"] != -100).sum())
        assert (ex[3][winner >= 0] != -100).all() and (winner >= 0).sum() <= n_gp
        if golden.name == "s3_bigspp":
            assert len(fits) == 0 and (winner == -1).all()
        else:
            assert 4 <= n_gp <= 94 and (winner >= 0).any(), (golden.name, n_gp)
            assert winner.max() < len(fits)
    finally:
        lib.gapro_schedule_free(sched)


def test_winner_histories_on_a_hand_built_schedule():
    """Boxes 0 and 1 overlap partially (a GP pair), box 2 lies inside box 1 within the 0.1 offset and overlaps box 0 (a
    second GP pair (0, 2) and a containment verdict (1, 2) -> 2), one superpoint lies in boxes 0, 1 and 2.  With these
    three boxes alone every superpoint tested by two fits lies in boxes 1 and 2 and is reset by the containment event, so
    the tie rule between two fits could not be seen in the final table: box 3 overlaps box 0 only and gives a third pair
    (0, 3), and superpoints in boxes {0, 1, 3} are tested by fits 0 and 2 and by no containment."""
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
        assert [(k, a, b) for k, a, b, _, _ in events] == [(1, 0, 1), (1, 0, 2), (1, 0, 3), (0, 1, 2)]
        assert [e[3] for e in events] == [0, 1, 2, 2]  # fit ids 0, 1, 2; the containment's winning box is 2
        assert [list(e[4]) for e in events] == [[6, 7, 8, 9, 10], [6, 12], [8, 9, 10], [6, 13]]
        # fit outputs chosen here: fit 0 on [6 7 8 9 10], fit 1 on [6 12], fit 2 on [8 9 10]
        pn = np.array([0.9, 0.8, 0.6, 0.7, 0.75, 0.95, 0.85, 0.65, 0.7, 0.5], dtype=np.float32)
        lb = np.array([0, 1, 0, 1, 0, 1, 0, 1, 0, 1], dtype=np.uint8)
        mu = np.arange(10, dtype=np.float32) - 4.5
        var = np.arange(10, dtype=np.float32) + 1.0
        cls64 = np.array([3, 5, 7, 18], dtype=np.int64)
        vol64 = np.array([8.0, 10.0, 1.4, 8.0])
        plain, ex, winner = _merge_both(lib, sched, S, (pn, lb, mu, var), cls64, vol64, 3)
        for a, b in zip(plain, ex):
            np.testing.assert_array_equal(a, b)
        want, hist = _replay_winner(events, n_bbs, pn)
        np.testing.assert_array_equal(winner, want)
        np.testing.assert_array_equal(winner, [-1, -1, -1, -1, -1, -1, -1, 0, 2, 0, 0, -1, 1, -1])
        # history 1: first taken by a fit, later reset by a containment event (it keeps the fit's mu / var, prob 1)
        reset = [sp for sp in range(S) if hist[sp] and hist[sp][0].startswith("fit") and hist[sp][-1] == "contain"]
        assert reset == [6] and winner[6] == -1
        assert ex[2][6] == 1.0 and ex[3][6] == mu[5] and ex[4][6] == var[5] and ex[1][6] == 2
        # history 2: tested by two fits; the later one wins only with a strictly larger p_new
        two = [sp for sp in range(S) if sum(h != "contain" for h in hist[sp]) == 2 and "contain" not in hist[sp]]
        assert two == [8, 9, 10]
        assert hist[8] == ["fit 0", "fit 2"] and winner[8] == 2          # 0.60 < 0.65
        assert hist[9] == ["fit 0", "tested 2"] and winner[9] == 0       # 0.70 == 0.70: the earlier fit stays
        assert hist[10] == ["fit 0", "tested 2"] and winner[10] == 0     # 0.75 > 0.50
        assert pn[3] == pn[8]
        # the labels follow the winner's outputs: superpoint 8 holds fit 2's row 0 (label 1 -> box 3 -> not a foreground
        # instance of the 3), superpoint 9 fit 0's row 3 (label 1 -> box 1)
        assert (ex[0][8], ex[1][8], ex[2][8]) == (18, -100, np.float32(0.65))
        assert (ex[0][9], ex[1][9], ex[2][9]) == (5, 1, np.float32(0.7))
    finally:
        lib.gapro_schedule_free(sched)


def test_point_refine_abi():
    # sizes follow the C declarations (natural alignment): i64 | 2 x i32 | 11 pointers;  i64 | 6 x i32
    assert C.sizeof(_lib.PointRefineScene) == 8 + 2 * 4 + 11 * 8
    assert C.sizeof(_lib.PointRefineModel) == 8 + 6 * 4
    assert _lib.PointRefineScene.sp_row.offset == 32 and _lib.PointRefineScene.var.offset == 96
    assert _lib.PointRefineModel.sem1.offset == 16 and _lib.PointRefineModel.inst2.offset == 28
    lib = _lib.load()
    for name in ("gapro_schedule_merge_ex", "gapro_point_refine_gather", "gapro_point_refine_apply"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.gapro_version() == 200
    # without a device there is no context: every call is refused before it looks at anything else
    scenes = (_lib.PointRefineScene * 1)()
    models = (_lib.PointRefineModel * 1)()
    sp, mp = C.cast(scenes, C.c_void_p), C.cast(models, C.c_void_p)
    assert lib.gapro_point_refine_gather(None, None, 1, 6, sp, sp, 10, sp, sp) == -1
    assert lib.gapro_point_refine_gather(None, None, -1, 6, sp, sp, 10, sp, sp) == -1
    assert lib.gapro_point_refine_gather(None, None, 1, 6, sp, sp, -1, sp, sp) == -1
    assert lib.gapro_point_refine_gather(None, None, 1, 6, None, None, 10, None, None) == -1
    assert lib.gapro_point_refine_gather(None, None, 1, 6, sp, sp, 2 ** 31, sp, sp) == -1
    assert lib.gapro_point_refine_apply(None, None, 1, sp, sp, 1, mp, mp, 10, sp, sp, sp, sp, sp, None) == -1
    assert lib.gapro_point_refine_apply(None, None, -1, sp, sp, -1, mp, mp, -1, sp, sp, sp, sp, sp, None) == -1
    assert lib.gapro_point_refine_apply(None, None, 1, None, None, 1, None, None, 10, None, None, None, None, None,
                                        None) == -1
    z = np.zeros(4, np.int32)
    assert lib.gapro_schedule_merge_ex(None, None, None, None, None, None, None, 0, 18, _p(z), _p(z), _p(z), _p(z), _p(z),
                                       _p(z)) == -1


def test_vote_refuses_a_model_whose_two_boxes_are_equal():
    """Equal boxes make both labels of a segment argue for one box: rule 3 of the vote keys a candidate by the voters of ONE
    label while rule 4 sums mu / var over both, so the means would cover more rows than they are divided by.  The call
    refuses such a model with GAPRO_ERR_BAD_ARG in its loop over the models, which runs before the block checks and
    before the first copy or launch.  Without a device there is no context and the call returns before that loop, so the
    return code alone proves nothing here: the order is read off the source, with tables that every other check of the
    call accepts (tests/test_point_refine_edges_gpu.py holds the refusal with a context, the message and the untouched
    tables)."""
    import os
    import re

    import point_refine_cases as pc

    c = pc.vote_edge_case()
    boxes = c["boxes"].copy()
    assert (boxes[:, 0] != boxes[:, 1]).all() and (boxes >= 0).all()
    boxes[17, 1] = boxes[17, 0]
    nb, ng, nm = len(c["blocks"]), len(c["segs"]), len(boxes)
    # valid-looking scene and block arguments: the restated host checks pass, the superpoints are inside their scenes
    assert pc.check_blocks(c["blocks"], c["segs"], c["R"], c["R2"], 2, nm) is None
    assert (c["block_spp"] < np.asarray(c["n_spps"])[c["blocks"][:, 2]]).all() and c["blocks"][:, 4].max() <= 2048
    blocks, segs, models = pc.block_table(c["blocks"]), pc.segment_table(c["segs"]), pc.model_table(c["pairs"], 0)
    tabs = [np.zeros(max(c["n_spps"]), np.int32) for _ in range(5)]
    scenes = (_lib.PointRefineVoteScene * 2)()
    for q, s in zip(scenes, c["n_spps"]):
        q.sem_spp, q.inst_spp, q.prob_spp, q.mu_spp, q.var_spp = (t.ctypes.data for t in tabs)
        q.n_spps = s
    lib = _lib.load()
    sp = C.cast(scenes, C.c_void_p)
    rows = [_p(c["pn"]), _p(c["lab"]), _p(c["mu"]), _p(c["var"])]
    bspp = np.ascontiguousarray(c["block_spp"])
    for bx in (boxes, c["boxes"]):
        bx = np.ascontiguousarray(bx)
        assert lib.gapro_point_refine_vote(None, None, 2, sp, sp, nm, _p(models), _p(models), _p(bx), _p(bx), nb, _p(blocks),
                                           _p(blocks), _p(bspp), _p(bspp), ng, _p(segs), _p(segs), c["R"], c["R2"], *rows,
                                           None, None) == -1
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "gapro_amd", "csrc", "point_refine.hip")) as f:
        text = f.read()
    body = text[text.index("int gapro_point_refine_vote("):]
    test = body.index("h_model_boxes[2 * k] == h_model_boxes[2 * k + 1]")
    loop = body.rindex("for (int k = 0; k < n_models; ++k)", 0, test)
    fail = body.index("gapro_fail(ctx, GAPRO_ERR_BAD_ARG", test)
    assert re.search(r'"gapro_point_refine_vote: model %d:', body[fail:fail + 200])  # the message names the model
    assert loop < test < fail < body.index("check_blocks(") < body.index("hipMemcpyAsync") < body.index("hipLaunchKernelGGL")
    assert body[loop:fail].count(";") == 2  # the loop header only: nothing between the test and the refusal
    with open(os.path.join(root, "include", "gapro_hip.h")) as f:
        header = " ".join(f.read().split())
    assert "also refused: a negative box, * a model whose two boxes are equal" in header
