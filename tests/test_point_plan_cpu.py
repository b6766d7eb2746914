"""Host side of stage G (gapro_amd/point_level.py; no GPU and no library needed): plan_point_winner against a restatement
in plain loops and against plan_point_compete where the two must agree, the failure marking, the ``point_level``
normalisation, and the order of library calls and stage events of the one chain in every mode, driven by a stub runner."""
from types import SimpleNamespace as NS

import numpy as np
import pytest

from gapro_amd._lib import GaproError
from gapro_amd.point_level import (mark_failed, plan_point_compete, plan_point_winner, point_level_kw, refine_chain,
                                   refine_plan)


def _descs(n):
    return [NS(b1=10 + k, b2=20 + 2 * k, m1=3, m2=4) for k in range(n)]


def _winner_by_loops(winners, point_counts, fit_bases, descs):
    """plan_point_winner's rules, one superpoint at a time: (sp_row, models, rows)."""
    sp_row, models, rows = [], [], 0
    for si, (w, pc, fb) in enumerate(zip(winners, point_counts, fit_bases)):
        row_of = [-1] * len(pc)
        for k in sorted({int(x) for x in w if x >= 0}) if w is not None else []:
            first = rows
            for sp in range(len(pc)):
                if w[sp] == k:
                    row_of[sp] = rows
                    rows += int(pc[sp])
            models.append((fb + k, si, first, rows - first, descs[fb + k].b1, descs[fb + k].b2))
        sp_row += row_of
    return sp_row, models, rows


# three scenes: one that takes no part, one without a refined superpoint, one whose winners are out of superpoint order
WINNERS = [None, np.full(4, -1, np.int32), np.array([5, -1, 0, 2, 5, 0, -1, 2, 2, 0, -1, 5], np.int32)]
COUNTS = [np.array([3, 1, 2], np.int32), np.array([2, 2, 1, 7], np.int32),
          np.array([1, 9, 40, 1, 3, 2, 5, 1, 17, 6, 4, 8], np.int32)]
BASES = [2, 5, 9]


def test_plan_point_winner_against_loops():
    descs = _descs(16)
    plan = plan_point_winner(WINNERS, COUNTS, BASES, descs)
    sp_row, models, rows = _winner_by_loops(WINNERS, COUNTS, BASES, descs)
    assert plan["sp_row"].dtype == np.int64 and plan["sp_row"].tolist() == sp_row
    assert plan["models"] == models and [m[0] for m in models] == [9, 11, 14] and models[0][4:] == (19, 38)
    assert plan["rows"] == plan["expanded_rows"] == rows == 79 and plan["refined_spps"] == 9
    assert len(plan["blocks"]) == 0 and len(plan["segments"]) == 0
    # sp_row is -1 exactly on the unrefined superpoints; the row blocks are disjoint and cover [0, rows)
    flat_w = np.concatenate([np.full(3, -1), WINNERS[1], WINNERS[2]])
    flat_c = np.concatenate(COUNTS)
    assert ((plan["sp_row"] == -1) == (flat_w < 0)).all()
    taken = np.zeros(rows, dtype=np.int32)
    for sp in np.nonzero(flat_w >= 0)[0]:
        taken[plan["sp_row"][sp]:plan["sp_row"][sp] + flat_c[sp]] += 1
    assert (taken == 1).all()
    # a model's entries are contiguous, the models in (scene, fit) order, ascending superpoints inside
    at = 0
    for f, si, row0, t, b1, b2 in plan["models"]:
        assert row0 == at and si == 2 and (b1, b2) == (descs[f].b1, descs[f].b2)
        mine = np.nonzero(WINNERS[2] == f - BASES[2])[0]
        assert (np.diff(plan["sp_row"][7 + mine]) > 0).all() and plan["sp_row"][7 + mine[0]] == row0
        assert t == int(COUNTS[2][mine].sum())
        at += t
    assert at == rows and [m[:2] for m in plan["models"]] == sorted(m[:2] for m in plan["models"])
    empty = plan_point_winner([], [], [], [])
    assert (empty["rows"], empty["expanded_rows"], empty["models"], len(empty["sp_row"])) == (0, 0, [], 0)
    assert len(empty["blocks"]) == 0 and len(empty["segments"]) == 0


def _hand_built(winner):
    """The four-box schedule of tests/test_point_compete_cpu.py, from its rule: fit 0 lists superpoints [6 7 8 9 10],
    fit 1 [6 12], fit 2 [8 9 10]; a superpoint's testers are the fits that list it, in fit order."""
    S, lists = 14, [[6, 7, 8, 9, 10], [6, 12], [8, 9, 10]]
    per = [[(k, ls.index(sp)) for k, ls in enumerate(lists) if sp in ls] for sp in range(S)]
    off = np.cumsum([0] + [len(p) for p in per]).astype(np.int64)
    fit = np.array([k for p in per for k, _ in p], np.int32)
    pos = np.array([j for p in per for _, j in p], np.int32)
    pc = np.full(S, 9, np.int32)
    pc[[7, 8, 9, 10, 12]] = [3, 1, 4, 2, 5]
    return np.array(winner, np.int32), pc, (off, fit, pos)


def test_the_two_planners_agree_where_one_fit_tests_a_superpoint():
    scenes = [_hand_built([-1, -1, -1, -1, -1, -1, -1, 0, 2, 0, 0, -1, 1, -1]),  # the winners the merge gives there
              _hand_built([-1, -1, -1, -1, -1, -1, -1, 0, 0, 2, 2, -1, 1, -1])]
    winners, counts, testers = ([s[i] for s in scenes] for i in range(3))
    descs = _descs(6)
    pw = plan_point_winner(winners, counts, [0, 3], descs)
    pcm = plan_point_compete(winners, counts, testers, [0, 3], descs)
    assert pw["rows"] == pcm["rows"] == 30 and pw["refined_spps"] == pcm["refined_spps"] == 10
    # the rows a superpoint holds in the winner plan: up to the next block's first row
    starts = np.sort(pw["sp_row"][pw["sp_row"] >= 0])
    n_rows = dict(zip(starts.tolist(), np.diff(np.r_[starts, pw["rows"]]).tolist()))
    block_of = np.nonzero(pcm["sp_row"] >= 0)[0]  # blocks are in (scene, superpoint) order
    single = 0
    for b, sp in zip(pcm["blocks"], block_of):
        if b["n_seg"] == 1:
            assert n_rows[int(pw["sp_row"][sp])] == b["n_rows"]
            single += 1
    assert single == 4  # superpoints 7 and 12 of either scene


def _jobs(errors=(None, None, None)):
    return [NS(error=e, fit_base=fb) for e, fb in zip(errors, (0, 4, 9))]


def test_mark_failed():
    models = [(1, 0, 0, 5, 0, 1), (5, 1, 5, 3, 0, 1), (7, 1, 8, 2, 0, 2), (10, 2, 10, 4, 1, 2)]
    jobs = _jobs()
    mark_failed(np.zeros(4, np.int32), models, jobs, True)
    assert [j.error for j in jobs] == [None, None, None]
    # two failed models of one scene leave the first one's error, which names the scene-local fit
    mark_failed(np.array([0, -3, -4, 0], np.int32), models, jobs, False)
    assert jobs[0].error is None and jobs[2].error is None and isinstance(jobs[1].error, GaproError)
    assert "point-level prediction from GP fit 1 of the scene failed" in str(jobs[1].error)
    assert jobs[1].error.code == -3
    # a job that already carries an error keeps it; strict raises the first error in job order
    earlier = ValueError("earlier")
    jobs = _jobs((None, earlier, None))
    mark_failed(np.array([0, -3, 0, -5], np.int32), models, jobs, False)
    assert jobs[0].error is None and jobs[1].error is earlier and jobs[2].error.code == -5
    assert "GP fit 1 of the scene failed" in str(jobs[2].error)
    jobs = _jobs()
    with pytest.raises(GaproError, match="GP fit 3 of the scene failed") as exc:
        mark_failed(np.array([0, 0, -3, -5], np.int32), models, jobs, True)
    assert exc.value is jobs[1].error and jobs[2].error.code == -5 and jobs[0].error is None
    jobs = _jobs((earlier, None, None))
    with pytest.raises(ValueError, match="earlier"):
        mark_failed(np.array([0, 0, -3, 0], np.int32), models, jobs, True)
    assert "GP fit 3 of the scene failed" in str(jobs[1].error)


def test_point_level_kw():
    assert point_level_kw(False) == {} and point_level_kw(np.bool_(False)) == {}
    assert point_level_kw(True) == point_level_kw("winner") == point_level_kw(np.bool_(True)) == dict(point_level=True)
    assert point_level_kw("compete") == dict(point_level="compete") and point_level_kw("vote") == dict(point_level="vote")
    for bad in ("Winner", 1, None):
        with pytest.raises(ValueError):
            point_level_kw(bad)


# ---------------------------------------------------------------------- the chain on a stub runner
class _Buf:
    """A device buffer as far as the chain looks at one: address, slices, re-typing, a blocking copy to the host."""

    def __init__(self, n=0, shape=None):
        self.a, self.shape = np.zeros(max(int(n), 1), np.uint8), shape

    def data_ptr(self):
        return self.a.ctypes.data

    def __getitem__(self, s):
        b = _Buf()
        b.a = self.a[s]
        return b

    def view(self, _):
        return self

    def numel(self):
        return len(self.a)

    def cpu(self):
        return self.a


def _stub(mode, winner):
    """A runner that logs the library entry points (apply with its model count) and the stage events of one scene."""
    log = []

    class Lib:
        def __getattr__(self, name):
            return lambda *a: log.append(name + (":%d" % a[5] if name.endswith("apply") else "")) or 0

    be = NS(empty=_Buf, from_numpy=lambda a: _Buf(a.nbytes), empty_typed=lambda shape, _: _Buf(4 * shape[0] * shape[1], shape),
            f32=0, u8=0, current_stream=lambda: NS(synchronize=lambda: None))

    def predict(d_state, h_m, pd, feats, d_rows, no):
        log.append("gapro_svgp_predict_batch")
        return _Buf(17 * no), _Buf(4 * len(h_m))

    runner = NS(lib=Lib(), ctx=NS(handle=None, check=lambda rc: None), be=be, point_mode=mode, strict=True,
                _ident_rows=None, _sh=lambda: None, _stage=log.append, _predict_launch=predict)
    winner, pc, testers = _hand_built(winner)
    S = len(pc)
    job = NS(n_points=int(pc.sum()), n_spps=S, feats=_Buf(8), outputs=[_Buf(8) for _ in range(5)], error=None,
             dev=dict(spp_inv=_Buf(8), mu_var_spp=(_Buf(8), _Buf(8))), host=dict(winner=winner, point_count=pc),
             fit_base=0, instance_box=np.zeros((3, 6)), boxes_cls=np.array([3, 5, 7, 18]))
    descs = [NS(b1=0, b2=k + 1, m1=3, m2=4) for k in range(3)]
    state = NS(jobs=[job], keep_models=False, descs=descs, feats_spp_all=_Buf(8, (S, 6)),
               pending=NS(state_off=np.arange(3) * 100, d_state=_Buf(8)))
    plan = plan_point_winner([winner], [pc], [0], descs) if mode == "winner" else \
        plan_point_compete([winner], [pc], [testers], [0], descs)
    return runner, state, plan, log


HEAD = ["broadcast", "gapro_point_refine_gather", "gather"]
EXPAND = ["gapro_point_refine_expand", "expand"]
PREDICT = ["gapro_svgp_predict_batch", "predict"]
SEQUENCES = {
    "winner": HEAD + PREDICT + ["gapro_point_refine_apply:3", "apply"],
    "compete": HEAD + EXPAND + PREDICT + ["gapro_point_refine_apply:0", "apply", "gapro_point_refine_compete", "compete"],
    "vote": HEAD + EXPAND + PREDICT + ["gapro_point_refine_vote", "vote"],
}


@pytest.mark.parametrize("mode", ["winner", "compete", "vote"])
def test_call_sequence_of_the_chain(mode):
    runner, state, plan, log = _stub(mode, [-1, -1, -1, -1, -1, -1, -1, 0, 2, 0, 0, -1, 1, -1])
    keep = refine_chain(runner, state, plan, [0], _Buf(20 * 14))
    assert log == SEQUENCES[mode] and len(keep) >= 11
    assert (runner._ident_rows is not None) == (mode == "winner")  # identity rows for "winner", the expanded list else
    # nothing refined: apply's mu / var broadcast alone; "vote" launches nothing and builds no scene table
    runner, state, plan, log = _stub(mode, [-1] * 14)
    keep = refine_chain(runner, state, plan, [0], _Buf(20 * 14))
    if mode == "vote":
        assert log == ["broadcast"] and keep == []
    else:
        assert log == ["broadcast", "gapro_point_refine_apply:0", "apply"] and len(keep) == 4


def test_refine_plan_sets_last_refine_and_refuses_long_row_lists():
    runner, state, _, log = _stub("winner", [-1, -1, -1, -1, -1, -1, -1, 0, 2, 0, 0, -1, 1, -1])
    plan = refine_plan(runner, state)
    last = dict(runner.last_refine)
    assert last.pop("plan_s") >= 0 and log == []
    assert last == dict(refined_spps=5, rows=15, models=3, expanded_rows=15) and plan["rows"] == 15
    state.jobs[0].host["point_count"] = np.full(14, 2 ** 29, np.int32)  # 5 refined superpoints: 5 * 2^29 rows
    with pytest.raises(GaproError, match=r"point_level: 2684354560 rows in one batch exceed the int32 row index"):
        refine_plan(runner, state)
    state.jobs[0].error = ValueError("failed before the plan")  # such a scene takes no part
    assert refine_plan(runner, state)["rows"] == 0 and runner.last_refine["refined_spps"] == 0
