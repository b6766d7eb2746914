"""Stage G of the pipeline, the opt-in ``point_level`` path: per-point GP labels inside GP-labelled superpoints.

Three modes share one host plan shape and one device chain:

  plan    refine_plan: plan_point_winner ("winner") or plan_point_compete ("compete", "vote"), pure NumPy
  chain   refine_chain: scene table -> gather -> expand (where the plan has segments) -> ONE predict launch -> the
          mode's tail -> status read-back
  tails   "winner": apply with the models; "compete": apply (mu / var only), then compete; "vote": the superpoint
          vote on the merge's tables, in front of the label broadcast

Plain functions; the ones that need device facilities take the runner (the Pipeline) first.  A Pipeline without
``point_level`` runs nothing of this module beyond point_mode.
"""
from __future__ import annotations

import ctypes as C
import time

import numpy as np

from ._lib import GaproError, PointRefineModel, PointRefineScene, PointRefineVoteScene, PredictDesc
from .fit_runner import ROW_FIELDS, _host, _ptr, block_views

# the host images of gapro_point_refine_block / gapro_point_refine_segment (include/gapro_hip.h)
BLOCK_DTYPE = np.dtype([("row_start", np.int64), ("n_rows", np.int32), ("scene", np.int32), ("seg_start", np.int32),
                        ("n_seg", np.int32)], align=True)
SEGMENT_DTYPE = np.dtype([("out_start", np.int64), ("model", np.int32), ("reserved", np.int32)], align=True)


def point_mode(point_level):
    """None (off), "winner", "compete" or "vote" for a ``point_level`` argument; ValueError for anything else."""
    if isinstance(point_level, (bool, np.bool_)):
        return "winner" if point_level else None
    if isinstance(point_level, str) and point_level in ("winner", "compete", "vote"):
        return point_level
    raise ValueError("point_level must be False, True, 'winner', 'compete' or 'vote', not %r" % (point_level,))


def point_level_kw(point_level):
    """The Pipeline keyword of a ``point_level`` argument in its one spelling per mode -- {} when off, True for
    "winner" -- so that callers which cache pipelines by their options share one for True and "winner"."""
    mode = point_mode(point_level)
    return dict(point_level=True if mode == "winner" else mode) if mode else {}


# ------------------------------------------------------------------ the host plan
def plan_point_winner(winners, point_counts, fit_bases, descs):
    """Host plan of a batch's point_level="winner" predict launch: pure NumPy, no device.  Inputs as for
    plan_point_compete, without the testers.

    A scene's refined superpoints (winner >= 0) are ordered by (winning fit, superpoint): the superpoints of one fit are
    contiguous and ascending, the fits in batch order.  Every fit that won at least one superpoint becomes a predict
    model whose rows are the points of its superpoints; sp_row[sp] is the first row of the superpoint's block.  The
    predict launch reads the gathered rows in order: expanded_rows == rows, no blocks, no segments.

    Returns dict(sp_row i64[sum S], blocks, segments (both empty), models [(batch fit index, scene, first row, rows,
    b1, b2)], rows R, expanded_rows R, refined_spps)."""
    i64 = np.int64
    sp_row = np.full(int(sum(len(pc) for pc in point_counts)), -1, dtype=i64)
    models, rows, n_ref, base = [], 0, 0, 0
    for si, (w, pc, fb) in enumerate(zip(winners, point_counts, fit_bases)):
        w = np.asarray(w) if w is not None else np.zeros(0, i64)
        ref = np.nonzero(w >= 0)[0]
        if len(ref):
            order = ref[np.argsort(w[ref], kind="stable")]
            cnt = np.asarray(pc)[order].astype(i64)
            start = rows + np.cumsum(cnt) - cnt
            sp_row[base + order] = start
            fit_ids, first = np.unique(w[order], return_index=True)
            for k, a, b in zip(fit_ids, first, np.r_[first[1:], len(order)]):
                d = descs[fb + int(k)]
                models.append((fb + int(k), si, int(start[a]), int(cnt[a:b].sum()), int(d.b1), int(d.b2)))
            rows += int(cnt.sum())
            n_ref += len(ref)
        base += len(pc)
    return dict(sp_row=sp_row, blocks=np.zeros(0, BLOCK_DTYPE), segments=np.zeros(0, SEGMENT_DTYPE), models=models,
                rows=rows, expanded_rows=rows, refined_spps=n_ref)


def plan_point_compete(winners, point_counts, testers, fit_bases, descs=None):
    """Host plan of a batch's point_level="compete" predict launch: pure NumPy, no device.

    Per scene: ``winners[i]`` i32[S] (gapro_schedule_merge_ex; None = the scene takes no part), ``point_counts[i]``
    i32[S], ``testers[i]`` = (offsets i64[S + 1], fit i32[n], pos i32[n]) from gapro_schedule_export_testers,
    ``fit_bases[i]`` = index of the scene's first fit among the batch's fit descriptors ``descs`` (optional; with them
    every model carries its b1, b2).

    A superpoint is refined iff winner >= 0.  Its points form one BLOCK of the gathered row table, the blocks ordered by
    (scene, superpoint): sp_row[sp] = first row, R rows in all.  Every fit that tested a refined superpoint is a predict
    MODEL (scene order, then fit order); a (tester, block) pair is a SEGMENT of the block's n_rows entries in the predict
    launch's row list, R2 entries in all.  The segments of a block are stored in tester order (the order in which the
    merge meets the fits); in the row list the segments of one model are contiguous, ascending in superpoint.

    Returns dict(sp_row i64[sum S], blocks BLOCK_DTYPE[], segments SEGMENT_DTYPE[], models [(batch fit index, scene,
    first entry, entries, b1, b2)], rows R, expanded_rows R2, refined_spps, multi_spps, scene_rows [(first row, rows)])."""
    i64 = np.int64
    sp_row = np.full(int(sum(len(pc) for pc in point_counts)), -1, dtype=i64)
    blocks, segs, models, scene_rows = [], [], [], []
    R = R2 = n_seg_tot = multi = n_ref = base = 0
    for si, (w, pc, (t_off, t_fit, _), fb) in enumerate(zip(winners, point_counts, testers, fit_bases)):
        S = len(pc)
        ref = np.nonzero(np.asarray(w) >= 0)[0] if w is not None else np.zeros(0, i64)
        scene_rows.append((R, 0))
        if len(ref):
            t_off = np.asarray(t_off, dtype=i64)
            cnt = np.asarray(pc)[ref].astype(i64)
            start = R + np.cumsum(cnt) - cnt
            sp_row[base + ref] = start
            ns = t_off[ref + 1] - t_off[ref]
            first_seg = np.cumsum(ns) - ns
            tot = int(ns.sum())
            blk = np.zeros(len(ref), dtype=BLOCK_DTYPE)
            blk["row_start"], blk["n_rows"], blk["scene"] = start, cnt, si
            blk["seg_start"], blk["n_seg"] = n_seg_tot + first_seg, ns
            blocks.append(blk)
            blk_of_seg = np.repeat(np.arange(len(ref)), ns)
            fit = np.asarray(t_fit)[np.repeat(t_off[ref] - first_seg, ns) + np.arange(tot)]
            order = np.argsort(fit, kind="stable")  # the row list: by (fit, superpoint)
            rows_o = cnt[blk_of_seg[order]]
            out_o = R2 + np.cumsum(rows_o) - rows_o
            sg = np.zeros(tot, dtype=SEGMENT_DTYPE)
            sg["out_start"][order] = out_o
            fits_u, first = np.unique(fit[order], return_index=True)
            sg["model"] = len(models) + np.searchsorted(fits_u, fit)
            segs.append(sg)
            for k, a, b in zip(fits_u, first, np.r_[first[1:], tot]):
                d = descs[fb + int(k)] if descs is not None else None
                models.append((fb + int(k), si, int(out_o[a]), int(rows_o[a:b].sum()),
                               int(d.b1) if d is not None else -1, int(d.b2) if d is not None else -1))
            scene_rows[-1] = (R, int(cnt.sum()))
            R += int(cnt.sum())
            R2 += int(rows_o.sum())
            n_seg_tot += tot
            multi += int((ns >= 2).sum())
            n_ref += len(ref)
        base += S
    return dict(sp_row=sp_row, blocks=np.concatenate(blocks) if blocks else np.zeros(0, BLOCK_DTYPE),
                segments=np.concatenate(segs) if segs else np.zeros(0, SEGMENT_DTYPE), models=models, rows=R,
                expanded_rows=R2, refined_spps=n_ref, multi_spps=multi, scene_rows=scene_rows)


def refine_plan(runner, state):
    """Host plan of the batch's point-level predict launch, from each scene's merge winners and point counts (no device
    round trip); "compete" and "vote" also ask every schedule for its testers.  Scenes that already failed take no
    part.  Row indices are int32 (the predict ABI): a longer row list is refused here, before anything is launched.
    Sets ``runner.last_refine``."""
    t0 = time.perf_counter()
    jobs = state.jobs
    winners = [j.host["winner"] if j.error is None else None for j in jobs]
    counts, bases = [j.host["point_count"] for j in jobs], [j.fit_base for j in jobs]
    if runner.point_mode == "winner":
        plan, what = plan_point_winner(winners, counts, bases, state.descs), "rows"
    else:
        testers = []
        for job in jobs:
            off = np.zeros(job.n_spps + 1, dtype=np.int64)
            fit = np.zeros(max(int(job.counts.n_fit_out), 1), dtype=np.int32)
            pos = np.zeros_like(fit)
            rc = runner.lib.gapro_schedule_export_testers(job.schedule, _ptr(off), _ptr(fit), _ptr(pos))
            if rc != 0:
                raise GaproError(rc, "gapro_schedule_export_testers")
            testers.append((off, fit, pos))
        plan, what = plan_point_compete(winners, counts, testers, bases, state.descs), "expanded rows"
    if plan["expanded_rows"] > 2**31 - 1:
        raise GaproError(-1, "point_level: %d %s in one batch exceed the int32 row index" % (plan["expanded_rows"], what))
    last = dict(refined_spps=plan["refined_spps"], rows=plan["rows"], models=len(plan["models"]),
                expanded_rows=plan["expanded_rows"])
    if "multi_spps" in plan:
        last["multi_spps"] = plan["multi_spps"]
    runner.last_refine = dict(last, plan_s=time.perf_counter() - t0)
    return plan


# ------------------------------------------------------------------ the chain
def mark_failed(status, models, jobs, strict):
    """A predict model whose status is not 0 fails its scene like a failed fit: ``job.error`` (the first failure of a
    scene stands, and so does an error the scene already carries); ``strict`` raises the first error in job order."""
    if (status != 0).any():
        for k in np.nonzero(status)[0]:
            job = jobs[models[k][1]]
            if job.error is None:
                job.error = GaproError(int(status[k]), "point-level prediction from GP fit %d of the scene failed"
                                       % (models[k][0] - job.fit_base))
        if strict:
            raise next(j.error for j in jobs if j.error is not None)


def _pair(job, b1: int, b2: int):
    """(sem, inst) of a point labelled 0 (box b1) and 1 (box b2): the merge's last loop (schedule.cpp) for a box."""
    n_fg, pair = len(job.instance_box), []
    for box in (b1, b2):
        pair += [int(job.boxes_cls[box]), box if box < n_fg else -100]
    return pair


def _identity_rows(runner, n: int):
    """i32[>= n] = 0, 1, 2, .. on the device (grow-only): the predict launch reads the gathered table in order."""
    cur = runner._ident_rows
    if cur is None or cur.numel() < n:
        cur = runner._ident_rows = runner.be.from_numpy(np.arange(max(n, 1 << 16) * 5 // 4, dtype=np.int32))
        runner.be.current_stream().synchronize()  # every pipeline stream reads it from now on
    return cur


def refine_chain(runner, state, plan, offs, d_tables):
    """The device chain of a planned batch, on the current stream: gather the refined superpoints' points into the row
    table, expand it to the row list where the plan has segments, ONE gapro_svgp_predict_batch over it (identity rows
    otherwise), then the mode's tail:

      "winner"   apply: mu / var broadcast, then every row's five values to its point
      "compete"  apply (mu / var broadcast alone), then compete: the merge per row.  keep_models: ``job.point_fit``
                 i32[N], the scene-local fit that labelled each point, -1 elsewhere
      "vote"     vote: the five superpoint values of every refined superpoint rewritten in ``d_tables`` (``offs``: each
                 scene's first byte) -- the caller runs this IN FRONT of the label broadcast, the other two behind it.
                 keep_models: ``job.vote_box`` / ``job.vote_count`` i32[S], and ``job.winner`` (a copy: job.host's
                 stays the merge's) becomes the representative fit where a vote took place

    A batch without a refined superpoint runs neither gather nor predict: only apply's mu / var broadcast, and nothing
    at all for "vote".  The one host wait is the read of the per-model status behind the last kernel; a failed model
    fails its scene (mark_failed).  Returns what must stay alive until the stream has run all of it."""
    lib, ctx, be = runner.lib, runner.ctx, runner.be
    mode, jobs, keep_models = runner.point_mode, state.jobs, state.keep_models
    R, R2, models = plan["rows"], plan["expanded_rows"], plan["models"]
    blocks, segs = plan["blocks"], plan["segments"]
    ns, nm, nb, nsg = len(jobs), len(models), len(blocks), len(segs)
    if keep_models:
        for job in jobs:
            if mode == "compete":
                job.point_fit = np.full(job.n_points, -1, dtype=np.int32)
            elif mode == "vote":
                if job.winner is not None:
                    job.winner = job.winner.copy()
                job.vote_box = np.full(job.n_spps, -1, dtype=np.int32)
                job.vote_count = np.zeros(job.n_spps, dtype=np.int32)
    runner._stage("broadcast")  # (the name of the chain's start in every mode; "vote" has broadcast nothing yet)
    if mode == "vote" and R == 0:
        return []
    # the scene table: what gather and apply / compete read of a scene ("vote": its superpoint tables in a second one)
    scenes = (PointRefineScene * ns)()
    d_scenes = be.empty(ns * C.sizeof(PointRefineScene))
    d_sp_row = be.from_numpy(plan["sp_row"])
    d_cursor = be.empty(4 * len(plan["sp_row"]))
    keep = [scenes, d_scenes, d_sp_row, d_cursor]
    if mode == "vote":
        vscenes = (PointRefineVoteScene * ns)()
        d_vscenes = be.empty(ns * C.sizeof(PointRefineVoteScene))
        keep += [vscenes, d_vscenes]
    base, tab = 0, d_tables.data_ptr()
    for i, (t, job, off) in enumerate(zip(scenes, jobs, offs)):
        S = job.n_spps
        t.n_points, t.n_spps, t.reserved = job.n_points, S, 0
        t.spp_inv, t.feats = job.dev["spp_inv"].data_ptr(), job.feats.data_ptr()
        t.sp_row, t.cursor = d_sp_row.data_ptr() + 8 * base, d_cursor.data_ptr() + 4 * base
        if mode == "vote":
            v = vscenes[i]
            v.sem_spp, v.inst_spp, v.prob_spp = tab + off, tab + off + 4 * S, tab + off + 8 * S
            v.mu_spp, v.var_spp, v.n_spps, v.reserved = tab + off + 12 * S, tab + off + 16 * S, S, 0
        else:
            t.mu_spp, t.var_spp = (x.data_ptr() for x in job.dev["mu_var_spp"])
            t.sem, t.inst, t.prob, t.mu, t.var = (x.data_ptr() for x in job.outputs)
        base += S
    sp = C.cast(scenes, C.c_void_p)

    def apply(n=0, *rows):
        """gapro_point_refine_apply with n models and their rows; without any, its mu / var broadcast alone"""
        rows = rows or (None, None, 0, None, None, None, None, None, None)
        ctx.check(lib.gapro_point_refine_apply(ctx.handle, runner._sh(), ns, sp, _ptr(d_scenes), n, *rows))
        runner._stage("apply")

    if R == 0:
        apply()
        return keep
    D = int(state.feats_spp_all.shape[1])
    row_feats = be.empty_typed((R, D), be.f32)
    row_point = be.empty(4 * R)
    ctx.check(lib.gapro_point_refine_gather(ctx.handle, runner._sh(), ns, D, sp, _ptr(d_scenes), R, _ptr(row_feats),
                                            _ptr(row_point)))
    runner._stage("gather")
    if nsg:
        d_blocks, d_segs = be.empty(nb * BLOCK_DTYPE.itemsize), be.empty(nsg * SEGMENT_DTYPE.itemsize)
        d_rows = be.empty(4 * R2)
        ctx.check(lib.gapro_point_refine_expand(ctx.handle, runner._sh(), nb, _ptr(blocks), _ptr(d_blocks), nsg,
                                                _ptr(segs), _ptr(d_segs), R, R2, _ptr(d_rows)))
        runner._stage("expand")
        keep += [blocks, segs, d_blocks, d_segs, d_rows]
    else:
        d_rows = _identity_rows(runner, R)
    pd = (PredictDesc * nm)()
    rm = (PointRefineModel * nm)()
    h_m = np.empty(nm, dtype=np.int32)
    off = state.pending.state_off
    for k, (q, r, (f, si, row0, t, b1, b2)) in enumerate(zip(pd, rm, models)):
        q.state_offset, q.row_offset, q.out_offset, q.t, q.reserved = int(off[f]), row0, row0, t, 0
        r.row_offset, r.t, r.scene = row0, t, si
        r.sem1, r.inst1, r.sem2, r.inst2 = _pair(jobs[si], b1, b2)
        h_m[k] = int(state.descs[f].m1 + state.descs[f].m2)
    out, pstat = runner._predict_launch(state.pending.d_state, h_m, pd, row_feats, d_rows, R2)
    runner._stage("predict")
    o = block_views(ROW_FIELDS, out, R2, be)
    res = (_ptr(o["probs_new"]), _ptr(o["labels"]), _ptr(o["mu"]), _ptr(o["var"]), _ptr(pstat))
    d_models = be.empty(nm * C.sizeof(PointRefineModel))
    keep += [rm, d_models, pd, row_feats, row_point, out, pstat]
    if mode == "winner":
        apply(nm, C.cast(rm, C.c_void_p), _ptr(d_models), R, _ptr(row_point), *res)
    elif mode == "compete":
        apply()
        row_model = be.empty(4 * R) if keep_models else None
        ctx.check(lib.gapro_point_refine_compete(
            ctx.handle, runner._sh(), ns, sp, _ptr(d_scenes), nm, C.cast(rm, C.c_void_p), _ptr(d_models), nb,
            _ptr(blocks), _ptr(d_blocks), nsg, _ptr(segs), _ptr(d_segs), R, R2, _ptr(row_point), *res, _ptr(row_model)))
        runner._stage("compete")
        keep.append(row_model)
    else:
        boxes = np.array([m[4:6] for m in models], dtype=np.int32)
        # the blocks are in (scene, superpoint) order (plan_point_compete): their scene-local superpoints
        block_spp = np.concatenate([np.nonzero(np.asarray(j.host["winner"]) >= 0)[0] for j in jobs
                                    if j.error is None] or [np.zeros(0, np.int64)]).astype(np.int32)
        assert len(block_spp) == nb
        d_boxes, d_block_spp = be.empty(8 * nm), be.empty(4 * nb)
        block_out = be.empty(12 * nb) if keep_models else None
        ctx.check(lib.gapro_point_refine_vote(
            ctx.handle, runner._sh(), ns, C.cast(vscenes, C.c_void_p), _ptr(d_vscenes), nm, C.cast(rm, C.c_void_p),
            _ptr(d_models), _ptr(boxes), _ptr(d_boxes), nb, _ptr(blocks), _ptr(d_blocks), _ptr(block_spp),
            _ptr(d_block_spp), nsg, _ptr(segs), _ptr(d_segs), R, R2, *res, _ptr(block_out)))
        runner._stage("vote")
        keep += [boxes, d_boxes, block_spp, d_block_spp, block_out]
    mark_failed(_host(pstat).view(np.int32)[:nm], models, jobs, runner.strict)  # the batch waits here for its predicts
    if keep_models and mode != "winner":
        fit_of = np.array([m[0] for m in models], dtype=np.int64)
        if mode == "compete":
            h_model = _host(row_model).view(np.int32)[:R]
            h_point = _host(row_point).view(np.int32)[:R]
            for job, (a, n) in zip(jobs, plan["scene_rows"]):
                took = h_model[a:a + n]
                ok = took >= 0
                job.point_fit[h_point[a:a + n][ok]] = (fit_of[took[ok]] - job.fit_base).astype(np.int32)
        else:
            h_out = _host(block_out).view(np.int32)[:3 * nb].reshape(nb, 3)
            for b in np.nonzero(h_out[:, 0] >= 0)[0]:
                job, s = jobs[int(blocks["scene"][b])], int(block_spp[b])
                job.winner[s] = int(fit_of[h_out[b, 0]]) - job.fit_base
                job.vote_box[s], job.vote_count[s] = h_out[b, 1], h_out[b, 2]
    return keep
