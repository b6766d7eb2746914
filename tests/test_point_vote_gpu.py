"""point_level="vote" on the MI355X: gapro_point_refine_vote on hand-made blocks, and Pipeline(point_level="vote") against
the NumPy assembly from the kept models.

Every comparison is bit for bit.  The vote counts with integer atomics; its three values are int64 fixed-point sums
(exact, so no order reaches them), one ldexp, one float64 division and one rounding to float32, which tests/vote_ref.py
restates; the chain and the assembly run the same predict kernel on the same states and feature rows (a predict row's
result does not depend on what shares its launch).  No tolerance applies."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import vote_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ("coords_float", "mask_feats", "spp", "instance_cls", "instance_box", "instance_box_volume", "wall_box",
        "wall_box_volume")
OPTS = dict(instance_classes=18, ground_h=0.1, thresh_spp_occu=0.999)
NAMES = ("s0_walls", "s2_dense", "s3_bigspp")
N_FG = 10  # the contract's boxes 0 .. 13: 10 and beyond are walls (inst -100)


def _np(t):
    if isinstance(t, np.ndarray):
        return t
    h = t.cpu()
    return h if isinstance(h, np.ndarray) else h.numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want, what):
    assert len(got) == len(want) == 5
    for j, (a, b) in enumerate(zip(got, want)):
        a, b = _np(a), _np(b)
        assert a.dtype == b.dtype and a.shape == b.shape, (what, j, a.dtype, b.dtype, a.shape, b.shape)
        assert np.array_equal(_bits(a), _bits(b)), "%s: output %d differs at %d of %d" % (what, j, int((a != b).sum()), len(a))


# ---------------------------------------------------------------------------------------------- the kernel alone
def _wide(rng, shape):
    """Magnitudes from 1e-30 to 1e6, either sign."""
    return (rng.choice([-1.0, 1.0], size=shape) * 10.0 ** rng.uniform(-30, 6, size=shape)).astype(np.float32)


def _contract_case():
    """Blocks as (scene, n_rows, [model per segment], kind) over 14 models (model 12 and 13 have status -5), boxes per
    model in BOXES.  The generic blocks run the sizes x the segment counts with random outputs; the named ones build a
    rule each."""
    rng = np.random.default_rng(23)
    boxes = np.array([(7, 9), (3, 8), (5, 9), (5, 11), (11, 5), (0, 1), (2, 13), (12, 4), (6, 10), (1, 2), (9, 3), (8, 0),
                      (4, 6), (13, 7)], np.int32)
    failed = (12, 13)
    spec = []
    i = 0
    for n in (1, 2, 63, 64, 65, 1100):
        for c in (1, 2, 3, 5):
            ms = [int(m) for m in rng.permutation(12)[:c]]
            spec.append((i % 2, n, ms, "random"))
            i += 1
    spec += [(0, 4, [0, 1], "tie_lower_box"),        # 2 : 2 between box 7 and box 3 -> 3, the second tester's b1
             (1, 9, [2, 3], "shared_box"),           # box 5 argued by two fits: 3 + 2 votes against 4 for box 9
             (0, 4, [4, 2], "representative_tie"),   # 2 voters each for box 5: the earliest tester, by its label 1
             (1, 64, [12, 5, 9], "failed_largest"),  # the failed model holds the largest p_new everywhere
             (0, 65, [13], "only_failed"),           # nobody votes
             (1, 66, [5, 6, 7], "all_nan"),          # nobody votes
             (0, 7, [8, 9], "no_positive"),          # p_new <= 0 everywhere: nobody votes
             (1, 130, [5, 6, 7], "nan_rows"),        # every third row NaN in all segments: fewer voters than rows
             (0, 200, [6, 10], "wall_winner"),       # box 13 wins: inst -100
             (1, 33, [0, 1, 2], "inf_mu"),           # a voter of the representative with mu = inf: mu NaN, var finite
             (0, 1100, [0, 1, 2, 3, 4], "to_permute"),
             (1, 1100, [0, 1, 2, 3, 4], "permuted")]
    order = [int(k) for k in rng.permutation(len(spec))]
    spec = [spec[k] for k in order]
    blocks, segs, row = [], [], 0
    for si, n, ms, kind in spec:
        blocks.append([row, n, si, len(segs), len(ms)])
        segs += [[-1, m] for m in ms]
        row += n
    R, R2 = row, 0
    for g in rng.permutation(len(segs)):  # the expanded rows in another order than the segments
        b = next(b for b in blocks if b[3] <= g < b[3] + b[4])
        segs[g][0] = R2
        R2 += b[1]
    pn = np.full(R2, 0.5, np.float32)
    lab = (rng.random(R2) < 0.5).astype(np.uint8)
    mu, var = _wide(rng, R2), np.abs(_wide(rng, R2))
    by_kind = {}
    for (si, n, ms, kind), b in zip(spec, blocks):
        by_kind.setdefault(kind, []).append(b)
        o = [segs[b[3] + s][0] for s in range(len(ms))]
        v = rng.uniform(0.05, 1, size=(len(ms), n)).astype(np.float32)
        lb = None
        if kind == "tie_lower_box":
            v, lb = np.array([[.9, .9, .1, .1], [.2, .2, .8, .8]], np.float32), np.zeros((2, 4), np.uint8)
        elif kind == "shared_box":
            v = np.array([[.9] * 3 + [.1] * 2 + [.9] * 4, [.2] * 3 + [.8] * 2 + [.2] * 4], np.float32)
            lb = np.array([[0] * 5 + [1] * 4, [0] * 9], np.uint8)
        elif kind == "representative_tie":
            v = np.array([[.9, .9, .1, .1], [.2, .2, .8, .8]], np.float32)
            lb = np.array([[1] * 4, [0] * 4], np.uint8)
        elif kind == "failed_largest":
            v[0] = 0.999
        elif kind == "all_nan":
            v[:] = np.nan
        elif kind == "no_positive":
            v[0], v[1] = 0.0, -0.5
        elif kind == "nan_rows":
            v[:, ::3] = np.nan
        elif kind == "wall_winner":
            v[0], v[1] = 0.9, 0.1
            lb = np.zeros((2, n), np.uint8)
            lb[0, : n // 2 + 10] = 1  # model 6 = (2, 13): label 1 -> box 13
        elif kind == "inf_mu":
            v[0], v[1:] = 0.9, 0.1
            lb = np.zeros((3, n), np.uint8)
            mu[o[0] + 5] = np.inf
        for s in range(len(ms)):
            pn[o[s]:o[s] + n] = v[s]
            if lb is not None:
                lab[o[s]:o[s] + n] = lb[s]
    # the permuted twin: the same rows in another order (the gather's order is not part of the contract)
    a, b = by_kind["to_permute"][0], by_kind["permuted"][0]
    perm = rng.permutation(1100)
    for s in range(5):
        oa, ob = segs[a[3] + s][0], segs[b[3] + s][0]
        for arr in (pn, lab, mu, var):
            arr[ob:ob + 1100] = arr[oa:oa + 1100][perm]
    status = np.zeros(len(boxes), np.int32)
    status[list(failed)] = -5
    cls = (np.arange(14) * 3 + 1).astype(np.int32)
    pairs = np.array([[cls[b1], b1 if b1 < N_FG else -100, cls[b2], b2 if b2 < N_FG else -100] for b1, b2 in boxes],
                     np.int32)
    # every block its own superpoint of its scene, in no order; five superpoints per scene belong to no block
    n_spps, block_spp = [], np.zeros(len(blocks), np.int32)
    for si in range(2):
        mine = [k for k, b in enumerate(blocks) if b[2] == si]
        block_spp[mine] = rng.permutation(len(mine) + 5)[:len(mine)]
        n_spps.append(len(mine) + 5)
    return dict(spec=spec, blocks=np.array(blocks, np.int64), segs=np.array(segs, np.int64), R=R, R2=R2, pn=pn, lab=lab,
                mu=mu, var=var, status=status, boxes=boxes, pairs=pairs, block_spp=block_spp, n_spps=n_spps,
                by_kind=by_kind, failed=failed)


def _contract_reference(c, start):
    """vote_ref.vote_block per block -> the five tables of both scenes (from `start`) and block_out."""
    tabs = [[a.copy() for a in sc] for sc in start]
    block_out = np.zeros((len(c["blocks"]), 3), np.int32)
    for k, (r0, n, si, s0, ns) in enumerate(c["blocks"]):
        sg = c["segs"][s0:s0 + ns]
        cut = lambda arr: np.stack([arr[o:o + n] for o, _ in sg])  # noqa: E731
        r = vote_ref.vote_block(int(n), [tuple(c["boxes"][m]) for _, m in sg], [c["status"][m] == 0 for _, m in sg],
                                cut(c["pn"]), cut(c["lab"]), cut(c["mu"]), cut(c["var"]))
        if r is None:
            block_out[k] = -1, -1, 0
            continue
        m = int(sg[r["seg"]][1])
        sp = c["block_spp"][k]
        sem, ins, prob, mu, var = tabs[si]
        sem[sp], ins[sp] = c["pairs"][m][2 if r["second"] else 0], c["pairs"][m][3 if r["second"] else 1]
        prob[sp], mu[sp], var[sp] = r["prob"], r["mu"], r["var"]
        block_out[k] = m, r["box"], r["votes"]
    return tabs, block_out


def test_vote_contract():
    import torch
    from gapro_amd._lib import (Context, PointRefineBlock, PointRefineModel, PointRefineSegment, PointRefineVoteScene)

    ctx = Context.get(0)
    lib = ctx.lib
    dev = torch.device("cuda", 0)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    c = _contract_case()
    R, R2 = c["R"], c["R2"]
    nb, ng, nm = len(c["blocks"]), len(c["segs"]), len(c["status"])
    blocks, segs = (PointRefineBlock * nb)(), (PointRefineSegment * ng)()
    for q, b in zip(blocks, c["blocks"]):
        q.row_start, q.n_rows, q.scene, q.seg_start, q.n_seg = (int(x) for x in b)
    for q, g in zip(segs, c["segs"]):
        q.out_start, q.model, q.reserved = int(g[0]), int(g[1]), 0
    models = (PointRefineModel * nm)()
    for q, pr in zip(models, c["pairs"]):
        q.row_offset, q.t, q.scene = 0, 0, 0
        q.sem1, q.inst1, q.sem2, q.inst2 = (int(x) for x in pr)
    rng = np.random.default_rng(4)
    start = [(rng.integers(-5, 0, S).astype(np.int32), rng.integers(-9, -5, S).astype(np.int32),
              np.full(S, 2, np.float32), rng.normal(size=S).astype(np.float32) - 50, np.full(S, -100, np.float32))
             for S in c["n_spps"]]
    want, want_out = _contract_reference(c, start)

    def dbuf(nbytes):
        return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)

    d_blocks, d_segs, d_models = dbuf(C.sizeof(blocks)), dbuf(C.sizeof(segs)), dbuf(C.sizeof(models))
    d_scenes, d_boxes, d_bspp = dbuf(2 * C.sizeof(PointRefineVoteScene)), dbuf(8 * nm), dbuf(4 * nb)
    boxes, bspp = c["boxes"].copy(), c["block_spp"].copy()
    d_in = [torch.from_numpy(a).to(dev) for a in (c["pn"], c["lab"], c["mu"], c["var"], c["status"])]

    def fresh():
        scenes, t = (PointRefineVoteScene * 2)(), []
        for sc, arrs, S in zip(scenes, start, c["n_spps"]):
            d = [torch.from_numpy(a).to(dev) for a in arrs]
            sc.sem_spp, sc.inst_spp, sc.prob_spp, sc.mu_spp, sc.var_spp = (x.data_ptr() for x in d)
            sc.n_spps = S
            t.append(d)
        return scenes, t

    def vote(scenes, n_blocks, out, r2=R2, n_models=nm, box=boxes, spp=bspp):
        p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
        return lib.gapro_point_refine_vote(
            ctx.handle, stream, 2, C.cast(scenes, C.c_void_p), p(d_scenes), n_models, C.cast(models, C.c_void_p),
            p(d_models), C.c_void_p(box.ctypes.data), p(d_boxes), n_blocks, C.cast(blocks, C.c_void_p), p(d_blocks),
            C.c_void_p(spp.ctypes.data), p(d_bspp), ng, C.cast(segs, C.c_void_p), p(d_segs), R, r2,
            *[x.data_ptr() for x in d_in], out)

    scenes, t = fresh()
    d_out = torch.full((3 * nb + 8,), -7, dtype=torch.int32, device=dev)
    # refused before anything is launched; n_blocks == 0 is a no-op
    assert vote(scenes, nb, d_out.data_ptr(), r2=2 ** 31) == -1
    assert vote(scenes, nb, d_out.data_ptr(), r2=R2 - 1) == -1
    assert vote(scenes, nb, d_out.data_ptr(), n_models=13) == -1  # a segment names model 13
    bad = boxes.copy()
    bad[3, 1] = -1
    assert vote(scenes, nb, d_out.data_ptr(), box=bad) == -1
    bad = bspp.copy()
    bad[5] = c["n_spps"][int(c["blocks"][5][2])]
    assert vote(scenes, nb, d_out.data_ptr(), spp=bad) == -1
    blocks[1].row_start -= 1  # overlaps the block before it
    assert vote(scenes, nb, d_out.data_ptr()) == -1
    blocks[1].row_start += 1
    assert vote(scenes, 0, d_out.data_ptr()) == 0
    torch.cuda.synchronize()
    assert (d_out == -7).all()
    for d, arrs in zip(t, start):
        for a, b in zip(d, arrs):
            assert np.array_equal(a.cpu().numpy(), b)
    ctx.check(vote(scenes, nb, d_out.data_ptr()))
    torch.cuda.synchronize()
    got_out = d_out.cpu().numpy()
    assert (got_out[3 * nb:] == -7).all()
    got_out = got_out[:3 * nb].reshape(nb, 3)
    assert np.array_equal(got_out, want_out)
    for si in range(2):
        for j, (a, b) in enumerate(zip(t[si], want[si])):
            a = a.cpu().numpy()
            assert a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b)), (si, j, int((_bits(a) != _bits(b)).sum()))
    # what the cases are there for, read off the device's result
    idx = {kind: [int(np.nonzero((c["blocks"] == np.array(b)).all(axis=1))[0][0]) for b in bs]
           for kind, bs in c["by_kind"].items()}

    def table(kind, j):
        k = idx[kind][0]
        return t[int(c["blocks"][k][2])][j].cpu().numpy()[c["block_spp"][k]]

    assert got_out[idx["tie_lower_box"][0]].tolist() == [1, 3, 2]       # box 3 < box 7; the second tester argues it
    assert got_out[idx["shared_box"][0]].tolist() == [2, 5, 5]          # 3 + 2 votes; the fit with 3 represents
    assert got_out[idx["representative_tie"][0]].tolist() == [4, 5, 4]  # 2 : 2 voters: the earliest tester
    assert table("representative_tie", 0) == c["pairs"][4][2]           # ... whose voters carry label 1
    assert got_out[idx["failed_largest"][0]][0] in (5, 9)
    for kind in ("only_failed", "all_nan", "no_positive"):
        k = idx[kind][0]
        assert got_out[k].tolist() == [-1, -1, 0]
        si, sp = int(c["blocks"][k][2]), c["block_spp"][k]
        assert [_bits(x.cpu().numpy())[sp] for x in t[si]] == [_bits(a)[sp] for a in start[si]]  # the merge's values stay
    k = idx["nan_rows"][0]
    assert 0 < got_out[k][2] <= 130 - 44  # the 44 NaN rows vote for nobody
    assert got_out[idx["wall_winner"][0]].tolist() == [6, 13, 110] and table("wall_winner", 1) == -100
    assert np.isnan(table("inf_mu", 3)) and np.isfinite(table("inf_mu", 4)) and np.isfinite(table("inf_mu", 2))
    ka, kb = idx["to_permute"][0], idx["permuted"][0]
    assert got_out[ka].tolist() == got_out[kb].tolist() and got_out[ka][2] > 0
    for j in range(5):
        assert _bits(np.array([table("to_permute", j)]))[0] == _bits(np.array([table("permuted", j)]))[0]
    # superpoints of no block keep their values; d_block_out == NULL gives the same tables
    for si in range(2):
        free = np.setdiff1d(np.arange(c["n_spps"][si]), c["block_spp"][c["blocks"][:, 2] == si])
        assert len(free) == 5
        for a, b in zip(t[si], start[si]):
            assert np.array_equal(_bits(a.cpu().numpy())[free], _bits(b)[free])
    scenes2, t2 = fresh()
    ctx.check(vote(scenes2, nb, None))
    torch.cuda.synchronize()
    for si in range(2):
        for a, b in zip(t2[si], t[si]):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---------------------------------------------------------------------------------------------- the whole chain
def _assemble(kw, plain, extra):
    """The "vote" result in NumPy from a return_models=True run of the plain pipeline, as the "compete" test assembles
    its own: refined = winner >= 0; the testers of a superpoint are the fits whose ``test`` lists it, in ``fits`` order;
    every tester is evaluated at the mask_feats rows of the points of the refined superpoints it tested
    (predict_gp_batch); then vote_ref.vote_block per refined superpoint and the box -> (sem, inst) rule."""
    from gapro_amd.gaussian_process_utils import predict_gp_batch

    sem, ins, prob, mu_s, var_s = (_np(x).copy() for x in plain)
    ranks = np.unique(np.asarray(kw["spp"]), return_inverse=True)[1].reshape(-1)
    winner = extra.winner.copy()
    S = len(winner)
    vote_box, vote_count = np.full(S, -1, np.int32), np.zeros(S, np.int32)
    feats = np.ascontiguousarray(np.asarray(kw["mask_feats"], dtype=np.float32))
    n_inst = len(kw["instance_box"])
    boxes_cls = np.concatenate([np.asarray(kw["instance_cls"], dtype=np.int64),
                                np.full(len(kw["wall_box"]) + 1, 18, dtype=np.int64)])
    refined_sp = extra.winner >= 0
    use = [k for k, f in enumerate(extra.fits) if refined_sp[np.asarray(f.test)].any()]
    moved = 0
    if use:
        pts = [np.nonzero(np.isin(ranks, np.asarray(extra.fits[k].test)[refined_sp[np.asarray(extra.fits[k].test)]]))[0]
               for k in use]
        got = dict(zip(use, zip(pts, predict_gp_batch([extra.fits[k].model for k in use], feats, pts))))
        for s in np.nonzero(refined_sp)[0]:
            mine = np.nonzero(ranks == s)[0]
            testers = [k for k in use if s in np.asarray(extra.fits[k].test)]  # ascending: the merge's order
            rows = {k: np.searchsorted(got[k][0], mine) for k in testers}  # pts are ascending
            cut = lambda j: np.stack([got[k][1][j][rows[k]] for k in testers])  # noqa: E731
            r = vote_ref.vote_block(len(mine), [(extra.fits[k].b1, extra.fits[k].b2) for k in testers],
                                    [True] * len(testers), cut(1), cut(2), cut(3), cut(4))
            if r is None:
                continue
            box = r["box"]
            moved += int(ins[mine[0]] != (box if box < n_inst else -100))
            sem[mine], ins[mine] = np.int32(boxes_cls[box]), np.int32(box if box < n_inst else -100)
            prob[mine], mu_s[s], var_s[s] = r["prob"], r["mu"], r["var"]
            winner[s], vote_box[s], vote_count[s] = testers[r["seg"]], box, r["votes"]
    return (sem, ins, prob, mu_s, var_s), refined_sp[ranks], winner, vote_box, vote_count, moved


def _flip_scene():
    """The smallest scene in which the vote moves a superpoint (none of the three goldens has one): boxes 0 and 1 overlap
    in x; six superpoints lie in box 0 alone (first feature about -1), six in box 1 alone (about +1), one on the floor,
    and ONE in both boxes: 12 of its points on box 0's side (-0.5), 8 far on box 1's side (+2).  Its pooled feature,
    +0.5, is on box 1's side and the merge gives it to box 1; 12 of its 20 points vote for box 0.  (The float64 oracle's
    fit says the same with p_new about 0.85 against 0.65: no close call.)"""
    rng = np.random.default_rng(0)
    pts, feats, spp = [], [], []

    def add(n, xlo, xhi, f, sid, z=(0.3, 0.9)):
        pts.append(np.c_[rng.uniform(xlo, xhi, n), rng.uniform(0.1, 0.9, n), rng.uniform(*z, n)])
        ft = np.zeros((n, 6), np.float32)
        ft[:, 0] = f
        ft[:, 1:] = rng.normal(0, 0.05, (n, 5))
        feats.append(ft)
        spp.extend([sid] * n)

    for k in range(6):
        add(10, 0.2, 1.3, -1.0 + 0.05 * k, k)
    for k in range(6):
        add(10, 2.2, 3.3, 1.0 + 0.05 * k, 6 + k)
    add(12, 1.55, 1.95, -0.5, 12)
    add(8, 1.55, 1.95, 2.0, 12)
    add(10, 4.0, 5.0, 0.0, 13, z=(0.0, 0.0))
    box = np.array([[0, 0, 0.2, 2, 1, 1], [1.5, 0, 0.2, 3.5, 1, 1]], np.float32)
    return dict(coords_float=np.concatenate(pts), mask_feats=np.concatenate(feats), spp=np.array(spp, np.int64) * 3 + 11,
                instance_cls=np.array([3, 5], np.int64), instance_box=box,
                instance_box_volume=np.prod(box[:, 3:] - box[:, :3], axis=1).astype(np.float32), wall_box=[],
                wall_box_volume=[], instance_classes=18, dataset_name="scannetv2", ground_h=0.1, training_iter=50,
                thresh_spp_occu=0.999)


@pytest.fixture(scope="module")
def runs():
    from conftest import Golden
    from gapro_amd import gen_pseudo_label_gaussian_process

    out = {}
    for name in NAMES + ("flip",):
        kw = Golden(name).api_inputs() if name != "flip" else _flip_scene()
        full = gen_pseudo_label_gaussian_process(**kw, device="cuda:0", return_models=True)
        vote = gen_pseudo_label_gaussian_process(**kw, device="cuda:0", point_level="vote", return_models=True)
        want, refined, winner, vote_box, vote_count, moved = _assemble(kw, full[:5], full[5])
        out[name] = dict(kw=kw, full=full, vote=tuple(_np(x) for x in vote[:5]), models=vote[5], want=want,
                         refined=refined, winner=winner, vote_box=vote_box, vote_count=vote_count, moved=moved)
    return out


def test_vote_equals_the_assembly_from_the_kept_models(runs):
    from gapro_amd import gen_pseudo_label_gaussian_process

    moved = 0
    for name, r in runs.items():
        plain = tuple(_np(x) for x in r["full"][:5])
        assert [x.dtype for x in r["vote"]] == [x.dtype for x in plain]
        assert [x.shape for x in r["vote"]] == [x.shape for x in plain]  # the default path's lengths
        _same(r["vote"], r["want"], name)
        m = r["models"]
        for got, want in ((m.winner, r["winner"]), (m.vote_box, r["vote_box"]), (m.vote_count, r["vote_count"])):
            assert got.dtype == np.int32 and np.array_equal(got, want), name
        assert m.point_fit is None and r["full"][5].vote_box is None
        # nothing outside a refined superpoint moves
        out = ~r["refined"]
        for j in range(3):
            assert np.array_equal(_bits(r["vote"][j][out]), _bits(plain[j][out])), (name, j)
        out_sp = r["full"][5].winner < 0
        for j in (3, 4):
            assert np.array_equal(_bits(r["vote"][j][out_sp]), _bits(plain[j][out_sp])), (name, j)
        assert (m.vote_count[out_sp] == 0).all() and (m.vote_box[out_sp] == -1).all()
        print("%s: %d refined superpoints, %d voted, %d end in another box than the merge's"
              % (name, int((~out_sp).sum()), int((m.vote_count > 0).sum()), r["moved"]))
        moved += r["moved"]
    # On the three goldens no superpoint moves (0 of 13, 44 and 0 voted ones, measured on the MI355X); the synthetic
    # scene is there so that the mode is distinguishable from the default: its superpoint 12 goes from box 1 to box 0
    assert moved >= 1 and runs["flip"]["moved"] == 1
    r = runs["flip"]
    mine = np.nonzero(np.asarray(r["kw"]["spp"]) == 3 * 12 + 11)[0]
    assert (_np(r["full"][1])[mine] == 1).all() and (r["vote"][1][mine] == 0).all()
    assert (_np(r["full"][0])[mine] == 5).all() and (r["vote"][0][mine] == 3).all()
    assert r["models"].vote_box[12] == 0 and r["models"].vote_count[12] == 12 and r["models"].winner[12] == 0
    assert 0.3 < r["vote"][2][mine[0]] < 0.6  # mean confidence (about 0.85) x vote share 12 / 20
    # broadcast_mu_var applies as on the default path
    kw = runs["s2_dense"]["kw"]
    b = gen_pseudo_label_gaussian_process(**kw, device="cuda:0", point_level="vote", broadcast_mu_var=True)
    ranks = np.unique(np.asarray(kw["spp"]), return_inverse=True)[1].reshape(-1)
    want = runs["s2_dense"]["want"]
    _same(b, want[:3] + (want[3][ranks], want[4][ranks]), "broadcast_mu_var")


@pytest.mark.parametrize("backend", ["torch", "native"])
def test_a_batch_does_not_change_a_scene(runs, backend):
    from gapro_amd.gen_ps_utils import gen_pseudo_label_gaussian_process_batch
    from gapro_amd.pipeline import Pipeline, make_job

    names = ["s3_bigspp", "s2_dense", "s0_walls"]
    if backend == "torch":
        outs = gen_pseudo_label_gaussian_process_batch([runs[n]["kw"] for n in names], device="cuda:0", point_level="vote")
    else:
        pipe = Pipeline(device=0, training_iter=50, backend="native", point_level="vote")
        assert pipe.point_level is True and pipe.point_mode == "vote" and pipe.point_outputs is False
        outs = pipe.run([make_job(*[runs[n]["kw"][k] for k in ARGS], **OPTS, backend=pipe.be) for n in names])
        assert pipe.last_refine["rows"] == sum(int(runs[n]["refined"].sum()) for n in names)
    for n, o in zip(names, outs):
        _same(o, runs[n]["want"], "%s in a batch of three (%s)" % (n, backend))


def test_cli_point_vote_in_a_fresh_process(tmp_path):
    """`gen_ps --point_vote --devices 0` over a small synthetic dataset in a child process: exit status 0, torch never
    imported, and every label file holds the arrays of Pipeline(point_level="vote"), at the default lengths."""
    import torch
    from gapro_amd.gen_ps import load_scene
    from gapro_amd.pipeline import Pipeline, make_job
    from gapro_amd.synth import make_scene, write_scannet_layout

    root, scenes = str(tmp_path / "dataset" / "scannetv2"), []
    for i in range(2):
        sc = make_scene(seed=30 + i, n_points=4000, n_objects=8, with_walls_json=(i == 0), obj_patch=25, plane_patch=80,
                        scan_name="scene%04d_00" % (700 + i))
        write_scannet_layout(sc, root)
        scenes.append(sc)
    save = str(tmp_path / "labels")
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from gapro_amd import gen_ps\n"
            "rc = gen_ps.main(['--save_folder', sys.argv[1], '--data_root', %r, '--point_vote', '--devices', '0'])\n"
            "print('TORCH_IMPORTED', 'torch' in sys.modules)\n"
            "sys.exit(rc)\n" % (ROOT, root))
    env = {k: v for k, v in os.environ.items() if k != "GAPRO_BACKEND"}
    r = subprocess.run([sys.executable, "-c", code, save], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "2 scenes written, 0 skipped/failed" in r.stdout
    assert "TORCH_IMPORTED False" in r.stdout and "the library's own arena" in r.stdout, r.stdout
    pipe = Pipeline(device=0, training_iter=50, point_level="vote")
    jobs = []
    for s in scenes:
        sc = load_scene(os.path.join(root, "train", s.scan_name + "_inst_nostuff.pth"), root)
        jobs.append(make_job(*[sc[k] for k in ARGS], **OPTS, device="cuda:0"))
    outs = pipe.run(jobs)
    assert pipe.last_refine["rows"] > 0
    for s, o, job in zip(scenes, outs, jobs):
        tup = torch.load(os.path.join(save, s.scan_name + ".pth"), weights_only=False)
        assert len(tup) == 5 and [len(a) for a in tup] == [s.n_points] * 3 + [job.n_spps] * 2
        _same(o, tup, s.scan_name)
