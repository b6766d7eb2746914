"""The point-level refine kernels (csrc/point_refine.hip) at their grid and table edges on the MI355X: the cases of
tests/point_refine_cases.py through the five entry points, called directly, against the NumPy references of that module.

Every comparison is bit for bit: the gather, apply, expand and compete kernels copy and select, and the vote's one
rounding is restated exactly by tests/vote_ref.py.  Every output buffer starts from a sentinel and has eight spare
elements behind it that must keep it.  tests/test_point_refine_edges_cpu.py shows that each case is what it claims and that
a kernel which forgot to wrap its grid could not produce the reference."""
import ctypes as C

import numpy as np
import pytest

import point_refine_cases as pc

pytestmark = pytest.mark.gpu

SENT, SENT_F, SPARE = pc.SENT, pc.SENT_F, pc.SPARE


class Gpu:
    def __init__(self):
        import torch
        from gapro_amd._lib import Context

        self.torch = torch
        self.ctx = Context.get(0)
        self.lib = self.ctx.lib
        self.dev = torch.device("cuda", 0)
        self.stream = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def up(self, a):
        """a host array on the device (an input: no spare)"""
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def out(self, a, fill):
        """an in/out array on the device with SPARE elements of `fill` behind it"""
        a = np.ascontiguousarray(a)
        return self.up(np.concatenate([a, np.full((SPARE,) + a.shape[1:], fill, a.dtype)]))

    def raw(self, nbytes):
        return self.torch.empty(max(int(nbytes), 1), dtype=self.torch.uint8, device=self.dev)

    def sync(self):
        self.torch.cuda.synchronize()

    def error(self):
        return (self.lib.gapro_last_error(self.ctx.handle) or b"").decode()


@pytest.fixture(scope="module")
def gpu():
    return Gpu()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _host(a):
    return C.c_void_p(a.ctypes.data)


def _fill_of(dtype):
    return SENT_F if dtype == np.float32 else SENT


def _tables_equal(got, want, what):
    """device arrays (n + SPARE each) against the reference's, bit for bit, and the spare elements untouched"""
    assert len(got) == len(want)
    for j, (t, b) in enumerate(zip(got, want)):
        a = t.cpu().numpy()
        assert a.dtype == b.dtype and len(a) == len(b) + SPARE, (what, j)
        assert (a[len(b):] == _fill_of(b.dtype)).all(), "%s: array %d written behind its end" % (what, j)
        x, y = pc.bits(a[:len(b)]), pc.bits(b)
        assert np.array_equal(x, y), "%s: array %d differs at %d of %d" % (what, j, int((x != y).sum()), len(b))


# ---------------------------------------------------------------------------------------------- gather
def _run_gather(gpu, case):
    from gapro_amd._lib import PointRefineScene

    ns, d, R = len(case["scenes"]), case["d"], case["R"]
    scenes = (PointRefineScene * ns)()
    keep = []
    for q, sc in zip(scenes, case["scenes"]):
        t = [gpu.up(sc["inv"]), gpu.up(sc["feats"]), gpu.up(sc["sp_row"]), gpu.out(np.full(sc["S"], 99, np.int32), 99)]
        keep.append(t)
        q.n_points, q.n_spps = sc["n"], sc["S"]
        q.spp_inv, q.feats, q.sp_row, q.cursor = (x.data_ptr() for x in t)
    d_scenes = gpu.raw(C.sizeof(scenes))
    row_feats = gpu.out(np.full((R, d), SENT_F, np.float32), SENT_F)
    row_point = gpu.out(np.full(R, SENT, np.int32), SENT)
    gpu.ctx.check(gpu.lib.gapro_point_refine_gather(gpu.ctx.handle, gpu.stream, ns, d, C.cast(scenes, C.c_void_p),
                                                   _p(d_scenes), case["n_rows"], _p(row_feats), _p(row_point)))
    gpu.sync()
    cursors = []
    for t, sc in zip(keep, case["scenes"]):
        cur = t[3].cpu().numpy()
        assert (cur[sc["S"]:] == 99).all()
        cursors.append(cur[:sc["S"]])
    return row_point.cpu().numpy(), row_feats.cpu().numpy(), cursors


@pytest.mark.parametrize("d", pc.GATHER_WIDTHS)
def test_gather_at_every_feature_width(gpu, d):
    case = pc.gather_width_case(d)
    assert pc.check_gather(case, *_run_gather(gpu, case)) == case["R"]


@pytest.mark.parametrize("n", pc.GATHER_LENGTHS)
def test_gather_of_a_scene_around_one_workgroup(gpu, n):
    case = pc.gather_length_case(n)
    assert pc.check_gather(case, *_run_gather(gpu, case)) == case["R"]


def test_gather_wraps_the_2048_workgroup_grid_and_survives_one_cursor(gpu):
    case = pc.gather_big_case()
    rp, rf, cur = _run_gather(gpu, case)
    assert pc.check_gather(case, rp, rf, cur) == case["R"]
    sc = case["scenes"][0]
    assert rp[sc["sp_row"][198]] == 0 and sc["n"] - 1 in rp[sc["sp_row"][199]:sc["sp_row"][199] + 5]
    assert cur[0][7] == pc.BIG_SPP


def test_gather_of_eight_scenes_takes_the_256_workgroup_grid(gpu):
    case = pc.gather_many_case()
    rp, rf, cur = _run_gather(gpu, case)
    assert pc.check_gather(case, rp, rf, cur) == case["R"]
    assert not cur[0].any() and not cur[5].any()  # the scenes that refine nothing: cleared, never advanced


def test_gather_with_a_plan_one_row_short_drops_one_point(gpu):
    case = pc.gather_short_case()
    rp, rf, cur = _run_gather(gpu, case)
    R = case["R"]
    assert pc.check_gather(case, rp, rf, cur) == R - 1  # every block but the last is complete, the last lacks one point
    assert rp[R - 1] == SENT and (rf[R - 1] == SENT_F).all() and rp[R - 2] != SENT
    last = case["scenes"][-1]
    sp = int(np.argmax(last["sp_row"]))
    got = rp[last["sp_row"][sp]:R - 1]
    assert len(set(got.tolist())) == last["count"][sp] - 1 and (last["inv"][got] == sp).all()


def test_gather_skips_ids_outside_the_superpoints(gpu):
    case = pc.gather_guard_case()
    rp, rf, cur = _run_gather(gpu, case)
    assert pc.check_gather(case, rp, rf, cur) == case["R"]
    sc = case["scenes"][0]
    outside = np.nonzero((sc["inv"] < 0) | (sc["inv"] >= sc["S"]))[0]
    assert len(outside) == 8 and not np.isin(rp, outside).any()


# ---------------------------------------------------------------------------------------------- apply
def _run_apply(gpu, c, use_status=True, null_rows=False):
    """One gapro_point_refine_apply; returns per scene the five device arrays (n + SPARE each)."""
    from gapro_amd._lib import PointRefineScene

    ns, nm = c["n_scenes"], len(c["t"])
    scenes = (PointRefineScene * ns)()
    keep, outs = [], []
    for si, q in enumerate(scenes):
        n = c["n_pts"][si]
        ins = [gpu.up(c["inv"][si]), gpu.up(c["mu_spp"][si]), gpu.up(c["var_spp"][si])]
        five = [gpu.out(a, _fill_of(a.dtype)) for a in c["start"][si]] + [gpu.out(np.full(n, SENT_F, np.float32), SENT_F)
                                                                         for _ in range(2)]
        keep.append(ins)
        outs.append(five)
        q.n_points, q.n_spps = n, c["spps"][si]
        q.spp_inv, q.mu_spp, q.var_spp = (x.data_ptr() for x in ins)
        q.sem, q.inst, q.prob, q.mu, q.var = (x.data_ptr() for x in five)
    d_scenes = gpu.raw(C.sizeof(scenes))
    models = pc.model_table(c["pairs"], c["scene_of"], c["off"], c["t"])
    d_models = gpu.raw(models.nbytes)
    if null_rows:
        rows = [None] * 5
    else:
        rows = [gpu.up(a if len(a) else np.zeros(4, a.dtype))
                for a in (c["row_point"], c["pn"], c["lab"], c["mu"], c["var"])]
    status = gpu.up(c["status"]) if use_status and nm else None
    gpu.ctx.check(gpu.lib.gapro_point_refine_apply(
        gpu.ctx.handle, gpu.stream, ns, C.cast(scenes, C.c_void_p), _p(d_scenes), nm, _host(models) if nm else None,
        _p(d_models) if nm else None, c["n_rows"], *[_p(x) for x in rows], _p(status)))
    gpu.sync()
    return outs


def _apply_equal(outs, want, what):
    for si, (got, ref) in enumerate(zip(outs, want)):
        _tables_equal(got, ref, "%s scene %d" % (what, si))


def test_apply_of_70_models_takes_the_64_workgroup_grid(gpu):
    c = pc.apply_many_case()
    _apply_equal(_run_apply(gpu, c), pc.apply_reference(c), "with status")
    _apply_equal(_run_apply(gpu, c, use_status=False), pc.apply_reference(c, use_status=False), "status NULL")


def test_apply_of_5_models_wraps_the_1024_workgroup_grid(gpu):
    c = pc.apply_few_case()
    _apply_equal(_run_apply(gpu, c), pc.apply_reference(c), "few")


def test_apply_of_more_models_than_one_grid_y(gpu):
    c = pc.apply_grid_y_case()
    _apply_equal(_run_apply(gpu, c), pc.apply_reference(c), "grid.y")


def test_apply_without_rows_only_broadcasts_mu_and_var(gpu):
    c = pc.apply_no_rows_case()
    want = pc.apply_reference(c)
    for si in range(c["n_scenes"]):  # what the reference says here: the start values and the superpoints' mu / var
        assert all(np.array_equal(a, b) for a, b in zip(want[si][:3], c["start"][si]))
        assert np.array_equal(want[si][3], c["mu_spp"][si][c["inv"][si]])
    _apply_equal(_run_apply(gpu, c), want, "t == 0 everywhere")
    none = dict(c, t=c["t"][:0], off=c["off"][:0], scene_of=c["scene_of"][:0], pairs=c["pairs"][:0], status=c["status"][:0])
    _apply_equal(_run_apply(gpu, none, null_rows=True), want, "n_models == 0, NULL rows")


@pytest.mark.parametrize("many", [False, True])
def test_the_mu_var_pass_alone_wraps_both_grids(gpu, many):
    c = pc.mu_var_case(many)
    _apply_equal(_run_apply(gpu, c, null_rows=True), pc.apply_reference(c), "mu / var")


# ---------------------------------------------------------------------------------------------- expand and compete
class _Blocks:
    """The tables of a block case on the host and their device copies' buffers."""

    def __init__(self, gpu, c):
        self.blocks, self.segs = pc.block_table(c["blocks"]), pc.segment_table(c["segs"])
        self.nb, self.ng = len(self.blocks), len(self.segs)
        self.d_blocks, self.d_segs = gpu.raw(self.blocks.nbytes), gpu.raw(self.segs.nbytes)

    def args(self):
        return (self.nb, _host(self.blocks), _p(self.d_blocks), self.ng, _host(self.segs) if self.ng else None,
                _p(self.d_segs) if self.ng else None)


def _run_expand(gpu, c):
    t = _Blocks(gpu, c)
    d_rows = gpu.out(np.full(c["R2"], SENT, np.int32), SENT)
    gpu.ctx.check(gpu.lib.gapro_point_refine_expand(gpu.ctx.handle, gpu.stream, *t.args(), c["R"], c["R2"], _p(d_rows)))
    gpu.sync()
    return d_rows


def _run_compete(gpu, c, start, use_status=True, want_model=True):
    from gapro_amd._lib import PointRefineScene

    t = _Blocks(gpu, c)
    ns, nm = len(c["n_pts"]), len(c["status"])
    scenes = (PointRefineScene * ns)()
    outs = []
    for q, arrs, n in zip(scenes, start, c["n_pts"]):
        five = [gpu.out(a, _fill_of(a.dtype)) for a in arrs]
        q.n_points, q.n_spps = n, 1
        q.sem, q.inst, q.prob, q.mu, q.var = (x.data_ptr() for x in five)
        outs.append(five)
    d_scenes = gpu.raw(C.sizeof(scenes))
    models = pc.model_table(c["pairs"], c["model_scene"])
    d_models = gpu.raw(models.nbytes)
    rows = [gpu.up(a) for a in (c["row_point"], c["pn"], c["lab"], c["mu"], c["var"])]
    status = gpu.up(c["status"]) if use_status else None
    row_model = gpu.out(np.full(c["R"], SENT, np.int32), SENT) if want_model else None
    gpu.ctx.check(gpu.lib.gapro_point_refine_compete(
        gpu.ctx.handle, gpu.stream, ns, C.cast(scenes, C.c_void_p), _p(d_scenes), nm, _host(models), _p(d_models),
        *t.args(), c["R"], c["R2"], *[_p(x) for x in rows], _p(status), _p(row_model)))
    gpu.sync()
    return outs, row_model


@pytest.mark.parametrize("which", ["edge", "single"])
def test_expand_and_compete_with_gaps_around_the_blocks(gpu, which):
    c = pc.compete_edge_case() if which == "edge" else pc.compete_single_case()
    start = pc.compete_start(c)
    want_rows, want, want_model = pc.contract_reference(c, start)
    of = pc.block_of_rows(c["blocks"], c["R"])
    assert (want_model[of < 0] == -1).all() and (of < 0).sum() >= (5 + 40 if which == "edge" else 500)
    _tables_equal([_run_expand(gpu, c)], [want_rows], "expand")
    assert (want_rows == SENT).sum() == pc.EDGE_HOLE * len(c["segs"])  # the holes keep the sentinel
    outs, row_model = _run_compete(gpu, c, start)
    _tables_equal([row_model], [want_model], "row_model")
    for si in range(len(c["n_pts"])):
        _tables_equal(outs[si], want[si], "compete scene %d" % si)
    got = row_model.cpu().numpy()[:c["R"]]
    assert (got[of < 0] == -1).all() and (got[(of >= 0) & (c["blocks"][np.maximum(of, 0), 4] == 0)] == -1).all()
    # d_row_model == NULL: the same five arrays; d_model_status == NULL: those of a case in which nobody failed
    outs2, _ = _run_compete(gpu, c, start, want_model=False)
    for si in range(len(c["n_pts"])):
        _tables_equal(outs2[si], want[si], "row_model NULL, scene %d" % si)
    live = dict(c, status=np.zeros_like(c["status"]))
    _, want_live, want_live_model = pc.contract_reference(live, start)
    assert not np.array_equal(want_live_model, want_model)
    outs3, row_model3 = _run_compete(gpu, c, start, use_status=False)
    _tables_equal([row_model3], [want_live_model], "status NULL: row_model")
    for si in range(len(c["n_pts"])):
        _tables_equal(outs3[si], want_live[si], "status NULL, scene %d" % si)


# ---------------------------------------------------------------------------------------------- vote
def _run_vote(gpu, c, start, both=True, blocks=None, boxes=None):
    """One gapro_point_refine_vote (both: with d_model_status and d_block_out, otherwise both NULL); returns the return
    code, the five tables per scene and block_out."""
    from gapro_amd._lib import PointRefineVoteScene

    t = _Blocks(gpu, c if blocks is None else dict(c, blocks=blocks))
    ns, nm = len(c["n_spps"]), len(c["status"])
    scenes = (PointRefineVoteScene * ns)()
    tabs = []
    for q, arrs, s in zip(scenes, start, c["n_spps"]):
        five = [gpu.out(a, _fill_of(a.dtype)) for a in arrs]
        q.sem_spp, q.inst_spp, q.prob_spp, q.mu_spp, q.var_spp = (x.data_ptr() for x in five)
        q.n_spps = s
        tabs.append(five)
    d_scenes = gpu.raw(C.sizeof(scenes))
    models = pc.model_table(c["pairs"], 0)
    boxes = np.ascontiguousarray(c["boxes"] if boxes is None else boxes, np.int32)
    bspp = np.ascontiguousarray(c["block_spp"], np.int32)
    d_models, d_boxes, d_bspp = gpu.raw(models.nbytes), gpu.raw(boxes.nbytes), gpu.raw(bspp.nbytes)
    rows = [gpu.up(a) for a in (c["pn"], c["lab"], c["mu"], c["var"])]
    status = gpu.up(c["status"]) if both else None
    block_out = gpu.out(np.full(3 * t.nb, SENT, np.int32), SENT) if both else None
    nb, hb, db, ng, hg, dg = t.args()
    rc = gpu.lib.gapro_point_refine_vote(
        gpu.ctx.handle, gpu.stream, ns, C.cast(scenes, C.c_void_p), _p(d_scenes), nm, _host(models), _p(d_models),
        _host(boxes), _p(d_boxes), nb, hb, db, _host(bspp), _p(d_bspp), ng, hg, dg, c["R"], c["R2"],
        *[_p(x) for x in rows], _p(status), _p(block_out))
    gpu.sync()
    return rc, tabs, block_out


def _vote_equal(tabs, block_out, want, want_out, what):
    for si, (got, ref) in enumerate(zip(tabs, want)):
        _tables_equal(got, ref, "%s scene %d" % (what, si))
    if block_out is not None:
        _tables_equal([block_out], [want_out.reshape(-1)], what + " block_out")


def test_vote_across_the_256_candidate_edge(gpu):
    c = pc.vote_edge_case()
    start = pc.vote_start(c)
    want, want_out = pc.vote_reference(c, start)
    assert [int(x) for x in want_out[[4, 5], 1]] == [20, 20]  # a loop that stopped at candidate 255 says 23 (CPU file)
    rc, tabs, block_out = _run_vote(gpu, c, start)
    gpu.ctx.check(rc)
    _vote_equal(tabs, block_out, want, want_out, "vote")
    # both optional arguments NULL: the same five tables (no model of the case has a status)
    rc, tabs2, _ = _run_vote(gpu, c, start, both=False)
    gpu.ctx.check(rc)
    _vote_equal(tabs2, None, want, want_out, "status and block_out NULL")


def test_vote_refuses_one_segment_too_many_and_equal_boxes(gpu):
    c = pc.vote_edge_case()
    start = pc.vote_start(c)
    untouched = [[a.copy() for a in sc] for sc in start]
    blocks = c["blocks"].copy()
    blocks[0, 3], blocks[0, 4] = 0, pc.VOTE_MAX_SEG + 1
    rc, tabs, block_out = _run_vote(gpu, c, start, blocks=blocks)
    assert rc == -1 and "%d segments" % (pc.VOTE_MAX_SEG + 1) in gpu.error()
    _vote_equal(tabs, block_out, untouched, np.full(3 * len(blocks), SENT, np.int32), "2049 segments")
    # a model whose two boxes are equal is refused before anything is launched, and the message names it
    boxes = c["boxes"].copy()
    boxes[17, 1] = boxes[17, 0]
    rc, tabs, block_out = _run_vote(gpu, c, start, boxes=boxes)
    assert rc == -1 and "model 17" in gpu.error() and "boxes %d, %d" % (boxes[17, 0], boxes[17, 0]) in gpu.error()
    _vote_equal(tabs, block_out, untouched, np.full(3 * len(blocks), SENT, np.int32), "equal boxes")


def test_vote_of_more_blocks_than_the_grid_holds(gpu):
    c = pc.vote_grid_case()
    start = pc.vote_start(c)
    want, want_out = pc.vote_grid_reference(c, start)
    assert len(c["blocks"]) == pc.VOTE_GRID + 3 and (want_out[-3:, 0] == 36).all()
    rc, tabs, block_out = _run_vote(gpu, c, start)
    gpu.ctx.check(rc)
    _vote_equal(tabs, block_out, want, want_out, "2^18 + 3 blocks")


def test_vote_of_one_block_of_70000_rows(gpu):
    c = pc.vote_big_case()
    start = pc.vote_start(c)
    want, want_out = pc.vote_reference(c, start)
    assert want_out[0, 2] > 10000 and np.isfinite(want[0][3][c["block_spp"][0]])
    rc, tabs, block_out = _run_vote(gpu, c, start)
    gpu.ctx.check(rc)
    _vote_equal(tabs, block_out, want, want_out, "70 000 rows")
