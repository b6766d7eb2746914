"""point_level="compete" on the MI355X: the per-point replay of the fit competition (gapro_point_refine_expand /
gapro_point_refine_compete, Pipeline(point_level="compete")).

Every comparison is bit for bit.  The two kernels do no floating-point arithmetic (they compare and copy), and the chain
and the NumPy assembly run the same predict kernel on the same states and the same feature rows (a predict row's result
does not depend on what shares its launch): every difference is a defect and no tolerance applies.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from point_refine_cases import contract_reference as _contract_reference

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ("coords_float", "mask_feats", "spp", "instance_cls", "instance_box", "instance_box_volume", "wall_box",
        "wall_box_volume")
OPTS = dict(instance_classes=18, ground_h=0.1, thresh_spp_occu=0.999)
NO_MULTI = ("s0_walls", "s1_nowalls", "s3_bigspp", "s4_dups")  # goldens without a superpoint tested by two fits


def _np(t):
    if isinstance(t, np.ndarray):
        return t
    h = t.cpu()
    return h if isinstance(h, np.ndarray) else h.numpy()


def _same(got, want, what):
    assert len(got) == len(want) == 5
    for j, (a, b) in enumerate(zip(got, want)):
        a, b = _np(a), _np(b)
        assert a.dtype == b.dtype and a.shape == b.shape, (what, j, a.dtype, b.dtype, a.shape, b.shape)
        assert np.array_equal(a, b), "%s: output %d differs at %d of %d points" % (what, j, int((a != b).sum()), len(a))


# ---------------------------------------------------------------------------------------------- the kernels alone
def _contract_case():
    """Two scenes, hand-made predict outputs.  Block sizes 1, 2, 63, 64, 65, 257, 1025 x segment counts 1, 2, 3, 8, the
    p_new patterns cycling over the blocks; models 16 (scene 0) and 17 (scene 1) have status -5."""
    rng = np.random.default_rng(11)
    sizes, counts = (1, 2, 63, 64, 65, 257, 1025), (1, 2, 3, 8)
    kinds = ("tie", "ulp", "decreasing", "random", "nan_first", "tie_then_ulp")
    spec = []  # (scene, n_rows, [model per segment], kind)
    i = 0
    for n in sizes:
        for c in counts:
            si = i % 2
            spec.append((si, n, [8 * si + k for k in range(c)], kinds[i % len(kinds)]))
            i += 1
    # the failed model: the only tester (its points keep what they hold); first, in the middle and last among others,
    # each time with the largest p_new, which must not count; and every value NaN (no segment can be taken)
    spec += [(0, 65, [16], "random"), (1, 5, [17], "tie"), (0, 64, [16, 2, 5], "failed_largest"),
             (1, 257, [9, 17, 12], "failed_largest"), (0, 3, [1, 4, 16], "failed_largest"), (1, 66, [8, 9, 10], "all_nan")]
    order = rng.permutation(len(spec))
    spec = [spec[k] for k in order]
    n_models, failed = 18, (16, 17)
    blocks, segs = [], []
    row = 0
    for si, n, ms, kind in spec:
        blocks.append([row, n, si, len(segs), len(ms)])
        segs += [[-1, m] for m in ms]
        row += n
    R = row
    # the row list in another order than the segments: a random permutation of the segments
    R2 = 0
    for g in rng.permutation(len(segs)):
        b = next(b for b in blocks if b[3] <= g < b[3] + b[4])
        segs[g][0] = R2
        R2 += b[1]
    pn = np.full(R2, 0.123, np.float32)
    for (si, n, ms, kind), b in zip(spec, blocks):
        v = np.zeros((len(ms), n), np.float32)
        if kind == "tie":
            v[:] = rng.uniform(0.5, 1, size=n).astype(np.float32)
        elif kind == "ulp":  # every later segment one float32 step above the one before: the last wins
            v[0] = rng.uniform(0.5, 0.9, size=n).astype(np.float32)
            for s in range(1, len(ms)):
                v[s] = np.nextafter(v[s - 1], np.float32(2))
        elif kind == "decreasing":
            v[0] = rng.uniform(0.9, 1, size=n).astype(np.float32)
            for s in range(1, len(ms)):
                v[s] = np.nextafter(v[s - 1], np.float32(0)) if s % 2 else v[s - 1] - np.float32(0.01)
        elif kind == "random":
            v[:] = rng.uniform(0.5, 1, size=v.shape).astype(np.float32)
        elif kind == "nan_first":
            v[:] = rng.uniform(0.5, 1, size=v.shape).astype(np.float32)
            v[0] = np.nan
            v[-1, ::3] = np.nan
        elif kind == "tie_then_ulp":  # equal values, then one step up at the last segment on every other row
            v[:] = rng.uniform(0.5, 0.9, size=n).astype(np.float32)
            v[-1, ::2] = np.nextafter(v[-1, ::2], np.float32(2))
        elif kind == "failed_largest":
            v[:] = rng.uniform(0.5, 0.9, size=v.shape).astype(np.float32)
            for s, m in enumerate(ms):
                if m in failed:
                    v[s] = 0.99
        elif kind == "all_nan":
            v[:] = np.nan
        for s in range(len(ms)):
            o = segs[b[3] + s][0]
            pn[o:o + n] = v[s]
    lab = (rng.random(R2) < 0.5).astype(np.uint8)
    mu = rng.normal(size=R2).astype(np.float32)
    var = rng.uniform(0.1, 2, size=R2).astype(np.float32)
    status = np.zeros(n_models, np.int32)
    status[list(failed)] = -5
    pairs = rng.integers(0, 40, size=(n_models, 4)).astype(np.int32)
    pairs[3, 3] = -100
    model_scene = np.array([0] * 8 + [1] * 8 + [0, 1], np.int32)
    # the rows' points: a permutation of each scene's points, 100 more points than rows in each scene
    n_pts, row_point = [], np.zeros(R, np.int32)
    for si in range(2):
        mine = np.concatenate([np.arange(b[0], b[0] + b[1]) for b in blocks if b[2] == si])
        n = len(mine) + 100
        row_point[mine] = rng.permutation(n)[:len(mine)]
        n_pts.append(n)
    big = [b for b in blocks if b[1] == 1025]
    row_point[big[0][0] + 7] = n_pts[big[0][2]]  # one point index just outside its scene, one negative
    row_point[big[1][0] + 1000] = -3
    return dict(spec=spec, blocks=np.array(blocks, np.int64), segs=np.array(segs, np.int64), R=R, R2=R2, pn=pn, lab=lab,
                mu=mu, var=var, status=status, pairs=pairs, model_scene=model_scene, n_pts=n_pts, row_point=row_point,
                failed=failed)


def test_expand_and_compete_contract():
    import torch
    from gapro_amd._lib import (Context, PointRefineBlock, PointRefineModel, PointRefineScene, PointRefineSegment)

    ctx = Context.get(0)
    lib = ctx.lib
    dev = torch.device("cuda", 0)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    c = _contract_case()
    R, R2 = c["R"], c["R2"]
    nb, ng, nm = len(c["blocks"]), len(c["segs"]), len(c["status"])
    assert sorted(set(int(b[1]) for b in c["blocks"]))[:7] == [1, 2, 3, 5, 63, 64, 65] and R2 > R > 5000
    blocks, segs = (PointRefineBlock * nb)(), (PointRefineSegment * ng)()
    for q, b in zip(blocks, c["blocks"]):
        q.row_start, q.n_rows, q.scene, q.seg_start, q.n_seg = (int(x) for x in b)
    for q, g in zip(segs, c["segs"]):
        q.out_start, q.model, q.reserved = int(g[0]), int(g[1]), 0
    models = (PointRefineModel * nm)()
    for q, pr, si in zip(models, c["pairs"], c["model_scene"]):
        q.row_offset, q.t, q.scene = 0, 0, int(si)
        q.sem1, q.inst1, q.sem2, q.inst2 = (int(x) for x in pr)
    rng = np.random.default_rng(3)
    start = [(rng.integers(-5, 0, n).astype(np.int32), rng.integers(-9, -5, n).astype(np.int32),
              np.full(n, 1, np.float32), rng.normal(size=n).astype(np.float32) - 50, np.full(n, -100, np.float32))
             for n in c["n_pts"]]
    want_rows, want, want_model = _contract_reference(c, start)

    def dbuf(nbytes):
        return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)

    d_blocks, d_segs = dbuf(C.sizeof(blocks)), dbuf(C.sizeof(segs))
    d_models, d_scenes = dbuf(C.sizeof(models)), dbuf(2 * C.sizeof(PointRefineScene))
    bp, gp, mp = (C.cast(x, C.c_void_p) for x in (blocks, segs, models))
    pb, pg = C.c_void_p(d_blocks.data_ptr()), C.c_void_p(d_segs.data_ptr())

    # ---- expand
    d_rows = torch.full((R2 + 8,), -7, dtype=torch.int32, device=dev)
    assert lib.gapro_point_refine_expand(ctx.handle, stream, nb, bp, pb, ng, gp, pg, R, 2 ** 31, d_rows.data_ptr()) == -1
    assert lib.gapro_point_refine_expand(ctx.handle, stream, nb, bp, pb, ng, gp, pg, R, R2 - 1, d_rows.data_ptr()) == -1
    assert lib.gapro_point_refine_expand(ctx.handle, stream, nb, bp, pb, ng, gp, pg, R - 1, R2, d_rows.data_ptr()) == -1
    assert lib.gapro_point_refine_expand(ctx.handle, stream, nb, bp, pb, ng, gp, pg, R, R2, None) == -1
    assert lib.gapro_point_refine_expand(ctx.handle, stream, 0, None, None, 0, None, None, R, R2, None) == 0
    torch.cuda.synchronize()
    assert (d_rows == -7).all()
    ctx.check(lib.gapro_point_refine_expand(ctx.handle, stream, nb, bp, pb, ng, gp, pg, R, R2, d_rows.data_ptr()))
    torch.cuda.synchronize()
    got_rows = d_rows.cpu().numpy()
    assert (got_rows[R2:] == -7).all() and (want_rows >= 0).all()
    assert np.array_equal(got_rows[:R2], want_rows)

    # ---- compete
    def fresh():
        scenes = (PointRefineScene * 2)()
        t = []
        for sc, arrs, n in zip(scenes, start, c["n_pts"]):
            d = [torch.from_numpy(a).to(dev) for a in arrs]
            sc.n_points, sc.n_spps = n, 1
            sc.sem, sc.inst, sc.prob, sc.mu, sc.var = (x.data_ptr() for x in d)
            t.append(d)
        return scenes, t

    d_in = [torch.from_numpy(a).to(dev) for a in (c["row_point"], c["pn"], c["lab"], c["mu"], c["var"], c["status"])]
    tail = [x.data_ptr() for x in d_in]

    def compete(scenes, n_blocks, row_model, r2=R2, n_models=nm):
        return lib.gapro_point_refine_compete(ctx.handle, stream, 2, C.cast(scenes, C.c_void_p),
                                              C.c_void_p(d_scenes.data_ptr()), n_models, mp,
                                              C.c_void_p(d_models.data_ptr()), n_blocks, bp, pb, ng, gp, pg, R, r2,
                                              *tail, row_model)

    scenes, t = fresh()
    d_row_model = torch.full((R + 8,), -7, dtype=torch.int32, device=dev)
    # refused before anything is launched; n_blocks == 0 is a no-op
    assert compete(scenes, nb, d_row_model.data_ptr(), r2=2 ** 31) == -1
    assert compete(scenes, nb, d_row_model.data_ptr(), r2=R2 - 1) == -1
    assert compete(scenes, nb, d_row_model.data_ptr(), n_models=16) == -1  # a segment names model 16
    blocks[1].row_start -= 1  # overlaps the block before it
    assert compete(scenes, nb, d_row_model.data_ptr()) == -1
    blocks[1].row_start += 1
    assert compete(scenes, 0, d_row_model.data_ptr()) == 0
    torch.cuda.synchronize()
    assert (d_row_model == -7).all()
    for d, arrs in zip(t, start):
        for a, b in zip(d, arrs):
            assert np.array_equal(a.cpu().numpy(), b)
    ctx.check(compete(scenes, nb, d_row_model.data_ptr()))
    torch.cuda.synchronize()
    got_model = d_row_model.cpu().numpy()
    assert (got_model[R:] == -7).all()
    assert np.array_equal(got_model[:R], want_model)
    for si in range(2):
        for j, (a, b) in enumerate(zip(t[si], want[si])):
            a = a.cpu().numpy()
            assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True), (si, j, int((a != b).sum()))
    # what the cases are there for, read off the result
    first = {int(b[0]): (sp, b) for sp, b in zip(c["spec"], c["blocks"])}
    n_kept = 0
    for r0, ((si, n, ms, kind), b) in first.items():
        m = got_model[r0:r0 + n]
        ok = (c["row_point"][r0:r0 + n] >= 0) & (c["row_point"][r0:r0 + n] < c["n_pts"][si])
        if kind in ("tie", "decreasing") and ms[0] not in c["failed"]:
            assert (m[ok] == ms[0]).all(), kind  # an exact tie: the earliest segment; decreasing: the first
        if kind == "ulp":
            assert (m[ok] == ms[-1]).all()  # one float32 step more at every later segment: the last
        if kind == "tie_then_ulp" and len(ms) > 1:
            assert (m[0::2][ok[0::2]] == ms[-1]).all() and (m[1::2][ok[1::2]] == ms[0]).all()
        if kind == "nan_first" and len(ms) > 2:  # a NaN never wins; the last segment's NaNs leave the middle ones
            assert (m[ok] != ms[0]).all() and (m[ok] >= 0).all() and (m[0::3] != ms[-1]).all()
        if kind == "failed_largest":
            assert not np.isin(m, c["failed"]).any() and (m[ok] >= 0).all()
        if all(k in c["failed"] for k in ms) or kind == "all_nan" or (kind == "nan_first" and len(ms) == 1):
            assert (m == -1).all()  # nobody could be taken: the points keep what they held
            n_kept += n
        assert (m[~ok] == -1).all()
    assert n_kept >= 65 + 5 + 66 and int((got_model[:R] == -1).sum()) >= n_kept + 2
    # d_row_model == NULL: the same five arrays
    scenes2, t2 = fresh()
    ctx.check(compete(scenes2, nb, None))
    torch.cuda.synchronize()
    for si in range(2):
        for a, b in zip(t2[si], t[si]):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---------------------------------------------------------------------------------------------- the whole chain
def _assemble(kw, plain, extra):
    """The "compete" result in NumPy from a return_models=True run of the plain pipeline: refined = winner >= 0; the
    testers of a superpoint are the fits whose ``test`` lists it, in ``fits`` order; every tester is evaluated at the
    mask_feats rows of the points of the refined superpoints it tested (predict_gp_batch); per point the first maximum
    under the strict float32 `<`, then the box -> (sem, inst) rule; mu[spp_inv] / var[spp_inv] elsewhere."""
    from gapro_amd.gaussian_process_utils import predict_gp_batch

    sem, ins, prob, mu_s, var_s = (_np(x).copy() for x in plain)
    ranks = np.unique(np.asarray(kw["spp"]), return_inverse=True)[1].reshape(-1)
    mu, var = mu_s[ranks], var_s[ranks]
    winner = extra.winner
    feats = np.ascontiguousarray(np.asarray(kw["mask_feats"], dtype=np.float32))
    n_inst = len(kw["instance_box"])
    boxes_cls = np.concatenate([np.asarray(kw["instance_cls"], dtype=np.int64),
                                np.full(len(kw["wall_box"]) + 1, 18, dtype=np.int64)])
    refined_sp = winner >= 0
    refined = refined_sp[ranks]
    point_fit = np.full(len(ranks), -1, np.int32)
    use = [k for k, f in enumerate(extra.fits) if refined_sp[np.asarray(f.test)].any()]
    if use:
        pts = [np.nonzero(np.isin(ranks, np.asarray(extra.fits[k].test)[refined_sp[np.asarray(extra.fits[k].test)]]))[0]
               for k in use]
        got = predict_gp_batch([extra.fits[k].model for k in use], feats, pts)
        best = np.zeros(len(ranks), np.float32)
        for k, p, (_, p_new, lab, m, v) in zip(use, pts, got):  # ascending k: the order the merge meets the fits
            f = extra.fits[k]
            take = best[p] < p_new  # strict, float32; False for a NaN
            q = p[take]
            box = np.where(lab[take], f.b2, f.b1)
            sem[q] = boxes_cls[box].astype(np.int32)
            ins[q] = np.where(box >= n_inst, -100, box).astype(np.int32)
            prob[q], mu[q], var[q], best[q] = p_new[take], m[take], v[take], p_new[take]
            point_fit[q] = k
    return (sem, ins, prob, mu, var), refined, point_fit, ranks


@pytest.fixture(scope="module")
def runs():
    """Every golden scene once: the return_models run, the "winner" run, the "compete" run and the NumPy assembly."""
    from conftest import GOLDEN_NAMES, Golden
    from gapro_amd import gen_pseudo_label_gaussian_process

    out = {}
    for name in GOLDEN_NAMES:
        kw = Golden(name).api_inputs()
        full = gen_pseudo_label_gaussian_process(**kw, device="cuda:0", return_models=True)
        win = gen_pseudo_label_gaussian_process(**kw, device="cuda:0", point_level=True)
        comp = gen_pseudo_label_gaussian_process(**kw, device="cuda:0", point_level="compete", return_models=True)
        want, refined, point_fit, ranks = _assemble(kw, full[:5], full[5])
        out[name] = dict(kw=kw, full=full, win=tuple(_np(x) for x in win), comp=tuple(_np(x) for x in comp[:5]),
                         models=comp[5], want=want, refined=refined, point_fit=point_fit, ranks=ranks)
    return out


def test_compete_equals_the_assembly_from_the_kept_models(runs):
    from gapro_amd import gen_pseudo_label_gaussian_process

    assert len(runs) == 6
    for name, r in runs.items():
        n = len(r["kw"]["spp"])
        assert [x.dtype for x in r["comp"]] == [np.int32, np.int32, np.float32, np.float32, np.float32]
        assert [len(x) for x in r["comp"]] == [n] * 5
        _same(r["comp"], r["want"], name)
        pf = r["models"].point_fit
        assert pf.dtype == np.int32 and pf.shape == (n,)
        assert np.array_equal(pf, r["point_fit"]), name
        assert np.array_equal(pf >= 0, r["refined"]), name  # every refined point was taken by somebody
        assert np.array_equal(r["models"].winner, r["full"][5].winner)
        other = int(((pf != r["full"][5].winner[r["ranks"]]) & r["refined"]).sum())
        print("%s: %d points, %d refined, %d labelled by another fit than their superpoint's winner"
              % (name, n, int(r["refined"].sum()), other))
        # with no superpoint tested twice the two modes are the same bits
        if name in NO_MULTI:
            _same(r["comp"], r["win"], name + " against point_level=True")
            assert other == 0
        # the probability never falls, and nothing outside a refined superpoint moves
        assert (r["comp"][2] >= r["win"][2]).all(), name
        out = ~r["refined"]
        for j in range(5):
            assert np.array_equal(r["comp"][j][out], r["win"][j][out], equal_nan=True), (name, j)
        for j in range(3):
            assert np.array_equal(r["comp"][j][out], _np(r["full"][j])[out]), (name, j)
    # "winner" is True; the plain outputs do not know about the feature; return_models without compete has no point_fit
    kw = runs["s2_dense"]["kw"]
    _same(gen_pseudo_label_gaussian_process(**kw, device="cuda:0", point_level="winner"), runs["s2_dense"]["win"], "winner")
    assert runs["s2_dense"]["full"][5].point_fit is None
    with pytest.raises(ValueError):
        gen_pseudo_label_gaussian_process(**kw, device="cuda:0", point_level="nonsense")


@pytest.mark.parametrize("backend", ["torch", "native"])
def test_batches_do_not_change_a_scene(runs, backend):
    """All six goldens as one batch and as three software-pipelined batches of two, the scene without fits first: per
    scene the bits of the single-scene run, on both backends."""
    from gapro_amd.gen_ps_utils import gen_pseudo_label_gaussian_process_batch
    from gapro_amd.pipeline import Pipeline, make_job

    names = ["s3_bigspp"] + [n for n in runs if n != "s3_bigspp"]
    if backend == "torch":
        import torch
        from gapro_amd.gen_ps_utils import _pipeline

        outs = gen_pseudo_label_gaussian_process_batch([runs[n]["kw"] for n in names], device="cuda:0",
                                                       point_level="compete")
        pipe, be = _pipeline(torch.device("cuda:0"), 50, point_level="compete"), None  # the pipeline that call used
    else:
        pipe = Pipeline(device=0, training_iter=50, backend="native", point_level="compete")
        be, outs = pipe.be, None
    assert pipe.point_level is True and pipe.point_mode == "compete"

    def jobs(ns):
        return [make_job(*[runs[n]["kw"][k] for k in ARGS], **OPTS, backend=be) for n in ns]

    if outs is None:
        outs = pipe.run(jobs(names))
    for n, o in zip(names, outs):
        _same(o, runs[n]["want"], "%s in one batch (%s)" % (n, backend))
    lr = pipe.last_refine
    assert (lr["refined_spps"], lr["rows"], lr["expanded_rows"], lr["multi_spps"]) == (160, 2974, 4585, 31)
    assert lr["rows"] == sum(int(runs[n]["refined"].sum()) for n in names)
    pairs = [names[0:2], names[2:4], names[4:6]]
    got = list(pipe.run_stream(iter([jobs(p) for p in pairs])))
    assert len(got) == 3
    for p, batch in zip(pairs, got):
        for n, o in zip(p, batch):
            _same(o, runs[n]["want"], "%s in a streamed pair (%s)" % (n, backend))
    assert pipe.last_refine["rows"] == sum(int(runs[n]["refined"].sum()) for n in pairs[-1])


def test_cli_point_compete_in_a_fresh_process(tmp_path):
    """`gen_ps --point_compete --devices 0` over a small synthetic dataset in a child process: exit status 0, torch never
    imported, and every label file holds the five point-length arrays of Pipeline(point_level="compete")."""
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
            "rc = gen_ps.main(['--save_folder', sys.argv[1], '--data_root', %r, '--point_compete', '--devices', '0'])\n"
            "print('TORCH_IMPORTED', 'torch' in sys.modules)\n"
            "sys.exit(rc)\n" % (ROOT, root))
    env = {k: v for k, v in os.environ.items() if k != "GAPRO_BACKEND"}
    r = subprocess.run([sys.executable, "-c", code, save], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "2 scenes written, 0 skipped/failed" in r.stdout
    assert "TORCH_IMPORTED False" in r.stdout and "the library's own arena" in r.stdout, r.stdout
    pipe = Pipeline(device=0, training_iter=50, point_level="compete")
    jobs = []
    for s in scenes:
        sc = load_scene(os.path.join(root, "train", s.scan_name + "_inst_nostuff.pth"), root)
        jobs.append(make_job(*[sc[k] for k in ARGS], **OPTS, device="cuda:0"))
    outs = pipe.run(jobs)
    print("the two scenes: %(refined_spps)d refined superpoints, %(multi_spps)d tested by several fits, %(rows)d -> "
          "%(expanded_rows)d rows" % pipe.last_refine)
    assert pipe.last_refine["rows"] > 0
    for s, o in zip(scenes, outs):
        tup = torch.load(os.path.join(save, s.scan_name + ".pth"), weights_only=False)
        assert len(tup) == 5 and [len(a) for a in tup] == [s.n_points] * 5
        _same(o, tup, s.scan_name)
