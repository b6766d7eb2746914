"""Point-level labels inside GP-labelled superpoints (Pipeline(point_level=True), csrc/point_refine.hip) on the MI355X.

The composition tests are bit for bit: the point-level chain and the NumPy assembly below run the same predict kernel on
the same states and the same feature rows (a predict row's result is its own), so every difference is a
defect of the new code and no tolerance applies.  Only the comparison with the float64 posterior has tolerances, the ones
tests/test_predict_gpu.py derives: var rtol 2^-23, mu rtol 2^-23 + atol 1e-10, p atol 1.2e-7.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP = 2.0 ** -23
ARGS = ("coords_float", "mask_feats", "spp", "instance_cls", "instance_box", "instance_box_volume", "wall_box",
        "wall_box_volume")
OPTS = dict(instance_classes=18, ground_h=0.1, thresh_spp_occu=0.999)


def _np(t):
    if isinstance(t, np.ndarray):
        return t
    h = t.cpu()
    return h if isinstance(h, np.ndarray) else h.numpy()


def _assemble(kw, plain, extra):
    """The point-level result in NumPy from a return_models=True run: the winners it returns, ranks from np.unique,
    predict_gp_batch of the winning models at the mask_feats rows of their superpoints' points, the box -> (sem, inst)
    rule, mu[spp_inv] / var[spp_inv] elsewhere.  Also the refined mask, and per point the model index and the label."""
    from gapro_amd.gaussian_process_utils import predict_gp_batch

    sem, ins, prob, mu_s, var_s = (_np(x).copy() for x in plain)
    ranks = np.unique(np.asarray(kw["spp"]), return_inverse=True)[1].reshape(-1)
    mu, var = mu_s[ranks], var_s[ranks]
    winner = extra.winner
    assert winner.dtype == np.int32 and winner.shape == mu_s.shape
    feats = np.ascontiguousarray(np.asarray(kw["mask_feats"], dtype=np.float32))
    n_inst = len(kw["instance_box"])
    boxes_cls = np.concatenate([np.asarray(kw["instance_cls"], dtype=np.int64),
                                np.full(len(kw["wall_box"]) + 1, 18, dtype=np.int64)])
    won = [int(k) for k in np.unique(winner) if k >= 0]
    pts = [np.nonzero(np.isin(ranks, np.nonzero(winner == k)[0]))[0] for k in won]
    refined = np.zeros(len(ranks), dtype=bool)
    which = np.full(len(ranks), -1)
    label = np.zeros(len(ranks), dtype=bool)
    if won:
        got = predict_gp_batch([extra.fits[k].model for k in won], feats, pts)
        for k, p, (_, p_new, lab, m, v) in zip(won, pts, got):
            f = extra.fits[k]
            box = np.where(lab, f.b2, f.b1)
            sem[p] = boxes_cls[box].astype(np.int32)
            ins[p] = np.where(box >= n_inst, -100, box).astype(np.int32)
            prob[p], mu[p], var[p] = p_new, m, v
            refined[p], which[p], label[p] = True, k, lab
    return (sem, ins, prob, mu, var), refined, which, label


@pytest.fixture(scope="module")
def runs():
    """Every golden scene once: the plain run, the return_models run, the point_level run and the NumPy assembly."""
    from conftest import GOLDEN_NAMES, Golden
    from gapro_amd import gen_pseudo_label_gaussian_process

    out = {}
    for name in GOLDEN_NAMES:
        kw = Golden(name).api_inputs()
        plain = gen_pseudo_label_gaussian_process(**kw, device="cuda:0")
        full = gen_pseudo_label_gaussian_process(**kw, device="cuda:0", return_models=True)
        point = gen_pseudo_label_gaussian_process(**kw, device="cuda:0", point_level=True)
        want, refined, which, label = _assemble(kw, full[:5], full[5])
        out[name] = dict(kw=kw, plain=plain, full=full, point=tuple(_np(x) for x in point), want=want, refined=refined,
                         which=which, label=label)
    return out


def _same(got, want, what):
    assert len(got) == len(want) == 5
    for j, (a, b) in enumerate(zip(got, want)):
        a = _np(a)
        assert a.dtype == b.dtype and a.shape == b.shape, (what, j, a.dtype, b.dtype, a.shape, b.shape)
        assert np.array_equal(a, b), "%s: output %d differs at %d of %d points" % (what, j, int((a != b).sum()), len(a))


def test_point_level_equals_the_assembly_from_the_kept_models(runs):
    n_ref = 0
    for name, r in runs.items():
        n = len(r["kw"]["spp"])
        assert [x.dtype for x in r["point"]] == [np.int32, np.int32, np.float32, np.float32, np.float32]
        assert [len(x) for x in r["point"]] == [n] * 5
        _same(r["point"], r["want"], name)
        print("%s: %d points, %d refined, %d models" % (name, n, int(r["refined"].sum()), len(np.unique(r["which"])) - 1))
        if name == "s3_bigspp":  # no fit: the broadcast of the plain result
            assert not r["refined"].any() and len(r["full"][5].fits) == 0
            ranks = np.unique(np.asarray(r["kw"]["spp"]), return_inverse=True)[1].reshape(-1)
            assert np.array_equal(r["point"][3], _np(r["plain"][3])[ranks])
        else:
            assert r["refined"].any()
        n_ref += int(r["refined"].sum())
    assert n_ref > 1000


def test_nothing_else_moves(runs):
    import torch

    changed = 0
    for name, r in runs.items():
        for a, b in zip(r["plain"], r["full"][:5]):  # the plain outputs do not know about the feature
            assert a.dtype == b.dtype and torch.equal(a, b)
        assert len(r["plain"][3]) == len(r["plain"][4]) == len(r["full"][5].winner) < len(r["plain"][0])
        out = ~r["refined"]
        for j in range(3):
            assert np.array_equal(r["point"][j][out], _np(r["plain"][j])[out]), (name, j)
        changed += int((r["point"][1] != _np(r["plain"][1])).sum())
        if r["refined"].any():  # a point's own features are not its superpoint's mean: its mu is its own
            ranks = np.unique(np.asarray(r["kw"]["spp"]), return_inverse=True)[1].reshape(-1)
            assert (r["point"][3] != _np(r["plain"][3])[ranks])[r["refined"]].any(), name
    print("refined points whose instance differs from their superpoint's: %d" % changed)
    # keyword-only, and broadcast_mu_var has nothing left to do
    from conftest import Golden
    from gapro_amd import gen_pseudo_label_gaussian_process

    kw = Golden("s5_lean").api_inputs()
    both = gen_pseudo_label_gaussian_process(**kw, device="cuda:0", point_level=True, broadcast_mu_var=True)
    _same(both, runs["s5_lean"]["point"], "point_level + broadcast_mu_var")
    with pytest.raises(TypeError):
        gen_pseudo_label_gaussian_process(*[kw[k] for k in ARGS], 18, "scannetv2", 0.1, 50, 0.999, True)


def _order(runs):
    return ["s3_bigspp"] + [n for n in runs if n != "s3_bigspp"]  # a scene without fits leads the batch / a pair


@pytest.mark.parametrize("backend", ["torch", "native"])
def test_batches_do_not_change_a_scene(runs, backend):
    """All six goldens as one batch and as three software-pipelined batches of two (the first pair led by the scene
    without fits): per scene the bits of the single-scene run -- row bases, scene offsets, slots, both backends."""
    from gapro_amd.gen_ps_utils import gen_pseudo_label_gaussian_process_batch
    from gapro_amd.pipeline import Pipeline, make_job

    names = _order(runs)
    if backend == "torch":
        outs = gen_pseudo_label_gaussian_process_batch([runs[n]["kw"] for n in names], device="cuda:0", point_level=True)
        import torch
        from gapro_amd.gen_ps_utils import _pipeline

        pipe, be = _pipeline(torch.device("cuda:0"), 50, point_level=True), None  # the pipeline that call used
        assert isinstance(pipe, Pipeline) and pipe.point_level
    else:
        pipe = Pipeline(device=0, training_iter=50, backend="native", point_level=True)
        be = pipe.be
        outs = None

    def jobs(ns):
        return [make_job(*[runs[n]["kw"][k] for k in ARGS], **OPTS, backend=be) for n in ns]

    if outs is None:
        outs = pipe.run(jobs(names))
    for n, o in zip(names, outs):
        _same(o, runs[n]["want"], "%s in one batch (%s)" % (n, backend))
    assert pipe.last_refine["rows"] == sum(int(runs[n]["refined"].sum()) for n in names)
    pairs = [names[0:2], names[2:4], names[4:6]]
    got = list(pipe.run_stream(iter([jobs(p) for p in pairs])))
    assert len(got) == 3
    for p, batch in zip(pairs, got):
        for n, o in zip(p, batch):
            _same(o, runs[n]["want"], "%s in a streamed pair (%s)" % (n, backend))
    # the plan of the last batch: its rows are the refined points of its two scenes, blocks disjoint and complete
    assert pipe.last_refine["rows"] == sum(int(runs[n]["refined"].sum()) for n in pairs[-1])
    assert pipe.last_refine["models"] == sum(len(np.unique(runs[n]["which"])) - 1 for n in pairs[-1])


@pytest.mark.parametrize("name", ["s2_dense", "s5_lean"])
def test_refined_points_against_the_float64_posterior(runs, name):
    """mu, sigma^2 and p of every refined point against the float64 posterior of the exported model at the point's own
    features (the oracle starts from the trained state: numerically soft fits do not enter).  p is derived from the
    point's probability with the label of its row: label ? prob : 1 - prob, exact in float32 for prob in [0.5, 1]; where
    the label is 0 the kernel's own 1 - p rounded once more (<= 2^-25), which with one float32 step of p below 0.5
    (<= 2^-25) stays inside the 1.2e-7 the predict tests allow."""
    from oracle import svgp_oracle as so

    r = runs[name]
    feats = np.asarray(r["kw"]["mask_feats"], dtype=np.float32)
    fits = r["full"][5].fits
    sizes = set()
    for k in np.unique(r["which"][r["refined"]]):
        mo = fits[int(k)].model
        sizes.add(mo.m)
        p = np.nonzero(r["which"] == k)[0]
        s, ell = mo.outputscale, mo.lengthscale
        d2 = ((mo.Z[:, None, :] - mo.Z[None, :, :]) ** 2).sum(-1)
        L = np.linalg.cholesky(s * np.exp(-0.5 * d2 / (ell * ell)) + mo.jitter * np.eye(mo.m))
        mu_r, var_r, p_r = so.svgp_predict(feats[p].astype(np.float64), mo.Z, mo.mean, mo.LS, mo.c, mo.rho_s, mo.rho_l,
                                           jitter=mo.jitter, L=L)
        _, _, prob, mu, var = (x[p] for x in r["point"])
        pd = np.where(r["label"][p], prob, np.float32(1) - prob)
        print("%s fit %d (M = %d, %d points): var rel %.3e  mu abs %.3e  p abs %.3e" % (
            name, k, mo.m, len(p), np.max(np.abs(var - var_r.astype(np.float32)) / var_r),
            np.max(np.abs(mu - mu_r.astype(np.float32))), np.max(np.abs(pd - p_r.astype(np.float32)))))
        np.testing.assert_allclose(var, var_r.astype(np.float32), rtol=ULP, atol=0)
        np.testing.assert_allclose(mu, mu_r.astype(np.float32), rtol=ULP, atol=1e-10)
        np.testing.assert_allclose(pd, p_r.astype(np.float32), rtol=0, atol=1.2e-7)
        assert ((prob >= 0.5) & (prob <= 1)).all()
    assert sizes and max(sizes) <= 128


def test_gather_contract():
    """gapro_point_refine_gather alone, two synthetic scenes of 2000 / 2137 points at feature width 7: per refined
    superpoint the block holds exactly its points (in any order) and every row its point's features, bit for bit; nothing
    outside the blocks is written.  Refined: a superpoint of one point, two of adjacent ids, the first and the last id."""
    import torch
    from gapro_amd import _lib
    from gapro_amd._lib import Context, PointRefineScene

    ctx = Context.get(0)
    lib = ctx.lib
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    D, S = 7, 41
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    scenes = (PointRefineScene * 2)()
    d_scenes = torch.empty(2 * C.sizeof(PointRefineScene), dtype=torch.uint8, device=dev)
    host, keep, rows = [], [], 0
    for si, n in enumerate((2000, 2137)):
        inv = rng.integers(0, S - 1, size=n).astype(np.int32)
        inv[inv == 17] = 18  # superpoint 17 gets exactly one point; S - 1 is the last id
        inv[n // 2] = 17
        inv[-3:] = S - 1
        feats = rng.normal(size=(n, D)).astype(np.float32)
        refined = [0, 9, 10, 17, 30, S - 1] if si == 0 else [3, 4, 17, 25]
        cnt = np.bincount(inv, minlength=S)
        sp_row = np.full(S, -1, dtype=np.int64)
        for sp in refined:
            sp_row[sp] = rows
            rows += int(cnt[sp])
        t = [torch.from_numpy(a).to(dev) for a in (inv, feats, sp_row)] + [torch.full((S,), 99, dtype=torch.int32,
                                                                                      device=dev)]
        keep.append(t)
        sc = scenes[si]
        sc.n_points, sc.n_spps = n, S
        sc.spp_inv, sc.feats, sc.sp_row, sc.cursor = (x.data_ptr() for x in t)
        host.append((inv, feats, sp_row, refined, cnt))
    R = rows
    row_feats = torch.full((R + 8, D), -7.0, dtype=torch.float32, device=dev)
    row_point = torch.full((R + 8,), -7, dtype=torch.int32, device=dev)
    sp = C.cast(scenes, C.c_void_p)
    args = (ctx.handle, stream, 2, D, sp, C.c_void_p(d_scenes.data_ptr()))
    # refused or nothing to do, before anything is launched
    assert lib.gapro_point_refine_gather(*args, -1, row_feats.data_ptr(), row_point.data_ptr()) == -1
    assert lib.gapro_point_refine_gather(*args, 2 ** 31, row_feats.data_ptr(), row_point.data_ptr()) == -1
    assert lib.gapro_point_refine_gather(*args, R, None, row_point.data_ptr()) == -1
    assert lib.gapro_point_refine_gather(ctx.handle, stream, -2, D, sp, C.c_void_p(d_scenes.data_ptr()), R,
                                         row_feats.data_ptr(), row_point.data_ptr()) == -1
    assert lib.gapro_point_refine_gather(*args, 0, None, None) == 0
    torch.cuda.synchronize()
    assert (row_point == -7).all() and (keep[0][3] == 99).all()
    ctx.check(lib.gapro_point_refine_gather(*args, R, row_feats.data_ptr(), row_point.data_ptr()))
    torch.cuda.synchronize()
    rf, rp = row_feats.cpu().numpy(), row_point.cpu().numpy()
    assert (rp[R:] == -7).all() and (rf[R:] == -7.0).all()
    assert 1 in [int(h[4][17]) for h in host]
    for si, (inv, feats, sp_row, refined, cnt) in enumerate(host):
        cur = keep[si][3].cpu().numpy()
        for s in range(S):
            assert cur[s] == (cnt[s] if s in refined else 0)
        for s in refined:
            a, b = int(sp_row[s]), int(sp_row[s]) + int(cnt[s])
            assert sorted(rp[a:b].tolist()) == np.nonzero(inv == s)[0].tolist(), (si, s)
            assert np.array_equal(rf[a:b].view(np.uint32), feats[rp[a:b]].view(np.uint32)), (si, s)
    assert _lib.GAPRO_OK == 0


def test_cli_point_level_in_a_fresh_process(tmp_path):
    """`gen_ps --point_level --devices 0` over a small synthetic dataset in a child process: exit status 0, torch never
    imported, and every label file holds the five point-length arrays of the API's point_level run on the same scene."""
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
            "rc = gen_ps.main(['--save_folder', sys.argv[1], '--data_root', %r, '--point_level', '--devices', '0'])\n"
            "print('TORCH_IMPORTED', 'torch' in sys.modules)\n"
            "sys.exit(rc)\n" % (ROOT, root))
    env = {k: v for k, v in os.environ.items() if k != "GAPRO_BACKEND"}
    r = subprocess.run([sys.executable, "-c", code, save], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "2 scenes written, 0 skipped/failed" in r.stdout
    assert "TORCH_IMPORTED False" in r.stdout and "the library's own arena" in r.stdout, r.stdout
    pipe = Pipeline(device=0, training_iter=50, point_level=True)
    jobs = []
    for s in scenes:
        sc = load_scene(os.path.join(root, "train", s.scan_name + "_inst_nostuff.pth"), root)
        jobs.append(make_job(*[sc[k] for k in ARGS], **OPTS, device="cuda:0"))
    n_diff = 0
    for s, job, o in zip(scenes, jobs, pipe.run(jobs)):
        tup = torch.load(os.path.join(save, s.scan_name + ".pth"), weights_only=False)
        assert len(tup) == 5 and [len(a) for a in tup] == [s.n_points] * 5
        _same(o, tup, s.scan_name)
        inv = _np(job.spp_inv).astype(np.int64)
        lo, hi = np.full(job.n_spps, np.inf), np.full(job.n_spps, -np.inf)
        np.minimum.at(lo, inv, tup[3])
        np.maximum.at(hi, inv, tup[3])
        n_diff += int((lo != hi).sum())  # superpoints whose points do not share one mu
    assert n_diff > 0, "no point-level value in the files: the fixture scenes have no refined superpoint"
