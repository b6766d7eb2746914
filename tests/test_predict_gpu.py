"""State export of the batched fit and gapro_svgp_predict_batch on the MI355X.

Tolerance of every comparison with float64 references (derived, not tuned: predicting from a fixed state is well
conditioned -- on the CPU, triangular solves against an explicit inv(L) differ by at most 4.8e-12 relative in sigma^2,
3.2e-13 in mu, 1.2e-13 in p up to M = 1040 on these row sets): two float64 evaluations that close round to float32
values at most one unit in the last place apart, so var rtol 2^-23, mu rtol 2^-23 + atol 1e-10, probs atol 1.2e-7;
labels equal wherever the reference's |p - 0.5| > 1e-6 (at most 0.1 % of a model's rows may be left out); probs_new ==
where(labels, probs, 1 - probs) exactly.
"""
import time

import numpy as np
import pytest

from predict_edge_cases import _as_ref, _check, _oracle

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
SIZES = [(1, 2, 6), (3, 4, 6), (20, 30, 6), (16, 16, 6), (40, 60, 6), (70, 80, 6), (10, 12, 32), (30, 40, 32),
         (120, 136, 6), (150, 170, 6), (260, 270, 6), (20, 25, 40), (500, 540, 6)]
T_FIT = 40


def _std(d):
    return 0.3 if d > 8 else 1.0


def _problem(m1, m2, d, t=T_FIT):
    from gapro_amd.synth import make_gp_problem

    return make_gp_problem(7 + m1, m1, m2, t, d, std=_std(d))


@pytest.fixture(scope="module")
def trained():
    """Every size of SIZES trained once, 50 steps, one mixed launch per feature width: plain call and return_models."""
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch

    by_d = {}
    for (m1, m2, d) in SIZES:
        by_d.setdefault(d, []).append((m1, m2))
    out = {}
    for d, sizes in by_d.items():
        parts, probs, base = [], [], 0
        for (m1, m2) in sizes:
            f, b1, b2, it = _problem(m1, m2, d)
            parts.append(f)
            probs.append((b1 + base, b2 + base, it + base))
            base += len(f)
        feats = np.concatenate(parts)
        plain, res_p, st_p = fit_gp_spp_batch(feats, probs, training_iter=50, keep_debug=True, return_status=True)
        outs, models, res_m, st_m = fit_gp_spp_batch(feats, probs, training_iter=50, return_models=True, keep_debug=True,
                                                     return_status=True)
        out[d] = dict(feats=feats, probs=probs, plain=plain, outs=outs, models=models, sizes=sizes,
                      loss=(res_p["loss"], res_m["loss"]), status=(st_p, st_m))
    return out


def _each(trained):
    for d, g in trained.items():
        for k, (m1, m2) in enumerate(g["sizes"]):
            yield d, m1, m2, g, k


def test_nothing_moves_when_a_state_is_asked_for(trained):
    from gapro_amd import _lib

    lib = _lib.load()
    routes = set()
    for d, g in trained.items():
        assert np.array_equal(g["status"][0], g["status"][1]) and (g["status"][0] == 0).all()
        assert np.array_equal(g["loss"][0], g["loss"][1])
        for a, b in zip(g["plain"], g["outs"]):
            for u, v in zip(a, b):
                assert u.dtype == v.dtype and np.array_equal(u, v)
        routes |= {int(lib.gapro_fit_route(m1 + m2, d)) for m1, m2 in g["sizes"]}
    assert routes == {0, 1, 2, 3, 4, 5}, routes  # every fit kernel family exported a state


def test_state_has_the_documented_shape(trained):
    for d, m1, m2, g, k in _each(trained):
        mo = g["models"][k]
        M = m1 + m2
        assert mo.Z.shape == (M, d) and mo.mean.shape == (M,) and mo.LS.shape == (M, M) and mo.status == 0
        assert mo.jitter == 1e-4 and np.array_equal(mo.LS, np.tril(mo.LS))
        assert np.isfinite(mo.Z).all() and np.isfinite(mo.mean).all() and np.isfinite(mo.LS).all()
        X = np.concatenate([g["feats"][g["probs"][k][0]], g["feats"][g["probs"][k][1]]]).astype(np.float64)
        assert np.abs(mo.Z - X).max() < 10.0 and not np.array_equal(mo.Z, X)  # trained away from Z = X, not far


def test_the_state_is_the_model_the_fit_predicted_with(trained):
    from gapro_amd.gaussian_process_utils import predict_gp_batch

    for d, g in trained.items():
        got = predict_gp_batch(g["models"], g["feats"], [p[2] for p in g["probs"]])
        for k, (m1, m2) in enumerate(g["sizes"]):
            _check(got[k], _as_ref(g["outs"][k]), "own test set (%d,%d,%d)" % (m1, m2, d))


def _unseen_rows(m1, m2, d, model):
    from gapro_amd.synth import make_gp_problem

    n = 5000 if m1 + m2 > 1000 else 20000
    f = make_gp_problem(1000 + m1, m1, m2, n, d, std=_std(d))[0][m1 + m2:]
    assert len(f) == n
    return np.concatenate([f, 4.0 * f[:2000], model.Z.astype(np.float32)]).astype(np.float32)


def test_predict_kernel_against_the_oracle_at_unseen_inputs(trained):
    from gapro_amd.gaussian_process_utils import predict_gp_batch

    for d, g in trained.items():
        tables = [_unseen_rows(m1, m2, d, g["models"][k]) for k, (m1, m2) in enumerate(g["sizes"])]
        base = np.cumsum([0] + [len(t) for t in tables])
        feats = np.concatenate(tables)
        rows = [np.arange(base[k], base[k + 1]) for k in range(len(tables))]
        got = predict_gp_batch(g["models"], feats, rows)
        for k, (m1, m2) in enumerate(g["sizes"]):
            _check(got[k], _oracle(g["models"][k], tables[k]), "unseen (%d,%d,%d)" % (m1, m2, d))


def test_a_rows_result_is_its_own(trained):
    from gapro_amd.gaussian_process_utils import predict_gp_batch

    g = trained[6]
    rng = np.random.default_rng(12)
    tables = [_unseen_rows(m1, m2, 6, g["models"][k])[:3000 + 37 * k] for k, (m1, m2) in enumerate(g["sizes"])]
    base = np.cumsum([0] + [len(t) for t in tables])
    feats = np.concatenate(tables)
    rows = [np.arange(base[k], base[k + 1]) for k in range(len(tables))]
    together = predict_gp_batch(g["models"], feats, rows)
    for k in range(len(tables)):
        alone = predict_gp_batch([g["models"][k]], feats, [rows[k]])[0]
        cut = 1 + int(rng.integers(0, len(rows[k]) - 1))
        two = [predict_gp_batch([g["models"][k]], feats, [r])[0] for r in (rows[k][:cut], rows[k][cut:])]
        perm = rng.permutation(len(rows[k]))
        shuffled = predict_gp_batch([g["models"][k]], feats, [rows[k][perm]])[0]
        for j in range(5):
            assert np.array_equal(together[k][j], alone[j]), (k, j)
            assert np.array_equal(np.concatenate([two[0][j], two[1][j]]), alone[j]), (k, j, cut)
            back = np.empty_like(shuffled[j])
            back[perm] = shuffled[j]
            assert np.array_equal(back, alone[j]), (k, j)


def test_large_t_and_t_zero():
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch, predict_gp_batch
    from gapro_amd.synth import make_gp_problem

    feats, b1, b2, it = make_gp_problem(57, 40, 60, 30, 6)
    _, models = fit_gp_spp_batch(feats, [(b1, b2, it)], training_iter=50, return_models=True)
    table = make_gp_problem(1040, 40, 60, 20000, 6)[0][100:]
    rng = np.random.default_rng(8)
    rows = rng.integers(0, len(table), size=1_000_000)
    out = predict_gp_batch(models, table, [rows])[0]
    assert all(len(o) == 1_000_000 for o in out)
    pick = rng.choice(1_000_000, size=50_000, replace=False)
    _check(tuple(o[pick] for o in out), _oracle(models[0], table[rows[pick]]), "T = 1e6 sample")
    # T = 0: nothing to do, nothing written, status OK -- alone and beside a model that has rows
    outs, st = predict_gp_batch(models, table, [np.zeros(0, np.int64)], return_status=True)
    assert st[0] == 0 and all(len(o) == 0 for o in outs[0])
    outs, st = predict_gp_batch(models * 2, table, [np.zeros(0, np.int64), rows[:100]], return_status=True)
    assert (st == 0).all() and len(outs[0][0]) == 0
    for j in range(5):
        assert np.array_equal(outs[1][j], out[j][:100])


def test_psd_retry_rule():
    """The duplicated-inducing-point construction of test_fit_gpu.py::test_psd_safe_cholesky_jitter_retries (variational
    jitter 0, zero training steps, so Z keeps its duplicates): K_ZZ is singular and whether a pivot comes out <= 0 is
    decided by the last bit, so variations are tried until predict without retries fails; with the default retries the
    same model reproduces the fit's outputs, and the clean neighbour of the same launch is untouched either way."""
    import torch
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch, predict_gp_batch
    from gapro_amd.gen_ps_utils import _pipeline
    from gapro_amd.synth import make_gp_problem

    f2, c1, c2, ct = make_gp_problem(34, 20, 25, 4, 6)
    pipe = _pipeline(torch.device("cuda", 0), 0)
    pipe50 = _pipeline(torch.device("cuda", 0), 50)  # predict_gp_batch takes its options from this one
    old = (pipe.opt.jitter, pipe.opt.psd_retries, pipe50.opt.psd_retries)
    found = False
    try:
        for seed in range(24):
            feats, b1, b2, it = make_gp_problem(330 + seed, 12, 14, 6, 6)
            feats = feats.copy()
            for k in range(1, 5):  # five copies of one point, three of another
                feats[b1[k]] = feats[b1[0]]
            feats[b2[5]] = feats[b2[2]]
            feats[b2[7]] = feats[b2[2]]
            allf = np.concatenate([feats, f2])
            off = len(feats)
            launch = [(b1, b2, it), (c1 + off, c2 + off, ct + off)]
            pipe.opt.jitter, pipe.opt.psd_retries = 0.0, 3
            outs, models, status = fit_gp_spp_batch(allf, launch, training_iter=0, return_models=True,
                                                    return_status=True)
            pipe.opt.jitter = old[0]
            assert (status == 0).all() and models[0].jitter == 0.0 and models[1].jitter == 0.0
            rows = [it, ct + off]
            pipe50.opt.psd_retries = 0
            got0, st0 = predict_gp_batch(models, allf, rows, return_status=True)
            pipe50.opt.psd_retries = 3
            assert st0[1] == 0
            if st0[0] == 0:
                continue  # every pivot of this variation happened to round to a positive number
            assert st0[0] == -5
            got, st = predict_gp_batch(models, allf, rows, return_status=True)
            assert (st == 0).all()
            for j in range(5):
                assert np.array_equal(got0[1][j], got[1][j])  # the clean neighbour does not notice
            _check(got[0], _as_ref(outs[0]), "duplicated points, retries", untrained=True)
            _check(got[1], _as_ref(outs[1]), "clean neighbour", untrained=True)
            found = True
            break
    finally:
        pipe.opt.jitter, pipe.opt.psd_retries, pipe50.opt.psd_retries = old
    assert found, "no variation produced a non-positive pivot"


def test_model_of_a_failed_fit_is_refused():
    from gapro_amd._lib import GaproError
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch, predict_gp_batch
    from gapro_amd.synth import make_gp_problem

    parts, probs, base = [], [], 0
    for i, (m1, m2) in enumerate([(20, 30), (70, 80), (9, 11)]):
        f, b1, b2, it = make_gp_problem(60 + i, m1, m2, 12, 6)
        parts.append(f.copy())
        probs.append((b1 + base, b2 + base, it + base))
        base += len(f)
    parts[1][5, 2] = np.nan  # a training superpoint of the second fit
    feats = np.concatenate(parts)
    outs, models, status = fit_gp_spp_batch(feats, probs, training_iter=50, return_models=True, return_status=True)
    assert status[0] == 0 and status[2] == 0 and status[1] != 0
    assert [m.status for m in models] == [int(s) for s in status]
    clean = np.nan_to_num(feats)
    rows = [p[2] for p in probs]
    with pytest.raises((ValueError, GaproError)):
        predict_gp_batch(models, clean, rows)
    got, st = predict_gp_batch(models, clean, rows, return_status=True)
    assert st[0] == 0 and st[2] == 0 and st[1] == status[1]
    for k in (0, 2):
        _check(got[k], _as_ref(outs[k]), "neighbour %d of a failed fit" % k)
    # non-finite FEATURES at predict time: that model says so, the others are served
    dirty = clean.copy()
    dirty[rows[0][3], 1] = np.nan
    got2, st2 = predict_gp_batch([models[0], models[2]], dirty, [rows[0], rows[2]], return_status=True)
    assert st2[0] == -4 and st2[1] == 0
    for j in range(5):
        assert np.array_equal(got2[1][j], got[2][j])


def test_scene_level_models_on_the_golden_scene():
    import torch
    from conftest import Golden
    from gapro_amd import gen_pseudo_label_gaussian_process
    from gapro_amd.gaussian_process_utils import predict_gp_batch

    g = Golden("s2_dense")
    kw = g.api_inputs()
    plain = gen_pseudo_label_gaussian_process(**kw, device="cuda:0")
    full = gen_pseudo_label_gaussian_process(**kw, device="cuda:0", return_models=True)
    assert len(plain) == 5 and len(full) == 6
    for a, b in zip(plain, full[:5]):
        assert a.dtype == b.dtype and torch.equal(a, b)
    extra = full[5]
    fits = extra.fits
    assert len(fits) == 24 == len(g.fits)
    for f, r in zip(fits, g.fits):
        assert len(f) == 5 and f.model.status == 0
        np.testing.assert_array_equal(f.train, np.concatenate([r["b1_inds"], r["b2_inds"]]))
        np.testing.assert_array_equal(f[3], r["intersect_inds"])
        assert f.m1 == len(r["b1_inds"])
    feats_spp = extra.feats_spp
    mu, var = full[3].cpu().numpy(), full[4].cpu().numpy()
    assert feats_spp.shape == (len(mu), 6) and feats_spp.dtype == np.float32
    models = [f.model for f in fits]
    at_test = predict_gp_batch(models, feats_spp, [f.test for f in fits])
    labelled = np.nonzero(mu != -100)[0]
    assert len(labelled)
    for s in labelled:
        ok = False
        for f, o in zip(fits, at_test):
            pos = np.nonzero(f.test == s)[0]
            if len(pos):
                m_, v_ = o[3][pos[0]], o[4][pos[0]]
                ok = ok or (abs(float(v_) - float(var[s])) <= ULP * abs(float(var[s]))
                            and abs(float(m_) - float(mu[s])) <= 1e-10 + ULP * abs(float(mu[s])))
        assert ok, "superpoint %d: no model that tested it predicts its (mu, var)" % s
    # point resolution: every model at the raw features of the points inside its test superpoints
    ranks = np.unique(np.asarray(kw["spp"]), return_inverse=True)[1].reshape(-1)
    pts = [np.nonzero(np.isin(ranks, f.test))[0] for f in fits]
    pf = np.asarray(kw["mask_feats"], dtype=np.float32)
    got = predict_gp_batch(models, pf, pts)
    for k, f in enumerate(fits):
        assert len(pts[k]) >= len(f.test)
        _check(got[k], _oracle(f.model, pf[pts[k]]), "points of fit %d" % k)


def test_predict_costs_less_than_the_fit_on_the_s3dis_shaped_scene():
    """From the operation counts alone: predicting a model at T rows is M^3 / 3 + 2 M^2 T, training it at least
    50 x 7.67 M^3 -- a factor of more than a hundred on this scene's 66 fits (every route).  A sanity bound."""
    import torch
    from gapro_amd import gen_pseudo_label_gaussian_process
    from gapro_amd._lib import Context
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch, predict_gp_batch
    from gapro_amd.gen_ps_utils import getInstanceInfo
    from gapro_amd.synth import make_scene

    sc = make_scene(seed=7, n_points=1_000_000, n_objects=40, with_walls_json=False, obj_patch=60, plane_patch=400)
    xyz = sc.aligned_xyz()
    _, cls, box, vol, _ = getInstanceInfo(xyz, sc.inst, sc.sem)
    kw = dict(coords_float=xyz, mask_feats=sc.default_feats().astype(np.float32), spp=sc.spp,
              instance_cls=cls.astype(np.int64), instance_box=box.astype(np.float32),
              instance_box_volume=vol.astype(np.float32), wall_box=[], wall_box_volume=[], instance_classes=13,
              ground_h=0.1, training_iter=50, thresh_spp_occu=0.999)
    plain = gen_pseudo_label_gaussian_process(**kw)
    full = gen_pseudo_label_gaussian_process(**kw, return_models=True)
    for a, b in zip(plain, full[:5]):
        assert torch.equal(a, b)
    extra = full[5]
    assert len(extra.fits) == 66
    lib = Context.get(0).lib
    routes = {int(lib.gapro_fit_route(f.model.m, 6)) for f in extra.fits}
    assert {0, 1, 3, 5} <= routes and (routes & {2, 4}), routes
    problems = [(f.train[:f.m1], f.train[f.m1:], f.test) for f in extra.fits]
    feats = extra.feats_spp
    fit_gp_spp_batch(feats, problems, training_iter=50, return_models=True)  # warm-up, same shapes
    t0 = time.perf_counter()
    outs, models = fit_gp_spp_batch(feats, problems, training_iter=50, return_models=True)
    t_fit = time.perf_counter() - t0
    rows = [p[2] for p in problems]
    predict_gp_batch(models, feats, rows)
    t0 = time.perf_counter()
    got = predict_gp_batch(models, feats, rows)
    t_pred = time.perf_counter() - t0
    print("66 fits: fit %.1f ms, predict at their own test sets %.1f ms" % (1e3 * t_fit, 1e3 * t_pred))
    for k, f in enumerate(extra.fits):
        assert np.array_equal(f.model.to_state(), models[k].to_state())  # the scene's models are the direct launch's
        assert np.isfinite(got[k][3]).all() and (got[k][4] > 0).all()
    assert t_pred < t_fit, (t_pred, t_fit)
