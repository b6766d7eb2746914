"""Every fit option and every per-fit output on every kernel route of the batched GP fit, against the float64 oracle.

The routes (gapro_fit_route: wave-per-fit 5, small-fit strip 3, 512-thread strip 0, LDS-staged 1, generic 2, cluster 4)
each carry their own likelihood epilogue, Adam step, psd-safe Cholesky and per-fit reductions; the other fit tests run
them at the default gapro_fit_options and read the five float32 per-row outputs.  Here, per case of
fit_option_cases.py (one per route and feature width; test_fit_options_cpu.py proves what the cases exercise):

  1. min_variance at a value that clamps during training and at prediction (the clamp and its zero variance gradient),
  2. the same clamp in the predict kernel, from models trained at the defaults,
  3. lr and jitter away from their defaults,
  4. the float64 per-fit outputs at the defaults: the final ELBO, the conditioning figure, the exported state,
  5. the amount the psd-safe Cholesky adds when it retries (psd_jitter 10^i, replacing),
  6. the validation of the options.

Options are set on the cached pipeline the fit functions use and restored afterwards.  Tolerances: the float32 outputs
by test_fit_gpu.py's _compare and test_predict_gpu.py's _check, unchanged; the loss 1e-9 absolute (test_svgp_kat.py);
cond rtol 1e-7 = eps x cond_2 <= 2.2e-16 M s / jitter ~ 8e-10 at M = 512, times 100 for the blocked factorisation; a
state field max(1e-8, 100 x d_ref), d_ref the discrepancy of the two oracle implementations in that field
(fit_option_cases.D_REF), 100 the headroom the project gives a third summation order elsewhere.
"""
import contextlib

import numpy as np
import pytest

import fit_option_cases as fc
from test_fit_gpu import _compare
from test_predict_gpu import _check

pytestmark = pytest.mark.gpu

PREDICT_V = (0.15, 0.3, 0.5, 0.6)


def _pipe(iters=fc.ITERS):
    import torch
    from gapro_amd.gen_ps_utils import _pipeline

    return _pipeline(torch.device("cuda", 0), iters)


@contextlib.contextmanager
def _options(pipe, flags=0, **kw):
    """gapro_fit_options fields of a cached pipeline for the duration of a block (flags are ORed into reserved)."""
    old = {k: getattr(pipe.opt, k) for k in kw}
    old["reserved"] = int(pipe.opt.reserved)
    try:
        for k, v in kw.items():
            setattr(pipe.opt, k, v)
        pipe.opt.reserved = old["reserved"] | flags
        yield pipe
    finally:
        for k, v in old.items():
            setattr(pipe.opt, k, v)


def _assert_route(case, flags=None):
    from gapro_amd import _lib

    flags = case.flags if flags is None else flags
    assert _lib.load().gapro_fit_route_flags(case.m1 + case.m2, case.d, flags) == case.route, case.name


def _fit(case, iters=fc.ITERS, **opts):
    """One launch of the case's problem on the case's route: (5-tuple of outputs, GPModel, result dict)."""
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch

    _assert_route(case)
    feats, b1, b2, it = fc.problem(case)
    with _options(_pipe(iters), flags=case.flags, **opts):
        outs, models, res = fit_gp_spp_batch(feats, [(b1, b2, it)], training_iter=iters, keep_debug=True,
                                             return_models=True)
    assert res["status"][0] == 0
    return outs[0], models[0], res


# ------------------------------------------------------------------------------------------ 1. the clamp, in the fit
@pytest.mark.parametrize("case", fc.CASES, ids=fc.IDS)
def test_min_variance_clamp_in_the_fit(case):
    v = case.v
    out, model, res = _fit(case, min_variance=v)
    ref, st = fc.reference(case, min_variance=v)
    raw = fc.raw_variances(st, fc.xy(case)[2])
    clamped = raw < v
    d_loss = abs(float(res["loss"][0]) - st["loss"][-1])
    var = out[4]
    print("%s min_variance %.1f: %d of %d test rows clamped; var rel %.2e  mu abs %.2e  p abs %.2e  loss abs %.2e"
          % (case.name, v, clamped.sum(), len(raw), np.max(np.abs(var - ref[1]) / ref[1]), np.max(np.abs(out[3] - ref[0])),
             np.max(np.abs(out[0] - ref[2])), d_loss))
    assert clamped.any() and not clamped.all()
    _compare(out, ref)
    np.testing.assert_array_equal(var[clamped], np.float32(v))
    assert (var[~clamped] > np.float32(v)).all()
    assert d_loss < 1e-9


# ------------------------------------------------------------------------- 4. loss, cond and state at the defaults
@pytest.fixture(scope="module")
def trained():
    """Every case trained at the default options: the cases of a feature width in one launch (the generic kernel's
    case, which needs its debug bit, in one of its own).  name -> (outputs, GPModel, loss, cond)."""
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch

    out = {}
    groups = [[c for c in fc.CASES if c.d == 6], [c for c in fc.CASES if c.d == 32 and c.flags == 0],
              [c for c in fc.CASES if c.flags != 0]]
    for group in groups:
        flags = group[0].flags
        parts, probs, base = [], [], 0
        for c in group:
            _assert_route(c, flags)
            f, b1, b2, it = fc.problem(c)
            parts.append(f)
            probs.append((b1 + base, b2 + base, it + base))
            base += len(f)
        with _options(_pipe(), flags=flags):
            outs, models, res = fit_gp_spp_batch(np.concatenate(parts), probs, training_iter=fc.ITERS, keep_debug=True,
                                                 return_models=True)
        assert (res["status"] == 0).all()
        for k, c in enumerate(group):
            out[c.name] = (outs[k], models[k], float(res["loss"][k]), float(res["cond"][k]))
    return out


@pytest.mark.parametrize("case", fc.CASES, ids=fc.IDS)
def test_loss_cond_and_state_at_the_defaults(case, trained):
    out, model, loss, cond = trained[case.name]
    ref, st = fc.reference(case)
    _compare(out, ref)
    d_loss = abs(loss - st["loss"][-1])
    want_cond = fc.cond_figure(fc.kzz(model.Z, model.rho_s, model.rho_l), model.jitter)
    dev = fc.state_deviation(model, st)
    print("%s route %d M %d: loss abs %.2e  cond %.6e rel %.2e  state %s"
          % (case.name, case.route, model.m, d_loss, cond, abs(cond - want_cond) / want_cond,
             "  ".join("%s %.1e (<= %.1e)" % (k, dev[k], fc.state_bound(case, k)) for k in fc.STATE_FIELDS)))
    assert d_loss < 1e-9
    assert model.jitter == 1e-4 and model.status == 0
    np.testing.assert_allclose(cond, want_cond, rtol=1e-7, atol=0)
    for k in fc.STATE_FIELDS:
        assert dev[k] <= fc.state_bound(case, k), (case.name, k, dev[k], fc.state_bound(case, k))


# ------------------------------------------------------------------------- 2. the clamp, in the predict kernel
def _predict_tables(trained):
    """Per feature width: (cases, models, feature table, one row vector per model): every model at its own inducing
    points (rounded to float32, as a feature table holds them) and at 2000 unseen rows of its problem."""
    from gapro_amd.synth import make_gp_problem

    for d in (6, 32):
        cases = [c for c in fc.CASES if c.d == d]
        models = [trained[c.name][1] for c in cases]
        tables = []
        for c, mo in zip(cases, models):
            unseen = make_gp_problem(1000 + c.m1, c.m1, c.m2, 2000, d, std=fc.std_of(d))[0][c.m1 + c.m2:]
            tables.append(np.concatenate([mo.Z.astype(np.float32), unseen]))
        base = np.cumsum([0] + [len(t) for t in tables])
        yield cases, models, np.concatenate(tables), [np.arange(base[k], base[k + 1]) for k in range(len(tables))], tables


def _predict_ref(model, X, min_variance):
    from oracle import svgp_oracle as so

    return so.svgp_predict(X.astype(np.float64), model.Z, model.mean, model.LS, model.c, model.rho_s, model.rho_l,
                           jitter=model.jitter, min_variance=min_variance)


def test_min_variance_clamp_in_the_predict_kernel(trained):
    from gapro_amd.gaussian_process_utils import predict_gp_batch

    both = set()
    for cases, models, feats, rows, tables in _predict_tables(trained):
        raws = [_predict_ref(mo, t, -np.inf)[1] for mo, t in zip(models, tables)]
        for v in PREDICT_V:
            with _options(_pipe(), min_variance=v):
                got = predict_gp_batch(models, feats, rows)
            for k, c in enumerate(cases):
                raw = raws[k]
                keep = np.abs(raw - v) > 1e-9 * v  # a row this close to the threshold may take either branch
                assert (~keep).mean() <= 1e-3
                clamped = raw[keep] < v
                ref = _predict_ref(models[k], tables[k][keep], v)
                out = tuple(o[keep] for o in got[k])
                _check(out, ref, "%s min_variance %.2f: %d of %d rows clamped" % (c.name, v, clamped.sum(), keep.sum()))
                np.testing.assert_array_equal(out[4][clamped], np.float32(v))
                assert (out[4][~clamped] >= np.float32(v)).all()  # (a raw variance 1e-8 above v rounds to float32(v))
                assert clamped.any() or v < 0.3  # (0.15 is there for the unclamped rows of the models with a small s)
                if not clamped.all():
                    both.add(c.name)
    assert both == set(fc.IDS), both  # every model met both branches at some value


def test_predict_at_the_default_min_variance_clamps_nothing(trained):
    from gapro_amd.gaussian_process_utils import predict_gp_batch

    for cases, models, feats, rows, tables in _predict_tables(trained):
        base = predict_gp_batch(models, feats, rows)
        assert _pipe().opt.min_variance == 1e-6
        with _options(_pipe(), min_variance=1e-6):
            same = predict_gp_batch(models, feats, rows)
        with _options(_pipe(), min_variance=0.0):
            none = predict_gp_batch(models, feats, rows)
        for k, c in enumerate(cases):
            assert (_predict_ref(models[k], tables[k], -np.inf)[1] > 1e-4).all()
            assert (base[k][4] > np.float32(1e-4)).all()
            for a, b, z in zip(base[k], same[k], none[k]):
                np.testing.assert_array_equal(a, b)
                np.testing.assert_array_equal(a, z)


# ------------------------------------------------------------------------------------------ 3. lr and jitter
@pytest.mark.parametrize("lr,jitter", fc.LR_JITTER)
@pytest.mark.parametrize("case", fc.CASES, ids=fc.IDS)
def test_lr_and_jitter(case, lr, jitter):
    out, model, res = _fit(case, lr=lr, jitter=jitter)
    ref, st = fc.reference(case, lr=lr, jitter=jitter)
    print("%s lr %g jitter %g: var rel %.2e  mu abs %.2e  p abs %.2e  loss abs %.2e"
          % (case.name, lr, jitter, np.max(np.abs(out[4] - ref[1]) / ref[1]), np.max(np.abs(out[3] - ref[0])),
             np.max(np.abs(out[0] - ref[2])), abs(float(res["loss"][0]) - st["loss"][-1])))
    _compare(out, ref)
    assert model.jitter == jitter


# ------------------------------------------------------------------------------------------ 5. the retry amount
def _with_duplicates(case, variation):
    """The case's shape with exact duplicates among its training rows (five copies of a point of side 1, three of a
    point of side 2, and so on: one group per 16 rows) and six test rows."""
    from gapro_amd.synth import make_gp_problem

    feats, b1, b2, it = make_gp_problem(3300 + variation, case.m1, case.m2, 6, case.d, std=fc.std_of(case.d))
    feats = feats.copy()
    for g in range(max(2, (case.m1 + case.m2) // 16)):
        side, copies = (b1, 4) if g % 2 == 0 else (b2, 2)
        first = 8 * (g // 2)
        if first + copies < len(side):
            for k in range(1, copies + 1):
                feats[side[first + k]] = feats[side[first]]
    return feats, b1, b2, it


@pytest.mark.parametrize("name", ["wave_d6", "small_d6", "strip_d6", "staged_d6", "generic_d32", "cluster4_d6"])
def test_psd_retry_adds_psd_jitter_times_ten_to_the_attempt(name):
    """K_ZZ with duplicated inducing points and no variational jitter is singular; at zero training steps the only
    factorisation is the prediction's.  Variations are tried (24 at most) until one fails without retries; with
    retries the first attempt adds psd_jitter, and the duplicates' pivots are then psd_jitter-sized, so the
    conditioning figure of the factor says how much the route really added."""
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch
    from gapro_amd.synth import make_gp_problem

    case = fc.BY_NAME[name]
    _assert_route(case)
    f2, c1, c2, ct = make_gp_problem(34, 20, 25, 4, case.d, std=fc.std_of(case.d))
    pipe = _pipe(0)
    found = None
    for variation in range(24):
        feats, b1, b2, it = _with_duplicates(case, variation)
        allf = np.concatenate([feats, f2])
        off = len(feats)
        launch = [(b1, b2, it), (c1 + off, c2 + off, ct + off)]
        with _options(pipe, flags=case.flags, jitter=0.0, psd_retries=0):
            outs0, res0, status0 = fit_gp_spp_batch(allf, launch, training_iter=0, keep_debug=True, return_status=True)
        assert status0[1] == 0
        if status0[0] == 0:
            continue  # every pivot of this variation happened to round to a positive number
        assert status0[0] == -5
        found = variation
        break
    assert found is not None, "no variation produced a non-positive pivot"
    K = fc.kzz(np.concatenate([feats[b1], feats[b2]]), 0.0, 0.0)
    for psd_jitter, rtol in ((1e-8, 1e-5), (1e-3, 1e-7)):
        with _options(pipe, flags=case.flags, jitter=0.0, psd_retries=3, psd_jitter=psd_jitter):
            outs, res, status = fit_gp_spp_batch(allf, launch, training_iter=0, keep_debug=True, return_status=True)
        assert (status == 0).all()
        for a, b in zip(outs0[1], outs[1]):
            np.testing.assert_array_equal(a, b)
        assert res["cond"][1] == res0["cond"][1]
        want = fc.cond_figure(K, psd_jitter)
        print("%s variation %d psd_jitter %g: cond %.9e, NumPy %.9e, rel %.2e; with ten times the amount %.3e"
              % (name, found, psd_jitter, res["cond"][0], want, abs(res["cond"][0] - want) / want,
                 fc.cond_figure(K, 10 * psd_jitter)))
        np.testing.assert_allclose(res["cond"][0], want, rtol=rtol, atol=0)
        assert np.isfinite(outs[0][3]).all() and (outs[0][0] == np.float32(0.5)).all()  # untrained: the prior


# ------------------------------------------------------------------------------------------ 6. option validation
BAD_OPTIONS = [dict(lr=0.0), dict(lr=float("nan")), dict(jitter=-1e-4), dict(psd_retries=9), dict(psd_jitter=-1.0),
               dict(min_variance=float("nan")), dict(min_variance=-1.0), dict(min_variance=float("inf"))]


@pytest.mark.parametrize("bad", BAD_OPTIONS, ids=["%s=%s" % kv for b in BAD_OPTIONS for kv in b.items()])
def test_fit_refuses_bad_options(bad):
    from gapro_amd._lib import GaproError
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch

    case = fc.BY_NAME["wave_d6"]
    feats, b1, b2, it = fc.problem(case)
    with _options(_pipe(), **bad):
        with pytest.raises(GaproError) as e:
            fit_gp_spp_batch(feats, [(b1, b2, it)], training_iter=fc.ITERS)
    assert e.value.code == -1
    if "min_variance" in bad:
        assert "min_variance" in str(e.value)
    _compare(fit_gp_spp_batch(feats, [(b1, b2, it)], training_iter=fc.ITERS)[0], fc.reference(case)[0])


@pytest.mark.parametrize("bad", [float("nan"), -1.0, float("inf")])
def test_predict_refuses_a_bad_min_variance(bad, trained):
    from gapro_amd._lib import GaproError
    from gapro_amd.gaussian_process_utils import predict_gp_batch

    case = fc.BY_NAME["wave_d6"]
    out, model, _, _ = trained[case.name]
    feats, b1, b2, it = fc.problem(case)
    with _options(_pipe(), min_variance=bad):
        with pytest.raises(GaproError) as e:
            predict_gp_batch([model], feats, [it])
    assert e.value.code == -1 and "min_variance" in str(e.value)
    again = predict_gp_batch([model], feats, [it])[0]
    _check(again, (out[3].astype(np.float64), out[4].astype(np.float64), out[0].astype(np.float64)), "after a refusal")


# ------------------------------------------------------------------ 7. the launch structure the library plans is issued
def test_every_timing_class_of_the_plan_is_issued_and_no_other():
    """One fit per route in one launch (test_fit_plan_cpu.ROUTE_M, two Adam steps): the timing marks the launch loop
    records are those of the classes in gapro_fit_launch_plan's steps for the same batch -- FitTiming.read() is positive
    for exactly these -- and every fit ends with status 0."""
    import torch
    from gapro_amd import _lib
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch
    from gapro_amd.synth import make_gp_problem
    from test_fit_plan_cpu import ROUTE_M, plan

    rc, steps, _ = plan(ROUTE_M, n_cu=torch.cuda.get_device_properties(0).multi_processor_count)
    assert rc == 0
    planned = {s[7] for s in steps}
    assert planned == {0, 1, 2, 3, 4}
    parts, probs, base = [], [], 0
    for i, m in enumerate(ROUTE_M):
        f, b1, b2, it = make_gp_problem(700 + i, m // 2, m - m // 2, 3 + i, 6)
        parts.append(f)
        probs.append((b1 + base, b2 + base, it + base))
        base += len(f)
    pipe = _pipe(2)
    pipe.profile_fit, pipe.fit_events = True, []
    try:
        _, status = fit_gp_spp_batch(np.concatenate(parts), probs, training_iter=2, return_status=True)
        assert len(pipe.fit_events) == 1
        ms = pipe.fit_events[0].read()
    finally:
        pipe.profile_fit, pipe.fit_events = False, []
    assert (np.asarray(status) == 0).all()
    by_class = {0: ms[0], 1: ms[1], 2: ms[3], 3: ms[4], 4: ms[5]}  # staged, strip, small, cluster, wave
    print("timing classes: %s" % by_class)
    assert {c for c, v in by_class.items() if v > 0} == planned
    assert ms[2] > 0
