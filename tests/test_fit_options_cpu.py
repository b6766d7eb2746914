"""The case table of fit_option_cases.py really exercises what test_fit_options_gpu.py claims.  Oracle only, no device.

Under a min_variance clamp a kernel and the oracle must take the SAME branch for every training column at every Adam
step and for every test row, and two correct float64 implementations drift ~1e-9 apart over fifty steps.  So every
case must keep its unclamped variances away from the clamp value along the whole trajectory (conditions, not
tolerances: a case that misses one gets another seed or clamp value), while the clamp must be active often enough for
a wrong clamp branch or a missing zero of the variance gradient to show.  The routes are asserted with the library's
own route function, which needs no device either.
"""
import numpy as np
import pytest

import fit_option_cases as fc
from oracle import svgp_oracle as so


@pytest.mark.parametrize("case", fc.CASES, ids=fc.IDS)
def test_case_runs_on_the_route_it_names(case):
    from gapro_amd import _lib

    lib = _lib.load()
    m = case.m1 + case.m2
    assert lib.gapro_fit_route_flags(m, case.d, case.flags) == case.route
    mp = lib.gapro_fit_padded_m(m, case.d)
    if case.name.startswith("wave_d32"):
        assert mp <= 32  # the wave kernel's centred-product form of G_Z
    if case.name == "staged_d6":
        assert mp == 160
    if case.name == "cluster4_d6":
        assert mp == 512  # four workgroups; cluster1_d32 stays below, on one
    if case.name == "cluster1_d32":
        assert 192 < mp < 512
    assert {c.route for c in fc.CASES if c.d == 6} == {5, 3, 0, 1, 4}
    assert {c.route for c in fc.CASES if c.d == 32} == {5, 3, 0, 1, 2, 4}


def test_oracle_min_variance_keyword_defaults_to_the_module_global():
    """min_variance=None is the module's MIN_VARIANCE in every function that takes the keyword, and a value reaches the
    clamp: the prior variance s + jitter - 0 of an untrained model is ln 2 + 1e-4."""
    case = fc.BY_NAME["wave_d6"]
    X, y, Xt = fc.xy(case)
    for fit in (so.svgp_fit_predict_manual, so.svgp_fit_predict_autograd):
        a = fit(X, y, Xt, 2)
        b = fit(X, y, Xt, 2, min_variance=so.MIN_VARIANCE)
        for u, v in zip(a, b):
            np.testing.assert_array_equal(u, v)
        hi = fit(X, y, Xt, 0, min_variance=0.75)[1]
        np.testing.assert_array_equal(hi, np.full(len(Xt), 0.75))
    M = len(X)
    args = (Xt, X, np.zeros(M), np.eye(M), 0.0, 0.0, 0.0)
    np.testing.assert_array_equal(so.svgp_predict(*args)[1], so.svgp_predict(*args, min_variance=so.MIN_VARIANCE)[1])
    np.testing.assert_array_equal(so.svgp_predict(*args, min_variance=0.75)[1], np.full(len(Xt), 0.75))
    aux = {}
    l0, g0 = so.svgp_loss_and_grads(X, y, X, np.zeros(M), np.eye(M), 0.0, 0.0, 0.0)
    l1, g1 = so.svgp_loss_and_grads(X, y, X, np.zeros(M), np.eye(M), 0.0, 0.0, 0.0, min_variance=0.75, aux=aux)
    assert l0 != l1 and np.allclose(aux["var_raw"], np.log(2.0) + so.JITTER, rtol=1e-9, atol=0)
    assert g1["rho_s"] != g0["rho_s"]  # the clamped columns' variance gradient is gone


@pytest.mark.parametrize("case", fc.CASES, ids=fc.IDS)
def test_clamp_preconditions(case):
    v = case.v
    assert v in (0.3, 0.5, 0.6)
    X, y, Xt = fc.xy(case)
    steps = []
    with fc.few_threads():
        (mu_m, var_m, p_m), st_m = so.svgp_fit_predict_manual(X, y, Xt, fc.ITERS, return_trace=True, min_variance=v,
                                                              step_aux=steps)
    raw = np.array([s["var_raw"] for s in steps])  # [step, training column]
    assert raw.shape == (fc.ITERS, len(X))
    clamped = raw < v
    n_steps, frac, gap = int(clamped.any(axis=1).sum()), float(clamped.mean(axis=1).max()), float(np.abs(raw - v).min())
    (mu_a, var_a, p_a), st_a = fc.reference(case, min_variance=v)
    raw_t = fc.raw_variances(st_a, Xt)
    n_t, gap_t = int((raw_t < v).sum()), float(np.abs(raw_t - v).min())
    d_var = float(np.max(np.abs(var_m - var_a) / var_a))
    d_loss = abs(st_m["loss"][-1] - st_a["loss"][-1])
    d_z = float(np.abs(st_m["Z"] - st_a["Z"]).max())
    print("%s v %.1f M %d: %d steps clamp, up to %.0f %% of the columns, trajectory gap %.2e; test rows %d of %d "
          "clamped, gap %.2e; the two oracles: var %.1e  Z %.1e  loss %.1e"
          % (case.name, v, len(X), n_steps, 100 * frac, gap, n_t, len(raw_t), gap_t, d_var, d_z, d_loss))
    assert n_steps >= 10
    assert frac >= 0.25
    assert gap >= 1e-7
    assert 1 <= n_t < len(raw_t)
    assert gap_t >= 1e-5
    # the reference under the clamp is itself reproducible far below what the GPU test allows a route
    np.testing.assert_array_equal(var_a[raw_t < v], v)
    np.testing.assert_array_equal(var_m[raw_t < v], v)
    assert d_var <= 1e-7 and d_loss <= 1e-10


@pytest.mark.parametrize("case", [c for c in fc.CASES if c.name != "generic_d32"],
                         ids=[n for n in fc.IDS if n != "generic_d32"])
def test_d_ref_table_is_what_the_two_oracles_give(case):
    """fc.D_REF against a fresh measurement.  The GPU test's bound on a state field is max(1e-8, 100 x d_ref): the
    table must not be larger than what the two oracles give here by more than the factor ten by which their last-bit
    differences (another BLAS, another thread count) move the figure."""
    assert fc.D_REF["generic_d32"] == fc.D_REF["cluster1_d32"]  # one problem on two routes
    d = fc.state_deviation(fc.reference(case)[1], fc.reference(case, impl="manual")[1])
    print("%s d_ref: %s" % (case.name, "  ".join("%s %.1e" % (k, d[k]) for k in fc.STATE_FIELDS)))
    for k in fc.STATE_FIELDS:
        assert fc.state_bound(case, k) <= max(1e-8, 1000.0 * d[k]), (k, d[k], fc.D_REF[case.name][k])
        assert fc.state_bound(case, k) <= 1e-7, k  # float64 state: four orders below the float32 outputs' 1e-5 .. 2e-7


@pytest.mark.parametrize("case", [c for c in fc.CASES if c.d == 6 and c.m1 + c.m2 <= 150],
                         ids=[c.name for c in fc.CASES if c.d == 6 and c.m1 + c.m2 <= 150])
def test_the_two_oracles_agree_at_other_lr_and_jitter(case):
    """The reference of the lr / jitter tests is itself reproducible within 1e-7 in sigma^2, a hundredth of the 1e-5 the
    kernels are held to."""
    for lr, jitter in fc.LR_JITTER:
        a = fc.reference(case, lr=lr, jitter=jitter)[0]
        b = fc.reference(case, lr=lr, jitter=jitter, impl="manual")[0]
        np.testing.assert_allclose(b[1], a[1], rtol=1e-7, atol=0)
        np.testing.assert_allclose(b[0], a[0], rtol=1e-6, atol=1e-9)
    # and the options do something: the three settings and the default give different variances
    vs = [fc.reference(case, lr=lr, jitter=j)[0][1] for lr, j in fc.LR_JITTER] + [fc.reference(case)[0][1]]
    for i in range(len(vs)):
        for k in range(i):
            assert np.max(np.abs(vs[i] - vs[k]) / vs[k]) > 1e-3
