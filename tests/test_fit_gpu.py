"""HIP batched SVGP fit vs the float64 oracle.  Tolerance: north_star asks GP variances within 1e-4
relative; the float64 kernel is held to 1e-6 (it typically agrees to ~1e-9), labels bit-exact."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VAR_RTOL = 1e-5  # << the 1e-4 of BASELINE.json's north_star (typical agreement: 5e-8 = float32 output rounding)
MU_ATOL = 1e-7


def test_mfma_f64_lane_maps():
    import torch
    from gapro_amd._lib import Context

    ctx = Context.get(0)
    rng = np.random.default_rng(0)
    K = 24
    P = rng.integers(-4, 5, size=(K, 16)).astype(np.float64)
    Q = rng.integers(-4, 5, size=(K, 16)).astype(np.float64)  # asymmetric: catches a transposed C map
    dP, dQ = torch.from_numpy(P).cuda(), torch.from_numpy(Q).cuda()
    dC = torch.zeros((16, 16), dtype=torch.float64, device="cuda")
    ctx.check(ctx.dbg.gapro_debug_mfma_tn(ctx.handle, None, C.c_void_p(dP.data_ptr()), C.c_void_p(dQ.data_ptr()),
                                           C.c_void_p(dC.data_ptr()), K))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dC.cpu().numpy(), P.T @ Q)


def test_fit_kernels_special_functions_against_scipy():
    """erfcx_tab / exp_neg / the Mills-ratio forms of csrc/fit_math.h (a 1.3 KB table and a short polynomial instead of
    the math library's erfcx and exp) against SciPy in float64: a few ulp, over the ranges the likelihood and the RBF
    kernel reach and far beyond them."""
    import torch
    from scipy import special as sp

    from gapro_amd._lib import Context

    ctx = Context.get(0)
    rng = np.random.default_rng(5)

    def run(x, which):
        dx = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()
        do = torch.empty_like(dx)
        ctx.check(ctx.dbg.gapro_debug_fit_math(ctx.handle, None, dx.numel(), C.c_void_p(dx.data_ptr()),
                                                C.c_void_p(do.data_ptr()), which))
        torch.cuda.synchronize()
        return do.cpu().numpy()

    def ulps(got, ref):
        return np.abs(got - ref) / np.spacing(np.abs(ref))

    x = np.concatenate([rng.uniform(0, 12, 200000), 10.0 ** rng.uniform(-300, 300, 20000), [0.0, 0.5, 1.0, 26.0, 1e308]])
    assert np.allclose(run(x, 0), sp.erfcx(x), rtol=1.2e-15, atol=0)  # (SciPy's own error is up to ~4 ulp near 0)
    assert run(np.array([np.inf]), 0)[0] == 0.0 and np.isnan(run(np.array([np.nan]), 0)[0])
    x = -np.concatenate([rng.uniform(0, 60, 200000), 10.0 ** rng.uniform(-300, 2.84, 20000), [0.0, 700.0, 708.0]])
    assert ulps(run(x, 1), np.exp(x)).max() <= 2
    assert run(np.array([-800.0, -1e300]), 1).max() <= 5e-324 and np.isnan(run(np.array([np.nan]), 1)[0])
    # r(z) = phi(z) / Phi(z) and log Phi(z) over both tails (reference: erfcx / log_ndtr, each good to an ulp or two)
    z = np.concatenate([rng.uniform(-40, 12, 200000), [-1e3, -37.5, -1e-9, 0.0, 1e-9, 8.0, 30.0]])
    with np.errstate(all="ignore"):  # both branches are evaluated everywhere
        ref_r = np.where(z < 0, np.sqrt(2 / np.pi) / sp.erfcx(-z / np.sqrt(2)),
                         np.exp(-0.5 * z * z) / np.sqrt(2 * np.pi) / sp.ndtr(z))
    for which in (2, 4):
        got = run(z, which)
        assert np.allclose(got, ref_r, rtol=4e-15, atol=0), np.abs(got / ref_r - 1).max()
    assert np.array_equal(run(z, 2), run(z, 4))  # the ratio-only form gives the bits of the form with the logarithm
    got = run(z, 3)
    assert np.allclose(got, sp.log_ndtr(z), rtol=4e-15, atol=3e-16), np.abs(got - sp.log_ndtr(z)).max()


def _oracle(feats, b1, b2, it, iters, init_mean=None):
    from oracle import svgp_oracle as so

    X = np.concatenate([feats[b1], feats[b2]]).astype(np.float64)
    y = np.r_[-np.ones(len(b1)), np.ones(len(b2))]
    Xt = feats[it].astype(np.float64)
    # torch autograd float64 is the reference (gradients right by construction); on tiny problems the
    # NumPy restatement itself drifts ~1e-6 from it while the kernel stays at float32 output rounding
    return so.svgp_fit_predict_autograd(X, y, Xt, iters, "f64", init_mean=init_mean)


def _compare(out, ref):
    probs, probs_new, labels, mu, var = out
    mu_r, var_r, p_r = ref
    assert probs.dtype == np.float32 and mu.dtype == np.float32 and var.dtype == np.float32 and labels.dtype == bool
    np.testing.assert_allclose(var, var_r, rtol=VAR_RTOL)
    np.testing.assert_allclose(mu, mu_r, rtol=1e-5, atol=MU_ATOL)
    np.testing.assert_allclose(probs, p_r, rtol=0, atol=2e-7)
    p32 = p_r.astype(np.float32)
    safe = np.abs(p_r - 0.5) > 1e-6  # a label can only differ when p sits within float32 rounding of 0.5
    np.testing.assert_array_equal(labels[safe], (p32 >= np.float32(0.5))[safe])
    np.testing.assert_array_equal(probs_new, np.where(labels, probs, np.float32(1) - probs))


@pytest.mark.parametrize("m1,m2,t,d", [(1, 2, 1, 6), (3, 4, 5, 6), (20, 30, 10, 6), (16, 16, 32, 6), (40, 60, 33, 6),
                                       (70, 80, 100, 6), (10, 12, 75, 32), (120, 136, 40, 6), (10, 13, 33, 6),
                                       (20, 25, 40, 6), (2, 46, 17, 6)])
@pytest.mark.parametrize("iters", [0, 3, 50])
def test_fit_matches_oracle(m1, m2, t, d, iters):
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch
    from gapro_amd.synth import make_gp_problem

    if m1 + m2 > 200 and iters == 3:
        pytest.skip("covered by 0 and 50")
    # d = 32 at unit std is a rounding-noise-driven problem (see make_gp_problem); scale it
    feats, b1, b2, it = make_gp_problem(7 + m1, m1, m2, t, d, std=0.3 if d > 8 else 1.0)
    out = fit_gp_spp_batch(feats, [(b1, b2, it)], training_iter=iters)[0]
    _compare(out, _oracle(feats, b1, b2, it, iters))


@pytest.mark.parametrize("m1,m2,t,iters,route", [(150, 170, 60, 50, 1), (200, 210, 90, 50, 1), (230, 245, 40, 50, 1),
                                                  (250, 262, 30, 50, 4), (260, 270, 90, 50, 4), (340, 360, 50, 50, 4),
                                                  (260, 270, 90, 5, 2)])
def test_fit_large_inducing_sets(m1, m2, t, iters, route):
    """BASELINE configs[3] territory (large overlap regions): M_p = 320, 416 and 480 run the LDS-staged kernel on one CU
    (32 x 32 wave tiles at 320; 64 x 64 from 352 on, with a last row / column of 32 x 32 tiles at M_p = 416 and 480);
    from M_p >= 512 on a fit is spread over 4, 8, ... workgroups by the cluster kernel (route 4), checked against the
    float64 oracle at the full 50 Adam steps; route 2 = the same fit kept on one workgroup in the generic kernel (debug
    bit 3 of gapro_fit_options.reserved)."""
    import torch
    from gapro_amd import _lib
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch
    from gapro_amd.gen_ps_utils import _pipeline
    from gapro_amd.synth import make_gp_problem

    want = route if route != 2 else 4
    assert _lib.load().gapro_fit_route(m1 + m2, 6) == want
    feats, b1, b2, it = make_gp_problem(40 + m1, m1, m2, t, 6)
    pipe = _pipeline(torch.device("cuda", 0), iters)
    old = pipe.opt.reserved
    if route == 2:
        pipe.opt.reserved = old | 8
    try:
        out = fit_gp_spp_batch(feats, [(b1, b2, it)], training_iter=iters)[0]
    finally:
        pipe.opt.reserved = old
    _compare(out, _oracle(feats, b1, b2, it, iters))


def test_cluster_kernel_is_deterministic_and_independent_of_its_neighbours():
    """A fit spread over several workgroups must not depend on what runs beside it or on where its workgroups land:
    the same problem alone, twice in one launch among other cluster fits of different sizes, and in a second launch
    gives bit-identical outputs (ordered two-stage sums; the cluster size is a function of M only)."""
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch
    from gapro_amd.synth import make_gp_problem

    parts, probs, base = [], [], 0
    for i, (m1, m2, t) in enumerate([(200, 215, 40), (250, 300, 10), (330, 330, 25), (30, 40, 5), (100, 90, 7)]):
        f, b1, b2, it = make_gp_problem(800 + i, m1, m2, t, 6)
        parts.append(f)
        probs.append((b1 + base, b2 + base, it + base))
        base += len(f)
    feats = np.concatenate(parts)
    launch = [probs[0], probs[1], probs[2], probs[3], probs[0], probs[4], probs[1]]
    a = fit_gp_spp_batch(feats, launch, training_iter=12)
    b = fit_gp_spp_batch(feats, launch[::-1], training_iter=12)[::-1]
    alone = fit_gp_spp_batch(feats, [probs[0]], training_iter=12)[0]
    for x, y in zip(a, b):
        for u, v in zip(x, y):
            np.testing.assert_array_equal(u, v)
    for k in (0, 4):
        for u, v in zip(a[k], alone):
            np.testing.assert_array_equal(u, v)
    for u, v in zip(a[1], a[6]):
        np.testing.assert_array_equal(u, v)


def test_fit_stress_32_concurrent_large_regions():
    """BASELINE configs[4] shape: 32 concurrent regions of ~50k points each, i.e. ~1000 inducing and ~1000
    undetermined superpoints per fit (cluster kernel, ~140 MB of workspace per fit, 1024 workgroups in the launch: four
    times the chip, so clusters also wait for each other's CUs).  Four distinct problems, each eight times in the
    launch: the copies must agree bit for bit whatever ran beside them, and one problem of the full 50-step launch is
    checked against the float64 oracle."""
    from gapro_amd import _lib
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch
    from gapro_amd.synth import make_gp_problem

    m1, m2, t = 500, 524, 1000
    assert _lib.load().gapro_fit_route(m1 + m2, 6) == 4  # cluster kernel: every fit over 32 workgroups
    feats_list, probs, base = [], [], 0
    for i in range(4):
        f, b1, b2, it = make_gp_problem(900 + i, m1, m2, t, 6)
        feats_list.append(f)
        probs.append((b1 + base, b2 + base, it + base))
        base += len(f)
    feats = np.concatenate(feats_list)
    launch = [probs[i % 4] for i in range(32)]
    full = fit_gp_spp_batch(feats, launch, training_iter=50)
    b1, b2, it = probs[0]
    _compare(full[0], _oracle(feats, b1, b2, it, 50))
    for i, (probs_, probs_new, labels, mu, var) in enumerate(full):
        assert np.isfinite(mu).all() and np.isfinite(var).all() and (var > 0).all()
        assert ((probs_ >= 0) & (probs_ <= 1)).all() and (probs_new >= 0.5).all()
        for a, b in zip(full[i], full[i % 4]):
            np.testing.assert_array_equal(a, b)


def test_fit_ill_conditioned_problems_stay_finite():
    """Perfectly symmetric (1 vs 1) or far-apart (d = 32, unit std) problems have gradients that are pure
    rounding noise, which Adam normalises to full steps: implementations legitimately differ there
    (oracle autograd vs oracle manual differ by 1e-2), so only sanity is asserted."""
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch
    from gapro_amd.synth import make_gp_problem

    for (m1, m2, t, d) in [(1, 1, 1, 6), (10, 12, 75, 32)]:
        feats, b1, b2, it = make_gp_problem(7 + m1, m1, m2, t, d)
        probs, probs_new, labels, mu, var = fit_gp_spp_batch(feats, [(b1, b2, it)], training_iter=50)[0]
        assert np.isfinite(mu).all() and np.isfinite(var).all() and (var > 0).all()
        assert ((probs >= 0) & (probs <= 1)).all() and (probs_new >= 0.5).all()


@pytest.mark.parametrize("m1,m2,t", [(70, 74, 20), (80, 88, 33), (100, 100, 40), (130, 135, 25), (148, 152, 30),
                                     (165, 165, 17)])
def test_fit_matches_oracle_where_m_p_is_an_odd_multiple_of_16(m1, m2, t):
    """Round 3: M_p goes in steps of 16 up to 336 (gapro_pad_m) and the staged kernel's 32 x 32 wave tiles take a last
    row / column of 16 x 16 tiles there (gemm_tn's half-tile extents): M_p = 144, 176, 208 with the copy-free product
    forms, 272, 304, 336 with the k-major ones; 50 Adam steps against the float64 oracle."""
    from gapro_amd import _lib
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch
    from gapro_amd.synth import make_gp_problem

    lay = (C.c_int64 * 8)()
    _lib.load().gapro_fit_workspace_layout(m1 + m2, t, 6, C.cast(lay, C.c_void_p))
    mp = (m1 + m2 + 15) // 16 * 16
    assert mp % 32 == 16 and int(lay[0]) == mp, (mp, list(lay))  # the layout's padded size is the odd multiple
    feats, b1, b2, it = make_gp_problem(300 + m1, m1, m2, t, 6)
    out = fit_gp_spp_batch(feats, [(b1, b2, it)], training_iter=50)[0]
    _compare(out, _oracle(feats, b1, b2, it, 50))


@pytest.mark.parametrize("d", [32, 40])
@pytest.mark.parametrize("m1,m2,t", [(130, 135, 21), (150, 150, 30), (160, 170, 12)])
def test_wide_features_where_round_3_padded_to_an_odd_multiple_of_16(m1, m2, t, d):
    """M = 265 / 300 / 330.  At D = 32 these fit neither LDS kernel, are padded to a multiple of 32
    (gapro_pad_m is a function of (M, D)) and run on the cluster kernel; at D = 40 they run on the generic kernel, padded
    to 32 as well (and its 32 x 32 tiles are only used where M_p is a multiple of 32).  Round 3 sent both to the generic kernel with M_p = 272 /
    304 / 336 and left the last 16 rows and columns of every product uncomputed."""
    from gapro_amd import _lib
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch
    from gapro_amd.synth import make_gp_problem

    lib = _lib.load()
    m = m1 + m2
    assert lib.gapro_fit_route(m, d) == (4 if d == 32 else 2)
    mp = lib.gapro_fit_padded_m(m, d)
    assert mp % 32 == 0 and mp >= m
    feats, b1, b2, it = make_gp_problem(900 + m1, m1, m2, t, d, std=0.3)
    out = fit_gp_spp_batch(feats, [(b1, b2, it)], training_iter=50)[0]
    _compare(out, _oracle(feats, b1, b2, it, 50))


def test_two_per_cu_build_has_the_bits_of_the_one_per_cu_build():
    """The staged kernel has one instantiation per register budget and product form (k_svgp_fit<WPS, KMIN>); a launch
    with more fits than CUs runs its M_p <= 256 fits two per CU in the 128-VGPR build, a smaller one in the 256-VGPR
    build.  The product forms are a function of M_p alone, so the same fit has the same bits in both -- M_p = 160
    (whole 32 x 32 tiles), 208 (edge tiles), 256 (workgroup-tiled products)."""
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch
    from gapro_amd.synth import make_gp_problem

    feats_list, probs = [], []
    base = 0
    for i, (m1, m2, t) in enumerate([(75, 80, 9), (100, 104, 12), (125, 128, 7)]):
        f, b1, b2, it = make_gp_problem(500 + i, m1, m2, t, 6)
        feats_list.append(f)
        probs.append((b1 + base, b2 + base, it + base))
        base += len(f)
    feats = np.concatenate(feats_list)
    singles = [fit_gp_spp_batch(feats, [p], training_iter=8)[0] for p in probs]
    many = fit_gp_spp_batch(feats, probs * 100, training_iter=8)  # 300 fits on 256 CUs: the two-per-CU launch
    for k in (0, 1, 2, 150, 151, 152, 297, 298, 299):
        for a, b in zip(many[k], singles[k % 3]):
            np.testing.assert_array_equal(a, b)


def test_fit_batch_equals_single_and_is_deterministic():
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch
    from gapro_amd.synth import make_gp_problem

    feats_list, probs = [], []
    base = 0
    for i, (m1, m2, t) in enumerate([(5, 9, 3), (33, 20, 17), (64, 64, 64), (2, 40, 1), (80, 90, 20)]):
        f, b1, b2, it = make_gp_problem(100 + i, m1, m2, t, 6)
        feats_list.append(f)
        probs.append((b1 + base, b2 + base, it + base))
        base += len(f)
    feats = np.concatenate(feats_list)
    batch = fit_gp_spp_batch(feats, probs, training_iter=20)
    again = fit_gp_spp_batch(feats, probs[::-1], training_iter=20)[::-1]
    for i, p in enumerate(probs):
        single = fit_gp_spp_batch(feats, [p], training_iter=20)[0]
        for a, b, c in zip(batch[i], single, again[i]):
            np.testing.assert_array_equal(a, b)  # bitwise: a fit does not depend on its batch
            np.testing.assert_array_equal(a, c)


def test_fit_with_supplied_initial_mean_and_api_shapes():
    import torch
    from gapro_amd.gaussian_process_utils import fit_gp_spp
    from gapro_amd.synth import make_gp_problem

    feats, b1, b2, it = make_gp_problem(11, 14, 18, 9, 6)
    rng = np.random.default_rng(5)
    im = 1e-3 * rng.standard_normal(32)  # what gpytorch draws unseeded
    f = torch.from_numpy(feats).cuda()
    out = fit_gp_spp(None, f, torch.from_numpy(b1).cuda(), torch.from_numpy(b2).cuda(), torch.from_numpy(it).cuda(),
                     training_iter=50, init_mean=im)
    assert all(o.is_cuda for o in out) and out[2].dtype == torch.bool and out[0].shape == (9,)
    ref = _oracle(feats, b1, b2, it, 50, init_mean=im)
    _compare(tuple(o.cpu().numpy() for o in out), ref)
    zero = fit_gp_spp(None, f, b1, b2, it, training_iter=50)
    assert not np.allclose(zero[3].cpu().numpy(), out[3].cpu().numpy(), rtol=1e-6, atol=0)


def test_stale_cholesky_switch_matches_oracle():
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch
    from gapro_amd.synth import make_gp_problem
    from oracle import svgp_oracle as so

    feats, b1, b2, it = make_gp_problem(21, 12, 10, 8, 6)
    out = fit_gp_spp_batch(feats, [(b1, b2, it)], training_iter=10, eval_stale_chol=True)[0]
    X = np.concatenate([feats[b1], feats[b2]]).astype(np.float64)
    y = np.r_[-np.ones(12), np.ones(10)]
    ref = so.svgp_fit_predict_autograd(X, y, feats[it].astype(np.float64), 10, "f64", eval_chol="stale")
    _compare(out, ref)


@pytest.mark.parametrize("m1,m2,t,route", [(180, 190, 21, 1), (260, 275, 17, 4)])
def test_stale_cholesky_and_initial_mean_on_the_large_fit_kernels(m1, m2, t, route):
    """The reference's two unverifiable knobs (prediction with the last training step's Cholesky factor;
    the 1e-3 randn initial variational mean) on the staged kernel's 64 x 64-tile path (M_p = 384) and on the cluster
    kernel (M_p = 544 over 4 workgroups), against the oracle with the same switches."""
    from gapro_amd import _lib
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch
    from gapro_amd.synth import make_gp_problem
    from oracle import svgp_oracle as so

    assert _lib.load().gapro_fit_route(m1 + m2, 6) == route
    feats, b1, b2, it = make_gp_problem(300 + m1, m1, m2, t, 6)
    im = 1e-3 * np.random.default_rng(5).standard_normal(m1 + m2)
    out = fit_gp_spp_batch(feats, [(b1, b2, it)], training_iter=50, eval_stale_chol=True, init_mean=[im])[0]
    X = np.concatenate([feats[b1], feats[b2]]).astype(np.float64)
    y = np.r_[-np.ones(m1), np.ones(m2)]
    ref = so.svgp_fit_predict_autograd(X, y, feats[it].astype(np.float64), 50, "f64", eval_chol="stale", init_mean=im)
    _compare(out, ref)


def test_fit_rejects_empty_side():
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch

    with pytest.raises(ValueError):
        fit_gp_spp_batch(np.zeros((4, 6), np.float32), [(np.array([], np.int64), np.array([1]), np.array([2]))])


def test_strip_and_staged_kernels_agree():
    """M_p <= 128 runs the strip-streaming kernel by default; the LDS-staged kernel (forced) must give the
    same answers up to float64 summation order."""
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch
    from gapro_amd.synth import make_gp_problem

    feats_list, probs = [], []
    base = 0
    for i, (m1, m2, t) in enumerate([(5, 9, 3), (33, 20, 17), (64, 64, 70), (50, 40, 1), (20, 90, 200)]):
        f, b1, b2, it = make_gp_problem(300 + i, m1, m2, t, 6)
        feats_list.append(f)
        probs.append((b1 + base, b2 + base, it + base))
        base += len(f)
    feats = np.concatenate(feats_list)
    a = fit_gp_spp_batch(feats, probs, training_iter=50)
    b = fit_gp_spp_batch(feats, probs, training_iter=50, force_staged=True)
    for x, y in zip(a, b):
        np.testing.assert_allclose(x[4], y[4], rtol=1e-6)
        np.testing.assert_allclose(x[3], y[3], rtol=1e-5, atol=1e-7)
        np.testing.assert_array_equal(x[2], y[2])


def test_fit_reports_non_finite_inputs_instead_of_returning_garbage():
    """A NaN feature makes K_ZZ non-finite: the Cholesky flags it on the device and the host raises (gpytorch
    raises NotPSDError / NanError in the same situation); the other fits of the batch do not hide it."""
    from gapro_amd._lib import GaproError
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch
    from gapro_amd.synth import make_gp_problem

    f0, b1, b2, it = make_gp_problem(1, 10, 12, 5, 6)
    f1, c1, c2, ct = make_gp_problem(2, 40, 30, 9, 6)
    f1 = f1.copy()
    f1[c1[3], 2] = np.nan
    feats = np.concatenate([f0, f1])
    off = len(f0)
    with pytest.raises(GaproError) as e:
        fit_gp_spp_batch(feats, [(b1, b2, it), (c1 + off, c2 + off, ct + off)], training_iter=5)
    assert e.value.code in (-4, -5)
    ok = fit_gp_spp_batch(feats, [(b1, b2, it)], training_iter=5)[0]  # the clean fit alone is fine
    assert np.isfinite(ok[3]).all()


def test_wave_kernel_and_small_fit_kernel_agree():
    """Round 5: fits of M_p <= 48 at D = 6 run one per WAVEFRONT (route 5, svgp_fit_wave.hip: every matrix as MFMA
    accumulator-layout register tiles, nothing leaves the CU between the first and the last Adam step); with debug bit 20
    they run on the small-fit strip kernel as in rounds 1-4.  Same arithmetic, different summation orders: the two must
    agree within float32 output rounding, for every block count (M_p = 16, 32, 48), ragged sizes, T beyond one 16-column
    block, a supplied initial mean, the stale-Cholesky switch, and a batch in which a wave takes several fits."""
    import torch
    from gapro_amd import _lib
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch
    from gapro_amd.gen_ps_utils import _pipeline
    from gapro_amd.synth import make_gp_problem

    lib = _lib.load()
    feats_list, probs = [], []
    base = 0
    for i, (m1, m2, t) in enumerate([(1, 2, 1), (7, 9, 5), (8, 8, 16), (10, 13, 33), (20, 12, 70), (17, 16, 1), (30, 18, 40),
                                     (2, 40, 9), (24, 24, 17)]):
        assert lib.gapro_fit_route(m1 + m2, 6) == 5
        f, b1, b2, it = make_gp_problem(700 + i, m1, m2, t, 6)
        feats_list.append(f)
        probs.append((b1 + base, b2 + base, it + base))
        base += len(f)
    feats = np.concatenate(feats_list)
    rng = np.random.default_rng(5)
    init = [1e-3 * rng.standard_normal(len(p[0]) + len(p[1])) for p in probs]
    for pipe_kw, im in ((dict(), None), (dict(eval_stale_chol=True), None), (dict(), init)):
        pipe = _pipeline(torch.device("cuda", 0), 50, **pipe_kw)  # the pipeline object fit_gp_spp_batch will use
        old = pipe.opt.reserved
        wave = fit_gp_spp_batch(feats, probs * 300, training_iter=50, init_mean=None if im is None else im * 300, **pipe_kw)
        pipe.opt.reserved = old | (1 << 20)
        try:
            small = fit_gp_spp_batch(feats, probs, training_iter=50, init_mean=im, **pipe_kw)
        finally:
            pipe.opt.reserved = old
        for k in range(len(probs)):
            for x, y in zip(wave[k], small[k]):
                np.testing.assert_allclose(np.asarray(x, np.float64), np.asarray(y, np.float64), rtol=0, atol=2e-6)
            for x, y in zip(wave[k], wave[k + len(probs) * 299]):  # the 300th copy: another wave, a later ticket
                np.testing.assert_array_equal(x, y)


def test_small_fit_kernel_and_strip_kernel_agree():
    """The 256-thread small-fit kernel (M_p <= 64, two fits per CU) and the 512-thread strip kernel are two builds of
    one source; with the small route switched off (gapro_fit_options.reserved bit 2) the same fits must come out
    of the other build within float32 rounding, and the route function must report what ran.  (Round 5: M_p <= 48 at
    D = 6 is the wave-per-fit kernel's by default, bit 20 keeps those fits here; M_p = 64 still arrives by itself.)"""
    import torch
    from gapro_amd import _lib
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch
    from gapro_amd.gen_ps_utils import _pipeline
    from gapro_amd.synth import make_gp_problem

    lib = _lib.load()
    for (m1, m2, t) in [(1, 2, 1), (7, 9, 5), (20, 28, 33), (31, 33, 64), (3, 4, 70)]:
        assert lib.gapro_fit_route(m1 + m2, 6) == (3 if m1 + m2 > 48 else 5)
        f, b1, b2, it = make_gp_problem(500 + m1, m1, m2, t, 6)
        pipe = _pipeline(torch.device("cuda", 0), 50)
        old = pipe.opt.reserved
        pipe.opt.reserved = old | (1 << 20)
        try:
            a = fit_gp_spp_batch(f, [(b1, b2, it)], training_iter=50)[0]
            pipe.opt.reserved = old | (1 << 20) | 4
            b = fit_gp_spp_batch(f, [(b1, b2, it)], training_iter=50)[0]
        finally:
            pipe.opt.reserved = old
        for x, y in zip(a, b):
            np.testing.assert_allclose(np.asarray(x, np.float64), np.asarray(y, np.float64), rtol=0, atol=2e-6)


def test_three_staged_launches_of_one_batch_match_the_oracle():
    """D = 16: one batch whose staged fits fall into all three launches of gapro_svgp_fit_batch -- M_p = 304 (k-major
    product forms, k_svgp_fit<2, false>), M_p = 256 (copy-free forms, but 2 x 16 x 256 staged coordinates push the LDS
    need beyond what fits a CU twice: k_svgp_fit<2, true> behind the former) and M_p = 144 (the rest) -- each against
    the float64 oracle, 50 Adam steps."""
    from gapro_amd import _lib
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch
    from gapro_amd.synth import make_gp_problem

    feats_list, probs, raw = [], [], []
    base = 0
    for i, (m1, m2, t) in enumerate([(150, 152, 20), (125, 128, 33), (70, 72, 9)]):
        assert _lib.load().gapro_fit_route(m1 + m2, 16) == 1
        f, b1, b2, it = make_gp_problem(700 + i, m1, m2, t, 16, std=0.5)
        feats_list.append(f)
        raw.append((f, b1, b2, it))
        probs.append((b1 + base, b2 + base, it + base))
        base += len(f)
    outs = fit_gp_spp_batch(np.concatenate(feats_list), probs, training_iter=50)
    for out, (f, b1, b2, it) in zip(outs, raw):
        _compare(out, _oracle(f, b1, b2, it, 50))


@pytest.mark.parametrize("m1,m2,t,route", [(1, 2, 3, 5), (5, 7, 9, 5), (8, 8, 40, 5), (14, 18, 70, 5), (9, 8, 1, 5),
                                           (20, 28, 12, 3), (40, 50, 33, 0), (90, 100, 40, 1), (120, 136, 25, 4),
                                           (120, 136, 25, 2), (250, 262, 30, 4)])
def test_fit_matches_oracle_with_deep_features_on_every_route(m1, m2, t, route):
    """D = 32 (--use_deepfeat) against the float64 oracle on each kernel: wave-per-fit (5; round 6: M_p <= 32, with G_Z
    as a centred product on the matrix cores instead of the narrow path's per-dimension differences), small-fit strip
    (3), 512-thread strip (0),
    LDS-staged (1), the cluster kernel (4: on ONE workgroup for 192 < M_p < 512, where 2 x 32 x M_p staged point
    coordinates do not fit the LDS beside the Cholesky block column, and over 4 at M_p = 512) and the generic kernel
    (2, debug bit 3), 50 Adam steps, the tolerances of D = 6."""
    import torch
    from gapro_amd import _lib
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch
    from gapro_amd.gen_ps_utils import _pipeline
    from gapro_amd.synth import make_gp_problem

    assert _lib.load().gapro_fit_route(m1 + m2, 32) == (route if route != 2 else 4)
    feats, b1, b2, it = make_gp_problem(70 + m1, m1, m2, t, 32, std=0.3)
    pipe = _pipeline(torch.device("cuda", 0), 50)
    old = pipe.opt.reserved
    if route == 2:
        pipe.opt.reserved = old | 8
    try:
        out = fit_gp_spp_batch(feats, [(b1, b2, it)], training_iter=50)[0]
    finally:
        pipe.opt.reserved = old
    _compare(out, _oracle(feats, b1, b2, it, 50))


@pytest.mark.parametrize("d,m1,m2,t", [(20, 250, 262, 30), (9, 300, 330, 17)])
def test_cluster_kernel_with_other_feature_widths(d, m1, m2, t):
    """Feature widths between the reference's two (8 < D < 32 takes the deep-feature gradient path with a partly
    empty second 16-column tile; M not a multiple of the 4-row blocks of the kernel evaluation)."""
    from gapro_amd import _lib
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch
    from gapro_amd.synth import make_gp_problem

    assert _lib.load().gapro_fit_route(m1 + m2, d) == 4
    feats, b1, b2, it = make_gp_problem(90 + d, m1, m2, t, d, std=0.4)
    out = fit_gp_spp_batch(feats, [(b1, b2, it)], training_iter=50)[0]
    _compare(out, _oracle(feats, b1, b2, it, 50))


def test_fit_status_is_per_fit_and_a_failed_fit_does_not_touch_its_neighbours():
    """gapro_svgp_fit_batch reports a gapro_status per fit and never fails the batch: a fit with a NaN feature row is
    flagged, the other fits of the same launch are bit-identical to a launch without it."""
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch
    from gapro_amd.synth import make_gp_problem

    parts, probs, base = [], [], 0
    for i, (m1, m2, t) in enumerate([(10, 12, 5), (40, 30, 9), (70, 80, 11), (100, 90, 7)]):
        f, b1, b2, it = make_gp_problem(600 + i, m1, m2, t, 6)
        parts.append(f.copy())
        probs.append((b1 + base, b2 + base, it + base))
        base += len(f)
    clean = fit_gp_spp_batch(np.concatenate(parts), probs, training_iter=20)
    parts[1][3, 2] = np.nan
    outs, status = fit_gp_spp_batch(np.concatenate(parts), probs, training_iter=20, return_status=True)
    assert status[1] in (-4, -5) and (np.delete(status, 1) == 0).all()
    for i in (0, 2, 3):
        for a, b in zip(outs[i], clean[i]):
            np.testing.assert_array_equal(a, b)


def test_failed_cluster_fit_does_not_touch_its_neighbours():
    """The same isolation on the cluster kernel (one fit over several workgroups, status reduced over the cluster): a
    NaN feature row in one of three large fits flags that fit only; the others equal a launch without it, bit for bit."""
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch
    from gapro_amd.synth import make_gp_problem

    parts, probs, base = [], [], 0
    for i, (m1, m2, t) in enumerate([(260, 270, 9), (300, 330, 5), (256, 262, 7), (40, 30, 6)]):
        f, b1, b2, it = make_gp_problem(650 + i, m1, m2, t, 6)
        parts.append(f.copy())
        probs.append((b1 + base, b2 + base, it + base))
        base += len(f)
    clean = fit_gp_spp_batch(np.concatenate(parts), probs, training_iter=8)
    parts[1][17, 4] = np.nan
    outs, status = fit_gp_spp_batch(np.concatenate(parts), probs, training_iter=8, return_status=True)
    assert status[1] in (-4, -5) and (np.delete(status, 1) == 0).all()
    for i in (0, 2, 3):
        for a, b in zip(outs[i], clean[i]):
            np.testing.assert_array_equal(a, b)


def test_psd_safe_cholesky_jitter_retries():
    """gpytorch's psd_safe_cholesky: K_ZZ with duplicated inducing points and no variational jitter is
    singular, and whether a pivot of its factorisation comes out <= 0 is decided by the last bit.  Variations of the
    problem are tried until one fails without retries (GAPRO_ERR_CHOLESKY for that fit ONLY, the clean neighbour of
    the same launch is untouched); with the default retries (K + 1e-8 * 10^i I, i < 3) the same launch goes
    through, and at zero training steps its predictive moments are the prior's, as the oracle's restatement of
    the same rule gives them."""
    import torch
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch
    from gapro_amd.gen_ps_utils import _pipeline
    from gapro_amd.synth import make_gp_problem
    from oracle import svgp_oracle as so

    f2, c1, c2, ct = make_gp_problem(34, 20, 25, 4, 6)
    pipe = _pipeline(torch.device("cuda", 0), 0)
    old = (pipe.opt.jitter, pipe.opt.psd_retries)
    found = None
    try:
        pipe.opt.jitter = 0.0
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
            pipe.opt.psd_retries = 0
            outs0, status0 = fit_gp_spp_batch(allf, launch, training_iter=0, return_status=True)
            assert status0[1] == 0
            if status0[0] == 0:
                continue  # every pivot of this variation happened to round to a positive number
            assert status0[0] == -5
            pipe.opt.psd_retries = 3
            outs, status = fit_gp_spp_batch(allf, launch, training_iter=0, return_status=True)
            assert (status == 0).all()
            for a, b in zip(outs0[1], outs[1]):
                np.testing.assert_array_equal(a, b)
            found = (feats, b1, b2, it, outs[0])
            break
    finally:
        pipe.opt.jitter, pipe.opt.psd_retries = old
    assert found is not None, "no variation produced a non-positive pivot"
    feats, b1, b2, it, out = found
    X = np.concatenate([feats[b1], feats[b2]]).astype(np.float64)
    y = np.r_[-np.ones(len(b1)), np.ones(len(b2))]
    mu_r, var_r, p_r = so.svgp_fit_predict_autograd(X, y, feats[it].astype(np.float64), 0, "f64", jitter=0.0)
    np.testing.assert_allclose(out[3], mu_r, rtol=0, atol=1e-6)
    # var = s + |L_S^T A|^2 - |A|^2 with L_S = I cancels only up to the conditioning of the near-singular factor
    np.testing.assert_allclose(out[4], var_r, rtol=1e-3)


@pytest.mark.parametrize("m1,m2,t", [(32, 32, 40), (64, 64, 40), (250, 262, 30)])
def test_mixed_precision_mode_tracks_the_oracles_restatement_of_the_reference_split(m1, m2, t):
    """gapro_fit_options.precision = MIXED (BASELINE configs[4]): the reference's own split -- float32 parameters, kernel
    matrices, A, B, variances and their gradients (v_mfma_f32), float64 for the Cholesky factor, the L^-1 products and
    their backward -- run by the cluster kernel.  (a) The forward pass (0 training steps) equals the oracle's torch
    restatement of the same split to float32 rounding, and the first Adam step stays within 5e-2 of the float64
    result.  No tighter step-by-step comparison between two float32 evaluations exists: Adam moves a parameter by
    lr * g / (|g| + 1e-8), so a gradient that is exactly zero in float64 (most of L_S and much of Z at the start) is
    float32 rounding noise of ~1e-8 .. 1e-7 and takes a near-full +-0.1 step whose sign is the noise's (tools/
    diag_mixed.py: the torch restatement is 7e-2 off in mu after ONE step).  (b) After 50 steps the kernel is as far
    from the float64 ground truth as that restatement is (both ~1e-2 in sigma^2 here: the 1e-4 of north_star is out
    of reach of ANY float32 evaluation of the reference, which is why float64 is the default;
    profiles/r02_precision_sweep.md); (c) it is deterministic; (d) the same kernel in float64 stays at float32 output
    rounding from the oracle."""
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch
    from gapro_amd.synth import make_gp_problem
    from oracle import svgp_oracle as so

    feats, b1, b2, it = make_gp_problem(4100 + m1, m1, m2, t, 6)
    X = np.concatenate([feats[b1], feats[b2]]).astype(np.float64)
    y = np.r_[-np.ones(m1), np.ones(m2)]
    Xt = feats[it].astype(np.float64)
    run = lambda iters, prec: fit_gp_spp_batch(feats, [(b1, b2, it)], training_iter=iters, precision=prec,  # noqa: E731
                                               cluster_all=True)[0]
    _compare(run(50, "f64"), so.svgp_fit_predict_autograd(X, y, Xt, 50, "f64"))  # (d)
    k0 = run(0, "mixed")
    mu0, var0, p0 = so.svgp_fit_predict_autograd(X, y, Xt, 0, "mixed")
    np.testing.assert_allclose(k0[4], var0, rtol=2e-6)  # (a)
    np.testing.assert_allclose(k0[3], mu0, rtol=0, atol=1e-6)
    k1 = run(1, "mixed")
    mu1, var1, _ = so.svgp_fit_predict_autograd(X, y, Xt, 1, "f64")
    np.testing.assert_allclose(k1[4], var1, rtol=5e-2)
    np.testing.assert_allclose(k1[3], mu1, rtol=0, atol=5e-2)
    k50, again = run(50, "mixed"), run(50, "mixed")
    for a, b in zip(k50, again):
        np.testing.assert_array_equal(a, b)  # (c)
    mu64, var64, p64 = so.svgp_fit_predict_autograd(X, y, Xt, 50, "f64")
    mum, varm, pm = so.svgp_fit_predict_autograd(X, y, Xt, 50, "mixed")
    e_oracle = float(np.max(np.abs(varm - var64) / var64))
    e_kernel = float(np.max(np.abs(k50[4] - var64) / var64))
    assert np.isfinite(k50[3]).all() and (k50[4] > 0).all()
    # (b): the same class as the restatement -- both are rounding noise amplified by Adam, not a fixed offset
    assert e_kernel < max(10 * e_oracle, 0.1), (e_kernel, e_oracle)
    assert np.max(np.abs(k50[0] - p64)) < max(10 * float(np.max(np.abs(pm - p64))), 0.1)


def test_fit_timing_spans_and_offsets_of_two_launches():
    """gapro_fit_timing: the device-side duration of a launch (HIP events on the library's own streams) and where a
    second launch lies on the time axis of the first -- what bench.py's roofline figure is made of."""
    import torch
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch
    from gapro_amd.gen_ps_utils import _pipeline
    from gapro_amd.synth import make_gp_problem

    parts, probs, base = [], [], 0
    for i, (m1, m2, t) in enumerate([(20, 25, 9), (60, 50, 11), (90, 100, 7)]):
        f, b1, b2, it = make_gp_problem(900 + i, m1, m2, t, 6)
        parts.append(f)
        probs.append((b1 + base, b2 + base, it + base))
        base += len(f)
    feats = np.concatenate(parts)
    pipe = _pipeline(torch.device("cuda", 0), 10)
    pipe.profile_fit, pipe.fit_events = True, []
    try:
        fit_gp_spp_batch(feats, probs, training_iter=10)
        fit_gp_spp_batch(feats, probs, training_iter=10)
        a, b = pipe.fit_events[-2:]
        ms_a, ms_b = a.read(), b.read()
        assert ms_a[2] > 0 and ms_b[2] > 0 and ms_a[4] == 0  # no cluster kernel in these launches
        assert ms_a[2] >= max(ms_a[0], ms_a[1], ms_a[3]) - 1e-3  # first start -> last end covers every kernel
        lo_a, hi_a = a.offsets(a)
        lo_b, hi_b = b.offsets(a)
        assert abs(lo_a) < 1e-3 and abs((hi_a - lo_a) - ms_a[2]) < 0.05
        assert lo_b >= hi_a - 0.05 and abs((hi_b - lo_b) - ms_b[2]) < 0.05  # the second launch was issued after the first
    finally:
        pipe.profile_fit, pipe.fit_events = False, []


_TIMEOUT_CHILD = r'''
import sys, time
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
from gapro_amd.gaussian_process_utils import fit_gp_spp_batch
from gapro_amd.gen_ps_utils import _pipeline
from gapro_amd.synth import make_gp_problem
parts, probs, base = [], [], 0
for i, (m1, m2, t) in enumerate([(265, 265, 9), (40, 30, 6), (300, 330, 5)]):
    f, b1, b2, it = make_gp_problem(660 + i, m1, m2, t, 6)
    parts.append(f); probs.append((b1 + base, b2 + base, it + base)); base += len(f)
pipe = _pipeline(torch.device("cuda:0"), 5)
pipe.retry_timeouts = False
t0 = time.time()
outs, status = fit_gp_spp_batch(np.concatenate(parts), probs, training_iter=5, return_status=True)
dt = time.time() - t0
print("STATUS", list(int(s) for s in status), "SECONDS %.2f" % dt, "FINITE", bool(np.isfinite(outs[1][3]).all()))
pipe.retry_timeouts = True
outs, status = fit_gp_spp_batch(np.concatenate(parts), probs, training_iter=5, return_status=True)
print("RETRIED", list(int(s) for s in status), "COUNT", pipe.timeout_retries)
np.savez(sys.argv[2], **{"o%d_%d" % (i, k): np.asarray(a) for i, o in enumerate(outs) for k, a in enumerate(o)})
'''


def test_cluster_barrier_gives_up_instead_of_hanging(tmp_path):
    """the cluster barrier is bounded.  With the test bit that keeps the last member of every
    cluster from ever arriving (as if it had not been given a CU), the cluster fits of the launch report
    GAPRO_ERR_TIMEOUT (-8) after the configured wait instead of spinning forever, and the launch's single-workgroup
    fit is untouched.  In a child process: the timeout is read from the environment once per process.
    VERDICT r03 item 5b: a timeout is transient, so by default (Pipeline.retry_timeouts) those fits are run once more on
    the single-workgroup route -- and come back with status 0 and the CORRECT outputs: equal, to float64 round-off
    across kernels, to what this process gets for the same fits without the test bit."""
    import os
    import subprocess
    import sys

    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch
    from gapro_amd.synth import make_gp_problem

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, GAPRO_CLUSTER_BARRIER_TIMEOUT_MS="400", GAPRO_FIT_FLAGS=str(32768))
    out = str(tmp_path / "retried.npz")
    r = subprocess.run([sys.executable, "-c", _TIMEOUT_CHILD, root, out], capture_output=True, text=True, timeout=300,
                       env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("STATUS")][0]
    assert "STATUS [-8, 0, -8]" in line and "FINITE True" in line, line
    assert float(line.split("SECONDS")[1].split()[0]) < 10.0, line
    assert "GAPRO_FIT_FLAGS=0x8000" in r.stderr  # the debug bits are never silent
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RETRIED")][0]
    assert "RETRIED [0, 0, 0] COUNT 2" in line, line
    parts, probs, base = [], [], 0
    for i, (m1, m2, t) in enumerate([(265, 265, 9), (40, 30, 6), (300, 330, 5)]):
        f, b1, b2, it = make_gp_problem(660 + i, m1, m2, t, 6)
        parts.append(f)
        probs.append((b1 + base, b2 + base, it + base))
        base += len(f)
    want = fit_gp_spp_batch(np.concatenate(parts), probs, training_iter=5)  # the cluster kernel, no test bit
    got = np.load(out)
    for i, o in enumerate(want):
        np.testing.assert_allclose(got["o%d_0" % i], o[0], rtol=0, atol=3e-7)
        np.testing.assert_array_equal(got["o%d_2" % i], o[2])
        np.testing.assert_allclose(got["o%d_3" % i], o[3], rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(got["o%d_4" % i], o[4], rtol=1e-5)


def test_cluster_staging_buffer_grows_with_the_launch():
    """the pinned / device block-table buffers hold two halves; a launch whose table needs up to
    twice the previous one must reallocate (it used to write past its half).  One small cluster launch, then one with
    ten 32-workgroup fits; both must come back clean, and a repeat of the first must reproduce its bits."""
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch
    from gapro_amd.synth import make_gp_problem

    f1, b1, b2, it = make_gp_problem(700, 265, 265, 7, 6)
    first = fit_gp_spp_batch(f1, [(b1, b2, it)], training_iter=2)
    parts, probs, base = [], [], 0
    for i in range(10):
        f, a, b, c = make_gp_problem(710 + i, 500, 500, 5, 6)  # M_p = 1024: 32 workgroups each
        parts.append(f)
        probs.append((a + base, b + base, c + base))
        base += len(f)
    outs, status = fit_gp_spp_batch(np.concatenate(parts), probs, training_iter=1, return_status=True)
    assert (status == 0).all() and all(np.isfinite(o[4]).all() for o in outs)
    again = fit_gp_spp_batch(f1, [(b1, b2, it)], training_iter=2)
    for a, b in zip(first[0], again[0]):
        np.testing.assert_array_equal(a, b)


def test_fits_taken_by_ticket_equal_the_static_block_mapping():
    """Round 4: a workgroup takes the next fit of its kernel's longest-first list when it starts (claim_fit; the grids
    are over-subscribed, spare workgroups exit) instead of running fit blockIdx.x (gapro_fit_options.reserved bit 18).
    Who runs a fit must not matter: a launch with more fits than the GPU holds at once, on every single-workgroup
    kernel, comes out with the same bits either way, and with the bits of the same fit launched alone (a fit claimed
    twice would race on its workspace, a fit never claimed would leave its outputs unwritten)."""
    import torch
    from gapro_amd import gen_ps_utils
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch
    from gapro_amd.synth import make_gp_problem

    parts, probs, base = [], [], 0
    shapes = [(7, 9, 5), (20, 28, 33), (31, 33, 64), (40, 39, 7), (45, 50, 90), (70, 74, 12), (60, 52, 31),
              (100, 60, 30), (130, 126, 20), (150, 160, 9)]
    for i, (m1, m2, t) in enumerate(shapes):
        f, b1, b2, it = make_gp_problem(1300 + i, m1, m2, t, 6)
        parts.append(f)
        probs.append((b1 + base, b2 + base, it + base))
        base += len(f)
    feats = np.concatenate(parts)
    many = probs * 90  # 900 fits: small 360, strip 360, staged 180 -- several rounds of workgroups per kernel
    pipe = gen_ps_utils._pipeline(torch.device("cuda:0"), 6)
    old = int(pipe.opt.reserved)
    try:
        pipe.opt.reserved = old | 262144
        ref, st_ref = fit_gp_spp_batch(feats, many, training_iter=6, return_status=True)
    finally:
        pipe.opt.reserved = old
    got, st = fit_gp_spp_batch(feats, many, training_iter=6, return_status=True)
    assert (st_ref == 0).all() and (st == 0).all()
    singles = [fit_gp_spp_batch(feats, [p], training_iter=6)[0] for p in probs]
    for k in range(len(many)):
        for x, y, z in zip(ref[k], got[k], singles[k % len(probs)]):
            np.testing.assert_array_equal(x, y)
            np.testing.assert_array_equal(y, z)


def test_fit_batch_refuses_retired_and_unknown_debug_bits():
    """A debug bit of gapro_fit_options.reserved that names no switch (a retired A/B switch, or one never defined) makes
    gapro_svgp_fit_batch fail with GAPRO_ERR_BAD_ARG and a message, instead of quietly running the default path; the
    same pipeline fits again once the bit is cleared."""
    import torch
    from gapro_amd import gen_ps_utils
    from gapro_amd._lib import GaproError
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch
    from gapro_amd.synth import make_gp_problem

    f, b1, b2, it = make_gp_problem(7, 20, 24, 9, 6)
    pipe = gen_ps_utils._pipeline(torch.device("cuda:0"), 3)
    old = int(pipe.opt.reserved)
    for bit in (32, 64, 128, 256, 512, 4096, 16384, 524288, 1 << 30):
        try:
            pipe.opt.reserved = old | bit
            with pytest.raises(GaproError) as e:
                fit_gp_spp_batch(f, [(b1, b2, it)], training_iter=3)
        finally:
            pipe.opt.reserved = old
        assert e.value.code == -1 and "debug bits" in str(e.value), bit
    assert np.isfinite(fit_gp_spp_batch(f, [(b1, b2, it)], training_iter=3)[0][3]).all()


def test_workgroup_tiled_products_are_bit_identical_to_the_per_wave_products():
    """Round 3: the staged kernel's products through an LDS ring shared by the workgroup (default at
    M_p = 256, 384; everywhere with gapro_fit_options.reserved bit 13; nowhere with bit 17) accumulate every 16 x 16
    block over the same k in the same order as the per-wave products, so the outputs are the same bits -- whole tiles,
    per-wave strips at ragged edges, lower-triangular outputs kept per-wave, trimmed ranges, prediction batches larger
    than M_p."""
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch
    from gapro_amd.synth import make_gp_problem

    parts, probs, base = [], [], 0
    for i, (m1, m2, t) in enumerate([(70, 74, 12), (80, 96, 50), (130, 126, 20), (100, 60, 300), (200, 190, 77),
                                     (230, 250, 33)]):
        f, b1, b2, it = make_gp_problem(300 + i, m1, m2, t, 6)
        parts.append(f)
        probs.append((b1 + base, b2 + base, it + base))
        base += len(f)
    feats = np.concatenate(parts)
    ref = fit_gp_spp_batch(feats, probs, training_iter=12)
    import torch
    from gapro_amd import gen_ps_utils

    pipe = gen_ps_utils._pipeline(torch.device("cuda:0"), 12)  # the cached pipeline fit_gp_spp_batch uses
    old = int(pipe.opt.reserved)
    try:
        pipe.opt.reserved = old | 131072  # the per-wave products everywhere
        ref = fit_gp_spp_batch(feats, probs, training_iter=12)
        pipe.opt.reserved = old | 8192    # the workgroup-tiled ones wherever they can run
        got = fit_gp_spp_batch(feats, probs, training_iter=12)
    finally:
        pipe.opt.reserved = old
    dflt = fit_gp_spp_batch(feats, probs, training_iter=12)  # and the default mix of the two
    for a, b in zip(ref, dflt):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
    for a, b in zip(ref, got):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)


def test_fit_stress_m2048_against_the_oracle():
    """BASELINE configs[4] at the size bench.py's `stress_m2048` key runs (M = 2048 pooled superpoints per
    region): four concurrent fits (two problems, each twice) on the cluster kernel, 32 workgroups each, three Adam
    steps -- enough for every phase of the forward and backward pass at 128 x 128 blocks of 16 -- against the float64
    autograd oracle; the copies must agree bit for bit."""
    from gapro_amd import _lib
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch
    from gapro_amd.synth import make_gp_problem

    m1, m2, t = 1000, 1048, 64
    assert _lib.load().gapro_fit_route(m1 + m2, 6) == 4
    parts, probs, base = [], [], 0
    for i in range(2):
        f, b1, b2, it = make_gp_problem(950 + i, m1, m2, t, 6)
        parts.append(f)
        probs.append((b1 + base, b2 + base, it + base))
        base += len(f)
    feats = np.concatenate(parts)
    out = fit_gp_spp_batch(feats, [probs[0], probs[1], probs[0], probs[1]], training_iter=3)
    for i in (0, 1):
        for a, b in zip(out[i], out[i + 2]):
            np.testing.assert_array_equal(a, b)
    b1, b2, it = probs[0]
    _compare(out[0], _oracle(feats, b1, b2, it, 3))
