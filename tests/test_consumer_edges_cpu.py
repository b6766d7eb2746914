"""The inputs of test_consumer_edges_gpu.py really are what consumer_cases.py claims (no device), and its tolerances ask
neither too little nor too much:
1. every case has the property its builder names;
2. at the moderate cases the NumPy references agree with oracle/consumer_oracle.py evaluated in float64 -- which the goldens
   pin to the real reference -- values to 1e-12, gradients to the oracle's autograd at 1e-9;
3. the oracle evaluated in float32, the reference's own precision, stays within HALF of the GPU file's tolerance on every
   value case;
4. each case can tell the mistake it exists for, at the GPU file's tolerance."""
import numpy as np
import pytest

import consumer_cases as cc


def _rel(a, b):
    return abs(a - b) / abs(b)


def _fails(got, want, rtol, atol=0.0):
    try:
        np.testing.assert_allclose(got, want, rtol=rtol, atol=atol)
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------------------------------ 1. pool cases
@pytest.mark.parametrize("name", cc.POOL_CASE_NAMES)
def test_pool_cases_are_what_they_claim(name):
    case = cc.pool_case(name)
    n, n_out = len(case.idx), cc.pool_n_out(case)
    assert all(len(c) == n for c in case.chans) and case.idx.min() >= 0 and case.idx.max() < n_out
    (means, count) = cc.pool_expected(case)
    assert all(m.dtype == np.float32 and m.shape == (n_out,) for m in means)
    if case.kind == "exact":
        # values k 2^-16 up to 100 in magnitude, the sentinel among them, at most 2^20 per superpoint: |sum k| < 2^53,
        # so the float64 sum is the integer sum in any order
        assert count.max() <= 1 << 20
        for c in case.chans:
            k = cc.as_float32(c).astype(np.float64) * cc.SCALE
            assert np.array_equal(k, np.rint(k)) and np.abs(k).max() <= 100 * cc.SCALE
        assert n == 1 or any((cc.as_float32(c) == cc.F32(cc.SENTINEL)).any() for c in case.chans[1:])
        assert int(np.abs(np.rint(cc.as_float32(case.chans[1]).astype(np.float64) * cc.SCALE)).sum()) < 1 << 53
        for a, b in zip(means, cc.pool_reference(case)[0]):  # and the float64 reference gives the same bits
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    want = {"n1": lambda: n == 1, "one_address": lambda: n_out == 1 and n > cc.POOL_SWEEP and count[0] == n,
            "n_out_255": lambda: n_out == cc.THREADS - 1, "n_out_256": lambda: n_out == cc.THREADS,
            "n_out_257": lambda: n_out == cc.THREADS + 1,
            "empties": lambda: [s for s in range(n_out) if count[s] == 0] == [0, n_out // 2, n_out - 1],
            "trailing": lambda: n_out - case.idx.max() - 1 > cc.THREADS and all((m[case.meta["used"]:] == 0).all() for m in means),
            "derived_n_out": lambda: case.n_out is None and n_out == cc.THREADS + 1,
            "idx_int32": lambda: case.meta["idx_dtype"] == "int32", "idx_on_cpu": lambda: case.meta["idx_on_cpu"],
            "columns": lambda: case.meta["columns"],
            "chan_float16": lambda: all(c.dtype == np.float16 for c in case.chans),
            "chan_float64": lambda: all(c.dtype == np.float64 and (c.astype(np.float32).astype(np.float64) != c).any()
                                        for c in case.chans),
            "random_small": lambda: case.kind == "ulp" and n_out == cc.THREADS + 1,
            "random_sweep": lambda: case.kind == "ulp" and n > cc.POOL_SWEEP and n % cc.THREADS}[name]
    assert want()
    if name not in ("empties", "trailing"):
        assert count.min() >= 1
    if name == "empties":
        assert all((m[list(case.meta["empty"])] == 0).all() for m in means)


def test_pool_guard_case_holds_only_the_four_bad_indices():
    dirty, clean = cc.pool_guard_case()
    n_out, bad = dirty.n_out, dirty.meta["bad"]
    assert sorted(set(dirty.idx[bad].tolist())) == [-2, -1, n_out, n_out + 1] == sorted(cc.bad_indices(n_out))
    good = dirty.idx[~bad]
    assert good.min() == 0 and good.max() == n_out - 1 and np.array_equal(good, clean.idx)
    # an unguarded kernel would reach sums[3 s .. 3 s + 2] and counts[s]: inside the canaries on either side
    for s in cc.bad_indices(n_out):
        assert -cc.CANARY_PAD <= 3 * s and 3 * s + 2 < 3 * n_out + cc.CANARY_PAD
        assert -cc.CANARY_PAD <= s < n_out + cc.CANARY_PAD
    assert clean.kind == "exact" and cc.pool_exact(clean)[1].min() >= 1


# ------------------------------------------------------------------------------------------ 1. BCE cases
@pytest.mark.parametrize("name", cc.BCE_CASE_NAMES)
def test_bce_cases_are_what_they_claim(name):
    case = cc.bce_case(name)
    G, P = case.x.shape
    value, grad = cc.bce_expected(name)
    assert case.y.shape == (G, P) and case.w.shape == (P,) and grad.shape == (G, P)
    x = case.x.astype(np.float64)
    if case.meta.get("moderate"):
        assert np.abs(x).max() <= 10.0 and np.isfinite(value) and value > 0
    if name.startswith("shape_"):
        assert (G, P) in cc.BCE_SHAPES
        if G > 1:  # just past one sweep, P a multiple neither of the workgroup nor of the sweep
            assert cc.LOSS_SWEEP < G * P <= cc.LOSS_SWEEP + G and P % cc.THREADS and cc.LOSS_SWEEP % P
    if name == "zero_columns":
        zero = case.w == 0
        assert 0 < zero.sum() < P and (grad[:, zero] == 0).all() and (grad[:, ~zero] != 0).all()
    if name == "soft_targets":
        assert ((case.y > 0) & (case.y < 1)).all()
    if name == "bool_targets":
        assert case.y.dtype == np.bool_ and 0 < case.y.sum() < case.y.size
    if name in ("saturated", "extreme"):
        mags = cc.SATURATED if name == "saturated" else cc.EXTREME
        assert set(np.unique(case.y)) == {0.0, 1.0}
        for m in mags:  # both signs on both sides: confident and right, confident and wrong
            for s in (1.0, -1.0):
                for t in (0.0, 1.0):
                    assert ((x == m * s) & (case.y == t)).sum() >= 8, (m, s, t)
    if name == "saturated":
        assert case.w.sum() * G <= 1e6
        assert cc.is_normal_f32(grad).all()  # so that atol 0 asks nothing a float32 cannot hold
        right = (x > 0) == (case.y == 1)
        assert np.abs(grad[right]).max() < 1e-13 and np.abs(grad[~right]).min() > 1e-4
    if name == "extreme":
        right = (x > 0) == (case.y == 1)
        assert np.abs(grad[right]).max() <= 1e-37 and np.abs(grad[~right]).min() > 1e-3
        assert np.isfinite(value) and value > 100
    if name == "zero_weights":
        assert case.w.sum() == 0 and np.isnan(value) and np.isnan(grad).all()  # 0 / 0 in the reference's lines
    if name == "transposed":
        assert case.meta["transposed"] and G != P
    if name == "logits_float16":
        assert np.array_equal(case.x.astype(np.float16).astype(np.float32), case.x)
    if name == "logits_bfloat16":
        assert not (case.x.view(np.uint32) & 0xFFFF).any() and len(np.unique(case.x)) > 100
    if name == "no_grad":
        assert case.meta["no_grad"] and G * P > cc.LOSS_SWEEP


# ------------------------------------------------------------------------------------------ 1. KL cases
@pytest.mark.parametrize("name", cc.KL_CASE_NAMES)
def test_kl_cases_are_what_they_claim(name):
    case = cc.kl_case(name)
    br = cc.kl_branches(case).reshape(-1)
    n = br.size
    n_unl, n_tiny, n_rest = ((br == b).sum() for b in (cc.UNLABELLED, cc.TINY, cc.REST))
    value, g_mu, g_lv = cc.kl_expected(name)
    assert np.isfinite(value) and np.isfinite(g_mu).all() and np.isfinite(g_lv).all()
    assert (g_mu[br == cc.UNLABELLED] == 0).all() and (g_lv[br == cc.UNLABELLED] == 0).all()
    var_l, mu_l = case.var_l.reshape(-1), case.mu_l.reshape(-1)
    if name.startswith("n1_"):
        assert n == 1 and br[0] == case.meta["branch"]
    if name.startswith("mixed_"):
        assert n in (cc.THREADS - 1, cc.THREADS, cc.THREADS + 1, cc.LOSS_SWEEP + 1) and min(n_unl, n_tiny, n_rest) >= n // 5
        assert br[-1] != cc.UNLABELLED or n < cc.LOSS_SWEEP or g_mu[-1] == 0
    if name.startswith("only_"):
        assert (br == case.meta["branch"]).all()
    if name == "only_unlabelled":
        assert value == 0.0 and not g_mu.any() and not g_lv.any()
    if name == "half_labelled":
        kind = case.meta["kind"]
        assert (mu_l[kind == 0] == -100).all() and (var_l[kind == 0] != -100).all()
        assert (var_l[kind == 1] == -100).all() and (mu_l[kind == 1] != -100).all()
        assert (br[kind != 2] == cc.UNLABELLED).all() and (br[kind == 2] != cc.UNLABELLED).all()
        assert n_tiny >= 20 and n_rest >= 20
        assert (var_l[kind == 0] <= case.eps).sum() >= 20 and (var_l[kind == 0] > case.eps).sum() >= 20
    if name.startswith("eps_boundary"):
        below, at, above = case.meta["around"]
        assert at == np.float32(case.eps) and below < at < above
        assert np.nextafter(below, np.float32(1)) == at == np.nextafter(above, np.float32(0))
        assert (br[var_l == below] == cc.TINY).all() and (br[var_l == at] == cc.TINY).all()
        assert (br[var_l == above] == cc.REST).all() and n_tiny == 200 and n_rest == 100
        # the three values fall the same way whether epsilon is compared as a float32 or as a float64
        assert float(below) < case.eps and float(at) <= case.eps < float(above)
    if name == "zero_variance":
        assert (var_l == 0).sum() >= 50 and (br[var_l == 0] == cc.TINY).all() and n_rest >= 50
    if name == "negative_variance":
        neg = (var_l < 0) & (var_l != -100)
        assert neg.sum() >= 50 and (br[neg] == cc.TINY).all() and n_rest >= 50 and n_unl >= 20
        assert set(np.unique(var_l[neg]).tolist()) == {float(np.float32(v)) for v in (-0.25, -1e-6, -99.5)}
    if name in ("options", "eps_boundary_options"):
        assert case.eps != cc.EPS and case.weight != 1.0 and float(np.float32(case.eps)) == case.eps
    if name == "options":
        live = br != cc.UNLABELLED
        assert ((var_l[live] > cc.EPS) & (var_l[live] <= case.eps)).sum() >= 20  # tiny only under this epsilon
        assert n_rest >= 20
    if name == "batched":
        assert case.mu_p.shape == case.lv_p.shape == case.meta["shape"] and case.mu_p.ndim == 2
    if name == "grad_logvar_only":
        assert case.meta["requires"] == (False, True)
    if name == "grad_none":
        assert case.meta["requires"] == (False, False)
    if name == "near_converged":
        live = br != cc.UNLABELLED
        d = (case.mu_p.astype(np.float64) - mu_l)[live]
        assert np.abs(d).max() < 1e-2 and np.abs(case.lv_p).max() < 1e-2 and n_tiny >= 5000 and n_rest >= 5000
    if name == "wide_logvar":
        assert case.lv_p.min() < -9.9 and case.lv_p.max() > 9.9 and min(n_tiny, n_rest) >= 500


# ------------------------------------------------------------------------------------------ 2. references == oracle, float64
def _t64(a):
    import torch

    return torch.from_numpy(np.asarray(a).astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("name", [n for n in cc.BCE_CASE_NAMES if cc.bce_case(n).meta.get("moderate")])
def test_bce_reference_agrees_with_the_oracle_in_float64(name):
    import torch
    from oracle.consumer_oracle import weighted_bce

    case = cc.bce_case(name)
    value, grad = cc.bce_expected(name)
    x = _t64(case.x).requires_grad_(True)
    ref = weighted_bce(x, _t64(case.y), _t64(case.w))
    (g,) = torch.autograd.grad(ref, x)
    assert _rel(value, float(ref.detach())) <= 1e-12
    np.testing.assert_allclose(grad, g.numpy(), rtol=1e-9, atol=0)


# the KL cases are all moderate but the wide one, whose exp(-2 lv) autograd carries as well as the closed form does
@pytest.mark.parametrize("name", cc.KL_CASE_NAMES)
def test_kl_reference_agrees_with_the_oracle_in_float64(name):
    import torch
    from oracle.consumer_oracle import kl_to_gp

    case = cc.kl_case(name)
    value, g_mu, g_lv = cc.kl_expected(name)
    mu_p, lv_p = _t64(case.mu_p).requires_grad_(True), _t64(case.lv_p).requires_grad_(True)
    # the oracle compares its float64 labels with the Python float; the cases keep away from where that could differ
    ref = kl_to_gp(mu_p, lv_p, _t64(case.mu_l), _t64(case.var_l), weight=case.weight, epsilon=case.eps)
    if name in ("only_unlabelled", "n1_unlabelled"):
        assert float(ref) == 0.0 == value
        return
    a, b = torch.autograd.grad(ref, (mu_p, lv_p))
    assert _rel(value, float(ref.detach())) <= 1e-12
    np.testing.assert_allclose(g_mu, a.numpy().reshape(-1), rtol=1e-9, atol=0)
    np.testing.assert_allclose(g_lv, b.numpy().reshape(-1), rtol=1e-9, atol=0)


def test_pool_reference_agrees_with_the_oracle_where_float32_sums_are_exact():
    """oracle.scatter_mean3 sums in float32: it can be held to the bits only where those sums are exact, the float16 case
    (multiples of 1/16, sums below 2^20 / 16)."""
    import torch
    from oracle.consumer_oracle import scatter_mean3

    case = cc.pool_case("chan_float16")
    ref = scatter_mean3(*(torch.from_numpy(cc.as_float32(c)) for c in case.chans), torch.from_numpy(case.idx.copy()), case.n_out)
    for a, b in zip(cc.pool_exact(case)[0], ref):
        np.testing.assert_array_equal(a, b.numpy())
    for name in ("n_out_257", "random_small"):  # elsewhere to float32 round-off
        case = cc.pool_case(name)
        ref = scatter_mean3(*(torch.from_numpy(cc.as_float32(c)) for c in case.chans), torch.from_numpy(case.idx.copy()), case.n_out)
        for a, b in zip(cc.pool_expected(case)[0], ref):
            np.testing.assert_allclose(a, b.numpy(), rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------------------ 3. float32 oracle within half
def _t32(a):
    import torch

    return torch.from_numpy(np.asarray(a).astype(np.float32))


@pytest.mark.parametrize("name", [n for n in cc.BCE_CASE_NAMES if n != "zero_weights"])
def test_float32_oracle_is_within_half_the_bce_value_tolerance(name):
    from oracle.consumer_oracle import weighted_bce

    case = cc.bce_case(name)
    f32 = float(weighted_bce(_t32(case.x), _t32(case.y), _t32(case.w)))
    err = _rel(f32, cc.bce_expected(name)[0])
    print("%s: float32 oracle value off by %.2e" % (name, err))
    assert err <= 0.5 * cc.BCE_VALUE_RTOL


@pytest.mark.parametrize("name", [n for n in cc.KL_CASE_NAMES if n not in ("only_unlabelled", "n1_unlabelled")])
def test_float32_oracle_is_within_half_the_kl_value_tolerance(name):
    from oracle.consumer_oracle import kl_to_gp

    case = cc.kl_case(name)
    f32 = float(kl_to_gp(_t32(case.mu_p), _t32(case.lv_p), _t32(case.mu_l), _t32(case.var_l), weight=case.weight,
                         epsilon=case.eps))
    err = _rel(f32, cc.kl_expected(name)[0])
    print("%s: float32 oracle value off by %.2e" % (name, err))
    assert err <= 0.5 * cc.KL_VALUE_RTOL


# ------------------------------------------------------------------------------------------ 4. each case tells its mistake
def test_one_sided_float64_sigmoid_fails_the_saturated_case():
    """1 / (1 + exp(-x)) - y in float64, the expression k_wbce_grad used: with y = 1 off by 3e-7 at x = 24, 1e-3 at 30,
    4e-2 at 36, exactly 0 from 37 on -- while the two-sided form passes its own float32 rounding.  The other confident
    and right side, x <= -24 with y = 0, is 1 / (1 + exp(|x|)) - 0 and never cancelled."""
    case = cc.bce_case("saturated")
    _, good = cc.bce_expected("saturated")
    _, old = cc.bce_reference(case, sigmoid="one_sided")
    assert _fails(old.astype(np.float32), good, cc.GRAD_RTOL)
    assert not _fails(good.astype(np.float32), good, cc.GRAD_RTOL)
    x = case.x.astype(np.float64)
    right = (x > 0) & (case.y == 1)
    rel = np.abs(old[right] - good[right]) / np.abs(good[right])
    mag = x[right]
    assert 1e-7 < rel[mag == 24].max() < 1e-5 and 1e-4 < rel[mag == 30].max() < 1e-2
    assert (old[right][mag >= 37] == 0).all() and (good != 0).all()
    assert not _fails(old[~right].astype(np.float32), good[~right], cc.GRAD_RTOL)  # nothing else ever cancelled
    # the moderate cases cannot see it: that is why the suite never did
    _, good_m = cc.bce_expected("shape_1x257")
    assert not _fails(cc.bce_reference(cc.bce_case("shape_1x257"), sigmoid="one_sided")[1], good_m, cc.GRAD_RTOL, cc.GRAD_ATOL)


def test_float64_autograd_of_the_value_cancels_too():
    """Why the gradient reference is the closed form: torch autograd through the oracle's expression, in float64, is as
    wrong on the saturated case as the old kernel."""
    import torch
    from oracle.consumer_oracle import weighted_bce

    case = cc.bce_case("saturated")
    x = _t64(case.x).requires_grad_(True)
    (g,) = torch.autograd.grad(weighted_bce(x, _t64(case.y), _t64(case.w)), x)
    assert _fails(g.numpy(), cc.bce_expected("saturated")[1], cc.GRAD_RTOL)


def test_float32_running_sum_fails_the_exact_pool_cases():
    for name in ("one_address", "n_out_257"):
        case = cc.pool_case(name)
        assert case.kind == "exact"
        f32 = cc.pool_reference(case, pool_float32_running=True)[0]
        want = cc.pool_exact(case)[0]
        assert any((a.view(np.uint32) != b.view(np.uint32)).any() for a, b in zip(f32, want)), name
    # and more than an ulp off where every sum meets one address
    case = cc.pool_case("one_address")
    f32, want = cc.pool_reference(case, pool_float32_running=True)[0], cc.pool_exact(case)[0]
    assert max(int(cc.ulp_distance(a, b).max()) for a, b in zip(f32, want)) > 1


def test_strict_compare_fails_the_epsilon_boundary_cases():
    for name in ("eps_boundary", "eps_boundary_options"):
        case = cc.kl_case(name)
        value, g_mu, g_lv = cc.kl_expected(name)
        wrong = cc.kl_reference(case, strict_eps=True)
        assert _fails(wrong[0], value, cc.KL_VALUE_RTOL) and _fails(wrong[1], g_mu, cc.GRAD_RTOL, cc.GRAD_ATOL)
        assert _fails(wrong[2], g_lv, cc.GRAD_RTOL, cc.GRAD_ATOL)
        moved = cc.kl_branches(case, strict_eps=True) != cc.kl_branches(case)
        assert moved.sum() == 100 and (case.var_l[moved] == np.float32(case.eps)).all()


def test_counting_half_labelled_entries_fails_the_half_labelled_case():
    case = cc.kl_case("half_labelled")
    value, g_mu, g_lv = cc.kl_expected("half_labelled")
    with np.errstate(all="ignore"):
        wrong = cc.kl_reference(case, half_labelled=True)
    assert _fails(wrong[0], value, cc.KL_VALUE_RTOL) and _fails(wrong[1], g_mu, cc.GRAD_RTOL, cc.GRAD_ATOL)
    assert _fails(wrong[2], g_lv, cc.GRAD_RTOL, cc.GRAD_ATOL)


def test_dropping_the_small_constants_fails_a_short_case():
    # + 1e-4 on the group counts: one part in 1e4 of a single-entry group
    for name in ("n1_tiny", "n1_rest"):
        value, g_mu, _ = cc.kl_expected(name)
        wrong = cc.kl_reference(cc.kl_case(name), count_eps=0.0)
        assert _fails(wrong[0], value, cc.KL_VALUE_RTOL) and _fails(wrong[1], g_mu, cc.GRAD_RTOL, cc.GRAD_ATOL), name
    # + 1e-6 on the row count: one part in 1e6 of a single row.  rtol 2e-6 cannot see that (it would from G = 0 only, which
    # the wrapper refuses), so the one-row cases hold their gradient to two float32 ulps as well: the gradient is a float64
    # evaluation rounded once
    for name in ("shape_1x1", "shape_1x257"):
        value, grad = cc.bce_expected(name)
        wrong = cc.bce_reference(cc.bce_case(name), row_eps=0.0)
        assert not _fails(wrong[0], value, cc.BCE_VALUE_RTOL) and not _fails(wrong[1], grad, cc.GRAD_RTOL)
        assert _fails(wrong[1], grad, cc.SHORT_GRAD_RTOL), name
        assert not _fails(grad.astype(np.float32), grad, cc.SHORT_GRAD_RTOL)
        assert _fails(wrong[1].astype(np.float32), grad, cc.SHORT_GRAD_RTOL), name
