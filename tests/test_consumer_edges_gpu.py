"""The consumer label ops (gapro_amd/consumer_ops.py over csrc/consumer.hip) at their kernel edges, against the plain
float64 references of consumer_cases.py: workgroup and grid-sweep boundaries, short inputs, saturated logits, the
var <= eps boundary, half-labelled entries, non-contiguous and non-float32 tensors, the launches without gradients, a side
stream, and indices out of range.

Tolerances are those of test_consumer_gpu.py: rtol 2e-6 for the BCE value and every gradient (atol 1e-30; 0 on the
saturated case), rtol 1e-5 for the KL value; the pool is bit-exact where its sums are exact and within one float32 ulp
elsewhere.  test_consumer_edges_cpu.py proves on the CPU that every case is what it claims, that float32 -- the
reference's own precision -- meets these tolerances with half to spare, and that each case fails under the mistake it
exists for, so that nothing here passes vacuously."""
import ctypes as C

import numpy as np
import pytest

import consumer_cases as cc

pytestmark = pytest.mark.gpu


def _dev(a, dtype=None):
    import torch

    t = torch.from_numpy(np.array(a))  # a writable copy
    return (t if dtype is None else t.to(dtype)).cuda()


def _max_rel(got, want):
    """Largest |got - want| / |want| over the entries with want != 0 (0 where both are 0)."""
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    live = want != 0
    return float((np.abs(got - want)[live] / np.abs(want)[live]).max()) if live.any() else 0.0


# ========================================================================================== pool
def _pool_inputs(case):
    import torch

    idx = torch.from_numpy(case.idx.copy())
    if case.meta.get("idx_dtype") == "int32":
        idx = idx.to(torch.int32)
    if not case.meta.get("idx_on_cpu"):
        idx = idx.cuda()
    if case.meta.get("columns"):
        both = torch.from_numpy(np.stack([np.array(c) for c in case.chans], axis=1)).cuda()
        chans = [both[:, k] for k in range(3)]
        assert not chans[0].is_contiguous()
    else:
        chans = [_dev(c) for c in case.chans]
    return chans, idx


def _run_pool(case):
    from gapro_amd.consumer_ops import pool_labels_to_superpoints

    chans, idx = _pool_inputs(case)
    return pool_labels_to_superpoints(*chans, idx, case.n_out)


def _check_pool(case, got, label=""):
    import torch

    want, _ = cc.pool_expected(case)
    worst = 0
    for g, w in zip(got, want):
        assert g.dtype == torch.float32 and g.is_cuda and tuple(g.shape) == w.shape
        worst = max(worst, int(cc.ulp_distance(g.cpu().numpy(), w).max()))
    print("pool %s%s: %d superpoints, largest distance %d ulp (%s)" % (case.name, label, len(want[0]), worst, case.kind))
    assert worst <= (0 if case.kind == "exact" else 1)


@pytest.mark.parametrize("name", cc.POOL_CASE_NAMES)
def test_pool_means(name):
    case = cc.pool_case(name)
    _check_pool(case, _run_pool(case))


def test_pool_refuses_indices_out_of_range():
    """Below 0 or at or above n_out, given or derived: a ValueError that names the range, before anything is launched."""
    import torch
    from gapro_amd.consumer_ops import pool_labels_to_superpoints

    case = cc.pool_case("idx_int32")
    chans = [_dev(c) for c in case.chans]
    for bad in cc.bad_indices(case.n_out):
        idx = case.idx.copy()
        idx[len(idx) // 2] = bad
        lo, hi = int(idx.min()), int(idx.max())
        out = None
        with pytest.raises(ValueError, match=r"\[%d, %d\].*\[0, %d\)" % (lo, hi, case.n_out)):
            out = pool_labels_to_superpoints(*chans, torch.from_numpy(idx).cuda(), case.n_out)
        assert out is None
    idx = case.idx.copy()
    idx[0] = -1
    with pytest.raises(ValueError):  # a negative index is refused when n_out is derived, too
        pool_labels_to_superpoints(*chans, torch.from_numpy(idx).cuda())
    idx[0] = case.n_out + 5  # while a large one only lengthens the derived output
    got = pool_labels_to_superpoints(*chans, torch.from_numpy(idx).cuda())
    assert len(got[0]) == case.n_out + 6 and float(got[0][case.n_out]) == 0.0
    _check_pool(case, _run_pool(case), " after the refusals")


def test_pool_kernel_skips_indices_out_of_range():
    """gapro_label_pool_mean itself, given -2, -1, n_out and n_out + 1 among good indices: the scratch and the outputs are
    carved out of the middle of larger allocations with 64 canary elements on either side, which is as far as an
    unguarded kernel would reach with these four; the canaries stay, and the means are those of the good points."""
    import torch
    from gapro_amd._lib import Context

    dirty, clean = cc.pool_guard_case()
    n_out, pad = dirty.n_out, cc.CANARY_PAD
    ctx = Context.get(0)
    dev = torch.device("cuda", 0)
    sums_all = torch.full((pad + 3 * n_out + pad,), 12345.0, dtype=torch.float64, device=dev)
    counts_all = torch.full((pad + n_out + pad,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    outs_all = [torch.full((pad + n_out + pad,), -7.5, dtype=torch.float32, device=dev) for _ in range(3)]
    sums, counts = sums_all[pad:pad + 3 * n_out], counts_all[pad:pad + n_out]
    outs = [o[pad:pad + n_out] for o in outs_all]
    assert sums.data_ptr() == sums_all.data_ptr() + 8 * pad and counts.data_ptr() == counts_all.data_ptr() + 4 * pad
    idx = _dev(dirty.idx)
    chans = [_dev(c) for c in dirty.chans]
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rc = ctx.lib.gapro_label_pool_mean(ctx.handle, stream, len(dirty.idx), n_out, idx.data_ptr(), chans[0].data_ptr(),
                                       chans[1].data_ptr(), chans[2].data_ptr(), sums.data_ptr(), counts.data_ptr(),
                                       outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    for whole, canary in ((sums_all, 12345.0), (counts_all, 0x5A5A5A5A)) + tuple((o, -7.5) for o in outs_all):
        assert bool((whole[:pad] == canary).all()) and bool((whole[-pad:] == canary).all())
    want, count = cc.pool_exact(clean)
    np.testing.assert_array_equal(counts.cpu().numpy(), count)
    for g, w in zip(outs, want):
        np.testing.assert_array_equal(g.cpu().numpy().view(np.uint32), w.view(np.uint32))


# ========================================================================================== weighted BCE
def _bce_inputs(case, requires_grad=True):
    """(leaf, logits as the op gets them, targets, weights) on the device."""
    import torch

    dtype = {"float16": torch.float16, "bfloat16": torch.bfloat16}.get(case.meta.get("dtype"))
    if case.meta.get("transposed"):
        leaf = _dev(case.x.T).contiguous().requires_grad_(requires_grad)  # [P, G]
        x = leaf.t()
        assert not x.is_contiguous()
    else:
        leaf = x = _dev(case.x, dtype).requires_grad_(requires_grad)
    return leaf, x, _dev(case.y), _dev(case.w)


def _run_bce(case, scale=1.0):
    from gapro_amd.consumer_ops import prob_weighted_bce_with_logits

    leaf, x, y, w = _bce_inputs(case)
    loss = prob_weighted_bce_with_logits(x, y, w)
    (scale * loss).backward()
    return loss.detach(), leaf.grad


def _check_bce(name, loss, grad, atol=cc.GRAD_ATOL, scale=1.0, label=""):
    import torch

    case = cc.bce_case(name)
    value, want = cc.bce_expected(name)
    assert loss.dtype == torch.float32 and loss.shape == () and grad.dtype == torch.float32
    if case.meta.get("transposed"):
        assert tuple(grad.shape) == case.x.T.shape  # in the layout of the tensor that was transposed
        grad = grad.t()
    assert tuple(grad.shape) == case.x.shape
    got = grad.cpu().numpy().astype(np.float64) / scale
    print("bce %s%s: [%d, %d] value %.9g off by %.2e, gradient by %.2e" % ((name, label) + case.x.shape + (
        float(loss), abs(float(loss) - value) / abs(value), _max_rel(got, want))))
    np.testing.assert_allclose(float(loss), value, rtol=cc.BCE_VALUE_RTOL)
    np.testing.assert_allclose(got, want, rtol=cc.GRAD_RTOL, atol=atol)
    return got, want


@pytest.mark.parametrize("name", cc.BCE_PLAIN)
def test_bce_value_and_gradient(name):
    case = cc.bce_case(name)
    loss, grad = _run_bce(case, scale=1.0 if name == "saturated" else 4.0)  # 4: exact in every format
    got, want = _check_bce(name, loss, grad, atol=0.0 if name == "saturated" else cc.GRAD_ATOL,
                           scale=1.0 if name == "saturated" else 4.0)
    if name == "zero_columns":
        assert (got[:, case.w == 0] == 0).all()
    if case.x.shape[0] == 1:  # one row: the 1e-6 of the row count shows only at this resolution (see consumer_cases.py)
        np.testing.assert_allclose(got, want, rtol=cc.SHORT_GRAD_RTOL, atol=0)


def test_bce_extreme_logits():
    """|x| = 100 and 1e4: the value, the confident-and-wrong gradients, and confident-and-right ones that have all but
    vanished (a float32 cannot hold them: at most 1e-37 in magnitude, of either sign or 0)."""
    case = cc.bce_case("extreme")
    value, want = cc.bce_expected("extreme")
    loss, grad = _run_bce(case)
    got = grad.cpu().numpy().astype(np.float64)
    right = (case.x > 0) == (case.y == 1)
    print("bce extreme: value %.9g off by %.2e, wrong-side gradient by %.2e, largest right-side gradient %.3g" % (
        float(loss), abs(float(loss) - value) / value, _max_rel(got[~right], want[~right]), np.abs(got[right]).max()))
    np.testing.assert_allclose(float(loss), value, rtol=cc.BCE_VALUE_RTOL)
    np.testing.assert_allclose(got[~right], want[~right], rtol=cc.GRAD_RTOL, atol=0)
    assert np.isfinite(got).all() and np.abs(got[right]).max() <= 1e-37


def test_bce_all_weights_zero_is_nan_and_the_device_goes_on():
    """sum w = 0: the reference's lines give 0 / 0, and so does the op -- value and every gradient NaN, no fault."""
    import torch

    value, want = cc.bce_expected("zero_weights")
    assert np.isnan(value) and np.isnan(want).all()
    loss, grad = _run_bce(cc.bce_case("zero_weights"))
    torch.cuda.synchronize()
    assert np.isnan(float(loss)) and bool(torch.isnan(grad).all())
    _check_bce("soft_targets", *_run_bce(cc.bce_case("soft_targets")), label=" after the NaN")


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_bce_low_precision_logits(dtype):
    """The gradient comes back in the logits' dtype: every entry is the rounding to that dtype of a value within rtol of
    the expected one (rounding is monotone: between the roundings of the two ends).  The backward pass is scaled by 2^14,
    exactly, so that every gradient is a normal float16."""
    import torch

    name = "logits_" + dtype
    case = cc.bce_case(name)
    tdt = getattr(torch, dtype)
    value, want = cc.bce_expected(name)
    want = want * 2.0 ** 14
    loss, grad = _run_bce(case, scale=2.0 ** 14)
    assert grad.dtype == tdt and loss.dtype == torch.float32 and tuple(grad.shape) == case.x.shape
    ends = [torch.from_numpy(want * f).to(torch.float32).to(tdt).double().numpy() for f in (1 - cc.GRAD_RTOL, 1 + cc.GRAD_RTOL)]
    lo, hi = np.minimum(*ends), np.maximum(*ends)
    got = grad.double().cpu().numpy()
    exact = torch.from_numpy(want).to(torch.float32).to(tdt).double().numpy()
    print("bce %s: value off by %.2e, %d of %d gradients are not the rounded expected value" % (
        name, abs(float(loss) - value) / value, int((got != exact).sum()), got.size))
    np.testing.assert_allclose(float(loss), value, rtol=cc.BCE_VALUE_RTOL)
    assert ((got >= lo) & (got <= hi)).all()
    assert (np.abs(exact) >= 2.0 ** -14).all() and np.abs(exact).max() < 100 and len(np.unique(got)) > 100


def test_bce_without_gradient_takes_the_one_workgroup_launch():
    import torch
    from gapro_amd.consumer_ops import prob_weighted_bce_with_logits

    case = cc.bce_case("no_grad")
    value, _ = cc.bce_expected("no_grad")
    leaf, x, y, w = _bce_inputs(case, requires_grad=False)
    plain = prob_weighted_bce_with_logits(x, y, w)
    assert not plain.requires_grad and plain.dtype == torch.float32
    with_grad, grad = _run_bce(case)
    rel = abs(float(plain) - float(with_grad)) / abs(float(with_grad))
    print("bce no_grad: value off by %.2e, from the gradient run by %.2e" % (abs(float(plain) - value) / value, rel))
    np.testing.assert_allclose(float(plain), value, rtol=cc.BCE_VALUE_RTOL)
    assert rel <= 1e-12  # both reduce in float64, in another order
    np.testing.assert_allclose(grad.cpu().numpy(), cc.bce_expected("no_grad")[1], rtol=cc.GRAD_RTOL, atol=cc.GRAD_ATOL)


# ========================================================================================== KL to GP
def _run_kl(case, requires=(True, True)):
    from gapro_amd.consumer_ops import kl_to_gp_loss

    mu_p, lv_p = _dev(case.mu_p).requires_grad_(requires[0]), _dev(case.lv_p).requires_grad_(requires[1])
    loss = kl_to_gp_loss(mu_p, lv_p, _dev(case.mu_l), _dev(case.var_l), weight=case.weight, epsilon=case.eps)
    if any(requires):
        loss.backward()
    return loss.detach(), mu_p.grad, lv_p.grad


def _check_kl(name, loss, g_mu, g_lv, label=""):
    import torch

    case = cc.kl_case(name)
    value, want_mu, want_lv = cc.kl_expected(name)
    assert loss.dtype == torch.float32 and loss.shape == ()
    errs = []
    for got, want in ((g_mu, want_mu), (g_lv, want_lv)):
        if got is None:
            errs.append(float("nan"))
            continue
        assert got.dtype == torch.float32 and tuple(got.shape) == case.mu_p.shape  # [B, n] comes back as [B, n]
        errs.append(_max_rel(got.cpu().numpy(), want))
    off = abs(float(loss) - value) / abs(value) if value else abs(float(loss))
    print("kl %s%s: n = %d value %.9g off by %.2e, d/dmu by %.2e, d/dlogvar by %.2e" % (
        name, label, case.mu_p.size, float(loss), off, errs[0], errs[1]))
    if value == 0.0:
        assert float(loss) == 0.0
    else:
        np.testing.assert_allclose(float(loss), value, rtol=cc.KL_VALUE_RTOL)
    for got, want in ((g_mu, want_mu), (g_lv, want_lv)):
        if got is not None:
            np.testing.assert_allclose(got.cpu().numpy().reshape(-1), want, rtol=cc.GRAD_RTOL, atol=cc.GRAD_ATOL)


@pytest.mark.parametrize("name", [n for n in cc.KL_CASE_NAMES if not n.startswith("grad_")])
def test_kl_value_and_gradients(name):
    _check_kl(name, *_run_kl(cc.kl_case(name)))


def test_kl_unlabelled_entries_get_exact_zeros():
    for name in ("half_labelled", "only_unlabelled", "mixed_257"):
        case = cc.kl_case(name)
        unl = cc.kl_branches(case).reshape(-1) == cc.UNLABELLED
        _, g_mu, g_lv = _run_kl(case)
        assert unl.any() and not g_mu.cpu().numpy().reshape(-1)[unl].any() and not g_lv.cpu().numpy().reshape(-1)[unl].any()


def test_kl_gradient_of_the_log_variance_only():
    case = cc.kl_case("grad_logvar_only")
    loss, g_mu, g_lv = _run_kl(case, case.meta["requires"])
    assert g_mu is None and g_lv is not None
    _check_kl("grad_logvar_only", loss, g_mu, g_lv)


def test_kl_without_gradients_takes_the_one_workgroup_launch():
    case = cc.kl_case("grad_none")
    plain, g_mu, g_lv = _run_kl(case, case.meta["requires"])
    assert g_mu is None and g_lv is None
    _check_kl("grad_none", plain, None, None)
    with_grad, g_mu, g_lv = _run_kl(case)
    _check_kl("grad_none", with_grad, g_mu, g_lv, " with gradients")
    assert abs(float(plain) - float(with_grad)) <= 1e-12 * abs(float(with_grad))


def test_kl_of_nothing_is_zero():
    import torch
    from gapro_amd.consumer_ops import kl_to_gp_loss

    empty = torch.empty(0, device="cuda")
    mu_p = torch.empty(0, device="cuda", requires_grad=True)
    loss = kl_to_gp_loss(mu_p, empty.clone(), empty, empty)
    loss.backward()
    assert float(loss.detach()) == 0.0 and loss.dtype == torch.float32 and tuple(mu_p.grad.shape) == (0,)


def test_consumer_ops_refuse_cpu_tensors():
    import torch
    from gapro_amd.consumer_ops import kl_to_gp_loss, pool_labels_to_superpoints, prob_weighted_bce_with_logits

    case = cc.kl_case("mixed_255")
    cpu = [torch.from_numpy(np.array(a)) for a in (case.mu_p, case.lv_p, case.mu_l, case.var_l)]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kl_to_gp_loss(*cpu)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kl_to_gp_loss(cpu[0], cpu[1].cuda(), cpu[2].cuda(), cpu[3].cuda())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        prob_weighted_bce_with_logits(cpu[0][None, :], cpu[1][None, :], cpu[2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pool_labels_to_superpoints(cpu[0], cpu[1], cpu[2], torch.zeros(len(cpu[0]), dtype=torch.int64))


# ========================================================================================== a side stream
def test_ops_on_a_side_stream_equal_the_default_stream():
    """Each op once under torch.cuda.stream(side), with unrelated work queued on the default stream before it: the launches,
    their memsets and their scratch must follow the current stream."""
    import torch

    pool_case, bce_name, kl_name = cc.pool_case("n_out_257"), "shape_5x52429", "mixed_262145"
    base_pool = [o.cpu().numpy() for o in _run_pool(pool_case)]
    base_bce = _run_bce(cc.bce_case(bce_name))
    base_kl = _run_kl(cc.kl_case(kl_name))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    busy = torch.randn(2048, 2048, device="cuda")
    torch.cuda.synchronize()
    for _ in range(20):  # a few milliseconds of work ahead on the default stream
        busy = busy @ busy * 1e-3
    with torch.cuda.stream(side):
        got_pool = _run_pool(pool_case)
        got_bce = _run_bce(cc.bce_case(bce_name))
        got_kl = _run_kl(cc.kl_case(kl_name))
    side.synchronize()
    torch.cuda.synchronize()
    _check_pool(pool_case, got_pool, " on a side stream")
    for a, b in zip(got_pool, base_pool):
        np.testing.assert_array_equal(a.cpu().numpy().view(np.uint32), b.view(np.uint32))
    _check_bce(bce_name, *got_bce, label=" on a side stream")
    _check_kl(kl_name, *got_kl, label=" on a side stream")
    for got, base in ((got_bce, base_bce), (got_kl, base_kl)):
        assert abs(float(got[0]) - float(base[0])) <= 1e-12 * abs(float(base[0]))
        for a, b in zip(got[1:], base[1:]):  # float64 sums in another order may move a float32 rounding: one ulp
            np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=2.0 ** -23, atol=0)
