"""gapro_spp_plan_build and gapro_spp_pool_forward / _backward on the MI355X: ``superpoint_plan`` / ``superpoint_pool``,
the ``scatter_*`` drop-ins, ``custom_scatter_mean``, ``isbnet_spp_pool`` and ``spformer_pool`` of consumer_ops on every
case of tests/spp_pool_cases.py against the NumPy restatement tests/spp_pool_ref.py.

Outputs, ``arg``, gradients, the CSR and ``spp_batch_offsets`` are compared BIT FOR BIT: float32 arithmetic in a defined
order, every operation rounded on its own on both sides.  Only torch's own ``index_add_`` statement, whose order is
undefined, is compared within the derived bound of two float32 sums of the same terms.
"""
import contextlib

import numpy as np
import pytest

import spp_pool_cases as cases
import spp_pool_ref as ref

pytestmark = pytest.mark.gpu

_REF = {}  # key -> the restatement's answer, computed once and left unchanged


def _want(key, fn):
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def _dev(a, i32=False):
    import torch

    a = np.ascontiguousarray(a)
    if i32 and a.dtype == np.int64:
        a = a.astype(np.int32)
    return torch.from_numpy(a).to("cuda:0")


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@contextlib.contextmanager
def no_host_read():
    """Fails on any synchronising call torch knows of: a device-to-host copy, ``item()``, a stream synchronisation."""
    import torch

    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode(before)


def _plan(case, check=True):
    from gapro_amd import consumer_ops as ops

    i32 = case.get("i32", False)
    kw = {}
    if "point_map" in case:
        kw.update(point_map=_dev(case["point_map"], i32), n_rows=case["R"])
    if "batch_offsets" in case:
        kw.update(batch_offsets=_dev(case["batch_offsets"], i32))
    return ops.superpoint_plan(_dev(case["index"], i32), n_spps=case["S"], check=check, **kw)


def _plan_want(name, case):
    return _want(("plan", name), lambda: ref.plan_ref(case["index"], case["S"], case.get("point_map"), case.get("R"),
                                                     case.get("batch_offsets")))


def _check_plan(plan, want):
    for k in ("seg_off", "seg_pts", "counts", "row_off", "row_pts", "seg_rows", "spp_batch_offsets"):
        if k in want:
            assert _same(getattr(plan, k).cpu().numpy(), want[k]), k
        else:
            assert getattr(plan, k) is None, k


def _check_pools(name, case, plan):
    """Forward, arg and gradient of both reductions through ``plan`` against the restatement."""
    from gapro_amd import consumer_ops as ops

    pm, R = case.get("point_map"), case.get("R")
    g = cases.upstream(case)
    for reduce in ("mean", "max"):
        want, want_arg = _want(("fwd", name, reduce),
                               lambda: ref.pool_forward_ref(case["src"], case["index"], case["S"], reduce, pm))
        x = _dev(case["src"]).requires_grad_(True)
        got = ops.superpoint_pool(x, plan, reduce, return_arg=reduce == "max")
        out, arg = got if reduce == "max" else (got, None)
        o = out.detach().cpu().numpy()
        assert _same(o, want), (reduce, np.flatnonzero(o.view(np.uint32) != want.view(np.uint32))[:8])
        if reduce == "max":
            assert _same(arg.cpu().numpy(), want_arg) and not arg.requires_grad
        want_back = _want(("bwd", name, reduce),
                          lambda: ref.pool_backward_ref(g, case["index"], case["S"], reduce, want_arg, pm, R))
        out.backward(_dev(g))
        assert _same(x.grad.cpu().numpy(), want_back), reduce


@pytest.mark.parametrize("name", cases.POOL_NAMES)
def test_plan_and_pools_bit_for_bit(name):
    case = cases.pool_cases()[name]
    plan = _plan(case)
    _check_plan(plan, _plan_want(name, case))
    _check_pools(name, case, plan)


def test_batch_offsets_equal_the_loop_of_unique():
    for name in ("batch_empty_sample", "batch_one_sample"):
        case = cases.pool_cases()[name]
        assert _same(_plan(case).spp_batch_offsets.cpu().numpy(), ref.unique_loop(case["index"], case["batch_offsets"]))


def test_two_runs_give_identical_bytes():
    from gapro_amd import consumer_ops as ops

    for name in ("one_segment", "segment_70000", "map_shared_rows", "second_byte"):
        case = cases.pool_cases()[name]
        runs = []
        for _ in range(2):
            plan = _plan(case)
            x = _dev(case["src"]).requires_grad_(True)
            out = ops.superpoint_pool(x, plan)
            out.backward(_dev(cases.upstream(case)))
            runs.append([t.cpu().numpy() for t in (plan.seg_off, plan.seg_pts, plan.counts, out.detach(), x.grad)])
        assert all(_same(a, b) for a, b in zip(*runs)), name


def test_pool_discriminates_the_wrong_conventions():
    from gapro_amd import consumer_ops as ops

    c = cases.pool_cases()["three_way"]
    got = ops.superpoint_pool(_dev(c["src"]), _plan(c)).cpu().numpy()
    assert _same(got, ref.pool_forward_ref(c["src"], c["index"], 1)[0])
    for wrong in ("reversed", "tree", "reciprocal"):
        assert not _same(got, ref.pool_forward_ref(c["src"], c["index"], 1, convention=wrong)[0]), wrong
    z = cases.pool_cases()["negative_zero"]
    zero = ops.superpoint_pool(_dev(z["src"]), _plan(z)).cpu().numpy()
    assert not np.signbit(zero[:3]).any() and (zero[:3] == 0).all()  # a lone -0.0, two of them, an empty segment
    m = cases.pool_cases()["max_edges"]
    out, arg = ops.superpoint_pool(_dev(m["src"]), _plan(m), "max", return_arg=True)
    arg = arg.cpu().numpy()
    assert arg[:, 0].tolist() == [0, 4, 6, 8, 10, 12, 15, 17, 16] and (arg[7] == 17).all()  # ties, zeros, NaNs, empty
    for wrong in ("last_tie", "nan"):
        assert not _same(arg, ref.pool_forward_ref(m["src"], m["index"], m["S"], "max", convention=wrong)[1]), wrong
    s = cases.shared_row_case()
    plan = _plan(s)
    x = _dev(s["src"]).requires_grad_(True)
    ops.superpoint_pool(x, plan).backward(_dev(s["g"]))
    assert _same(x.grad.cpu().numpy(), ref.pool_backward_ref(s["g"], s["index"], s["S"], point_map=s["point_map"], R=s["R"]))
    assert not _same(x.grad.cpu().numpy(), ref.pool_backward_ref(s["g"], s["index"], s["S"], point_map=s["point_map"],
                                                                 R=s["R"], convention="by_segment"))


@pytest.mark.parametrize("name", ("n257", "flat_1d", "empty_segments", "segment_lengths"))
def test_scatter_drop_ins(name):
    import torch

    from gapro_amd import consumer_ops as ops

    case = cases.pool_cases()[name]
    src, idx = _dev(case["src"]), _dev(case["index"])
    want, _ = _want(("fwd", name, "mean"), lambda: ref.pool_forward_ref(case["src"], case["index"], case["S"], "mean"))
    wmax, warg = _want(("fwd", name, "max"), lambda: ref.pool_forward_ref(case["src"], case["index"], case["S"], "max"))
    assert _same(ops.scatter_mean(src, idx, dim=0, dim_size=case["S"]).cpu().numpy(), want)
    out, arg = ops.scatter_max(src, idx, 0, dim_size=case["S"])
    assert _same(out.cpu().numpy(), wmax) and _same(arg.cpu().numpy(), warg)
    top = int(case["index"].max()) + 1  # dim_size=None: the reference's max + 1
    assert _same(ops.scatter_mean(src, idx).cpu().numpy(), want[:top])
    if src.dim() == 2:  # the reference's expanded index
        assert _same(ops.scatter_mean(src, idx[:, None].expand_as(src), dim_size=case["S"]).cpu().numpy(), want)
        with pytest.raises(ValueError, match="not built"):
            ops.scatter_mean(src, idx, dim=1)
    else:
        assert _same(ops.scatter_mean(src, idx, dim=-1, dim_size=case["S"]).cpu().numpy(), want)
    for dt in (torch.float32, torch.float16, torch.bfloat16):  # ISBNet's function: float32 inside, the dtype back
        half = src.to(dt)
        got = ops.custom_scatter_mean(half, idx)
        w16 = ref.pool_forward_ref(half.float().cpu().numpy(), case["index"], top)[0]
        assert got.dtype == dt and _same(got.float().cpu().numpy(), torch.from_numpy(w16).to(dt).float().numpy())
    assert ops.custom_scatter_mean(src, idx, pool=False) is src
    assert ops.custom_scatter_mean(src.half(), idx, output_type=torch.float32).dtype == torch.float32


def _isbnet_inputs(case):
    n = len(case["index"])
    return [_dev(cases._feats(n, c, 50 + c)) for c in (3, 32, 6)]


def test_isbnet_spp_pool_without_a_host_read():
    import torch

    from gapro_amd import consumer_ops as ops

    case = cases.pool_cases()["batch_empty_sample"]
    S, idx, off = case["S"], _dev(case["index"]), _dev(case["batch_offsets"])
    feats = _isbnet_inputs(case)
    feats[1].requires_grad_(True)
    warm = ops.isbnet_spp_pool(*feats, idx, off, n_spps=S)  # the context and torch's kernels are warm
    warm[1].sum().backward()
    feats[1].grad = None
    g = torch.ones((S, 32), dtype=torch.float32, device=idx.device)
    torch.cuda.synchronize()
    with no_host_read():
        got = ops.isbnet_spp_pool(*feats, idx, off, n_spps=S, check=False)
        got[1].backward(g)
    for t, out in zip(feats, got[:3]):
        assert _same(out.detach().cpu().numpy(), ref.pool_forward_ref(t.detach().cpu().numpy(), case["index"], S)[0])
    assert _same(got[3].cpu().numpy(), ref.unique_loop(case["index"], case["batch_offsets"]))
    assert _same(feats[1].grad.cpu().numpy(),
                 ref.pool_backward_ref(np.ones((S, 32), np.float32), case["index"], S))
    with pytest.raises(RuntimeError):  # the guard is one: check=True reads the status
        with no_host_read():
            ops.isbnet_spp_pool(*feats, idx, off, n_spps=S, check=True)
    raw = ops.isbnet_spp_pool(*feats, idx, off, n_spps=S, use_spp_pool=False)
    assert all(a is b for a, b in zip(raw[:3], feats)) and _same(raw[3].cpu().numpy(), got[3].cpu().numpy())


@pytest.mark.parametrize("pool", ("mean", "max"))
def test_spformer_pool_without_a_host_read(pool):
    import torch

    from gapro_amd import consumer_ops as ops

    case = cases.pool_cases()["map_repeats"]
    S, R, N = case["S"], case["R"], len(case["index"])
    idx, v2p = _dev(case["index"]), _dev(case["point_map"], True)
    x = _dev(case["src"]).requires_grad_(True)
    cf, rgb = _dev(cases._feats(R, 3, 60)).requires_grad_(True), _dev(cases._feats(R, 3, 61))
    labels = [cases._feats(N, 1, 62 + k)[:, 0] for k in range(3)]
    dl = [_dev(t) for t in labels]
    ops.spformer_pool(x, cf, rgb, idx, v2p, *dl, pool=pool, n_spps=S)[0].sum().backward()
    x.grad = None
    g = cases.upstream(case)
    dg = _dev(g)
    torch.cuda.synchronize()
    with no_host_read():
        got = ops.spformer_pool(x, cf, rgb, idx, v2p, *dl, pool=pool, n_spps=S, check=False)
        got[0].backward(dg)
    assert len(got) == 6 and len(ops.spformer_pool(x, cf, rgb, idx, v2p, pool=pool, n_spps=S)) == 3
    srcs = [case["src"], cf.detach().cpu().numpy(), rgb.cpu().numpy()]
    arg = None
    for k, (out, src) in enumerate(zip(got[:3], srcs)):
        want, a = ref.pool_forward_ref(src, case["index"], S, pool, case["point_map"])
        arg = a if k == 0 else arg
        assert _same(out.detach().cpu().numpy(), want), k
    for out, src in zip(got[3:], labels):
        assert _same(out.cpu().numpy(), ref.pool_forward_ref(src, case["index"], S, pool)[0])
    assert _same(x.grad.cpu().numpy(), ref.pool_backward_ref(g, case["index"], S, pool, arg, case["point_map"], R))
    assert cf.grad is None and not any(t.requires_grad for t in got[1:])  # the gradient reaches x only


@pytest.mark.parametrize("name", cases.BAD_NAMES)
def test_bad_indices_raise_or_leave_the_other_segments_exact(name):
    from gapro_amd._lib import GaproError

    case = cases.bad_cases()[name]
    want = _plan_want(("bad", name), case)
    assert want["flags"]
    with pytest.raises(GaproError) as err:
        _plan(case, check=True)
    assert err.value.code == ref.BAD_ARG
    plan = _plan(case, check=False)
    _check_plan(plan, want)
    _check_pools(("bad", name), case, plan)


def test_against_the_index_add_statement_on_the_device():
    import torch

    from gapro_amd import consumer_ops as ops

    for name in ("segment_lengths", "n4097", "map_shared_rows"):
        case = cases.pool_cases()[name]
        S, pm = case["S"], case.get("point_map")
        x, idx = _dev(case["src"]), _dev(case["index"])
        x2 = x.reshape(x.shape[0], -1)
        rows = x2 if pm is None else x2[_dev(pm)]
        sums = torch.zeros((S, x2.shape[1]), dtype=torch.float32, device=x.device).index_add_(0, idx, rows)
        stated = sums / torch.bincount(idx, minlength=S).clamp(min=1)[:, None].float()
        got = ops.superpoint_pool(x, _plan(case)).reshape(S, -1)
        err = (got.double() - stated.double()).abs().cpu().numpy()
        bound = ref.sum_bound(case["src"], case["index"], S, pm)
        print("%s: largest error / bound %.3g" % (name, (err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), name


def test_composed_chain_voxelise_pool_loss_backward():
    """voxelization_idx -> voxelization -> spformer_pool -> a scalar loss -> backward() on a 300-point scene of two
    samples, against the same chain restated in NumPy."""
    import voxelize_ref as vref

    from gapro_amd import consumer_ops as ops

    rng = np.random.default_rng(314)
    N, S = 300, 10
    coords = np.concatenate([np.repeat([0, 1], 150)[:, None], rng.integers(0, 5, (N, 3))], axis=1).astype(np.int64)
    spps = np.concatenate([rng.integers(0, 5, 150), rng.integers(5, 10, 150)]).astype(np.int64)
    feats, xyz, rgb = cases._feats(N, 6, 70), cases._feats(N, 3, 71), cases._feats(N, 3, 72)
    w = cases._feats(S, 6, 73)
    _, v2p, p2v = ops.voxelization_idx(_dev(coords), 2)
    d_feats = _dev(feats).requires_grad_(True)
    vox = [ops.voxelization(t, p2v, 4) for t in (d_feats, _dev(xyz), _dev(rgb))]
    pooled = ops.spformer_pool(*vox, _dev(spps), v2p, n_spps=S)
    (pooled[0] * _dev(w)).sum().backward()
    _, im, om, _ = vref.voxelize_idx_ref(coords, 4)
    assert _same(v2p.cpu().numpy(), im) and _same(p2v.cpu().numpy(), om)
    M = om.shape[0]
    want_vox = [vref.pool_forward_ref(t, om, 4) for t in (feats, xyz, rgb)]
    for got, src in zip(pooled, want_vox):
        assert _same(got.detach().cpu().numpy(), ref.pool_forward_ref(src, spps, S, "mean", im)[0])
    d_vox = ref.pool_backward_ref(w, spps, S, "mean", None, im, M)  # the product's gradient is w itself
    assert _same(d_feats.grad.cpu().numpy(), vref.pool_backward_ref(d_vox, om, N, 4))
