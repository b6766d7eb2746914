"""gapro_voxelize_count / _fill and gapro_voxel_pool_forward / _backward on the MI355X: ``voxelization_idx`` and
``voxelization`` of consumer_ops on every case of tests/voxelize_cases.py against the NumPy restatement
tests/voxelize_ref.py, and the device path against the host path.

Everything is compared BIT FOR BIT: the indexing is integer work, and the pooling is float32 arithmetic whose every
operation is rounded on its own on both sides, so there is no tolerance.  The restatement restates the reference's
source; it is not a run of it.
"""
import contextlib

import numpy as np
import pytest

import voxelize_cases as cases
import voxelize_ref as ref

pytestmark = pytest.mark.gpu

_REF = {}  # key -> the restatement's answer, computed once and left unchanged


def _want(key, fn):
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


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


def _run_device(case):
    from gapro_amd import consumer_ops as ops

    out = ops.voxelization_idx(_dev(case["coords"]), 4, case["mode"])
    assert all(t.is_cuda for t in out)
    return tuple(t.cpu().numpy() for t in out)


def _run_host(case):
    import torch

    from gapro_amd import consumer_ops as ops

    return tuple(t.numpy() for t in ops.voxelization_idx(torch.from_numpy(case["coords"].copy()), 4, case["mode"]))


def _collision_case():
    from gapro_amd import consumer_ops as ops

    return _want("collision", lambda: cases.collision_case(ops.voxelize_plan, ops.voxelize_hash))


def _check_index_case(name, case):
    from gapro_amd._lib import GaproError

    try:
        oc, im, om, flags = _want(("idx", name), lambda: ref.voxelize_idx_ref(case["coords"], case["mode"]))
    except ref.Refused:
        with pytest.raises(ValueError):
            _run_device(case)
        return
    if flags:
        with pytest.raises(GaproError) as err:
            _run_device(case)
        assert err.value.code == ref.BAD_ARG
        return
    got_oc, got_im, got_om = _run_device(case)
    assert _same(got_im, im) and _same(got_oc, oc) and _same(got_om, om)
    host = _run_host(case)
    assert all(_same(g, h) for g, h in zip((got_oc, got_im, got_om), host))  # the device path against the host path


@pytest.mark.parametrize("name", cases.INDEX_NAMES)
def test_device_path_equals_the_restatement_and_the_host_path(name):
    _check_index_case(name, cases.index_cases()[name])


def test_colliding_keys():
    _check_index_case("collision", _collision_case())


def test_two_runs_give_identical_bytes():
    for case in (_collision_case(), cases.index_cases()["one_voxel_1025"], cases.index_cases()["max_active_at_cap"]):
        one, two = _run_device(case), _run_device(case)
        assert all(_same(a, b) for a, b in zip(one, two))


def _pool_inputs(c):
    return _dev(c["feats"]), _dev(c["map_rule"])


@pytest.mark.parametrize("name", cases.POOL_NAMES)
def test_pool_forward_and_backward_bit_for_bit(name):
    import torch

    from gapro_amd import consumer_ops as ops
    from gapro_amd._lib import GaproError

    c = cases.pool_cases()[name]
    N, C = c["feats"].shape
    flags = ref.pool_flags(c["map_rule"], N)
    want = _want(("fwd", name), lambda: ref.pool_forward_ref(c["feats"], c["map_rule"], c["mode"]))
    feats, rule = _pool_inputs(c)
    feats.requires_grad_(True)
    if flags:
        with pytest.raises(GaproError) as err:
            ops.voxelization(feats, rule, c["mode"], check=True)
        assert err.value.code == ref.BAD_ARG
    out = ops.voxelization(feats, rule, c["mode"], check=not flags, n_points=N)
    got = out.detach().cpu().numpy()
    assert _same(got, want), np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:8]
    if flags & ref.POOL_TWICE:
        return  # the backward's contract is a table that lists a point at most once
    d_out = cases._feats(want.shape[0], C, 99)
    want_back = _want(("bwd", name), lambda: ref.pool_backward_ref(d_out, c["map_rule"], N, c["mode"]))
    out.backward(_dev(d_out))
    assert _same(feats.grad.cpu().numpy(), want_back)
    assert rule.grad is None and not torch.isnan(feats.grad).any()


def test_pool_discriminates_the_three_conventions():
    from gapro_amd import consumer_ops as ops

    x, table = cases.three_way_row()
    got = ops.voxelization(_dev(x), _dev(table), 4).cpu().numpy()
    assert _same(got, ref.pool_forward_ref(x, table, 4))
    for wrong in ("fused", "divide"):
        assert not _same(got, ref.pool_forward_ref(x, table, 4, convention=wrong))
    neg = cases.pool_cases()["negative_zero"]
    zero = ops.voxelization(*_pool_inputs(neg), 4, check=False).cpu().numpy()  # its table lists points twice
    assert not np.signbit(zero[:2]).any() and zero[0, 0] == 0 and (zero[1] == 0).all()  # -0.0 alone gives +0.0


def test_autograd_wiring_through_sum_backward():
    import torch

    from gapro_amd import consumer_ops as ops

    c = cases.index_cases()["random_1025"]
    coords = _dev(c["coords"])
    _, v2p, p2v = ops.voxelization_idx(coords, 1)  # the reference's names: v2p the voxel of a point, p2v the table
    feats = _dev(cases._feats(1025, 6, 98)).requires_grad_(True)
    ops.voxelization(feats * 1.0, p2v, 4).sum().backward()  # through a non-leaf, as coords_float in a model
    counts = p2v[:, 0].cpu().numpy()
    mult = (np.float32(1.0) / counts.astype(np.float32))[v2p.cpu().numpy()]
    assert _same(feats.grad.cpu().numpy(), np.repeat(mult[:, None], 6, axis=1))
    empty = ops.voxelization(feats, torch.zeros((0, 4), dtype=torch.int32, device=feats.device))
    assert empty.shape == (0, 6)


def test_check_false_makes_no_host_read():
    import torch

    from gapro_amd import consumer_ops as ops

    c = cases.pool_cases()["many_voxels"]
    feats, rule = _pool_inputs(c)
    feats.requires_grad_(True)
    want = _want(("fwd", "many_voxels"), lambda: ref.pool_forward_ref(c["feats"], c["map_rule"], c["mode"]))
    ops.voxelization(feats, rule, 4, check=False).sum().backward()  # the context and torch's kernels are warm
    feats.grad = None
    grad = torch.ones(want.shape, dtype=torch.float32, device=feats.device)
    torch.cuda.synchronize()
    with no_host_read():
        out = ops.voxelization(feats, rule, 4, check=False)
        out.backward(grad)
    assert _same(out.detach().cpu().numpy(), want) and feats.grad is not None
    with pytest.raises(RuntimeError):  # the guard is one: check=True reads the status
        with no_host_read():
            ops.voxelization(feats, rule, 4, check=True)
    bad = cases.pool_cases()["bad_indices"]
    feats, rule = _pool_inputs(bad)
    torch.cuda.synchronize()
    with no_host_read():
        out = ops.voxelization(feats, rule, 4, check=False)  # flagged entries are skipped, nothing is read back
    assert _same(out.cpu().numpy(), ref.pool_forward_ref(bad["feats"], bad["map_rule"], 4))
