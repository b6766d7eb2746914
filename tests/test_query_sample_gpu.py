"""gapro_fps_batch / gapro_ball_query_batch on the MI355X: the five public functions of consumer_ops (query sampling)
on every case of tests/query_sample_cases.py against the NumPy restatement tests/query_sample_ref.py.

Indices, counts and the returned running minima are compared BIT FOR BIT: everything is integer work or float32
arithmetic whose every operation is rounded on its own on both sides, so there is no tolerance.  The restatement
restates the source of the reference's CUDA kernels; it is not a run of them.
"""
import contextlib

import numpy as np
import pytest

import query_sample_cases as cases
import query_sample_ref as ref

pytestmark = pytest.mark.gpu

_REF = {}  # case name -> the restatement's answer, computed once and left unchanged


def _tables():
    from gapro_amd import consumer_ops as ops

    if "fps" not in _REF:
        _, xyz_capacity, capacity = ops.fps_plan(0)
        _REF["fps"] = cases.fps_cases(xyz_capacity, capacity)
        _REF["ball"] = cases.ball_cases()
    return _REF["fps"], _REF["ball"]


# the names are fixed by the cases file, not by the capacities: collected without the library
FPS_NAMES = sorted(cases.fps_cases(16, 64))
BALL_NAMES = sorted(cases.ball_cases())


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _want(kind, name, fn):
    key = (kind, name)
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


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


def _fps_run(c, **kw):
    from gapro_amd import consumer_ops as ops

    if c["form"] == "fps_batched":
        return ops.furthest_point_sample(_dev(c["xyz"]), c["npoint"], **kw).cpu().numpy().reshape(-1), None
    out = ops.furthestsampling_batchflat(_dev(c["xyz"]), _dev(c["offset"]), _dev(c["new_offset"]), return_dist=True, **kw)
    return out[0].cpu().numpy(), out[1].cpu().numpy()


def _fps_want(name, c):
    if c["form"] == "fps_batched":
        B, N, _ = c["xyz"].shape
        return _want("fps", name, lambda: ref.fps_ref(c["xyz"], np.arange(1, B + 1) * N,
                                                      np.arange(1, B + 1) * c["npoint"], skip_origin=True,
                                                      local_index=True))
    return _want("fps", name, lambda: ref.fps_ref(c["xyz"], c["offset"], c["new_offset"]))


@pytest.mark.parametrize("name", FPS_NAMES)
def test_fps_case_equals_the_restatement(name):
    from gapro_amd._lib import GaproError

    c = _tables()[0][name]
    idx, minima, flags = _fps_want(name, c)
    assert flags == c["flags"]
    if flags:
        with pytest.raises(GaproError) as err:
            _fps_run(c)
        assert err.value.code == ref.status_of(flags)
    got_idx, got_min = _fps_run(c, check=False) if flags else _fps_run(c)
    written = idx != -2  # a sample refused for its offsets writes nothing
    assert got_idx.dtype == np.int32 and got_idx.shape == idx.shape
    assert np.array_equal(got_idx[written], idx[written])
    if got_min is not None and not flags & ref.FLAG_OFFSETS:  # refused offsets may make samples share points
        known = ~np.isnan(minima)
        assert got_min.dtype == np.float32 and got_min[known].tobytes() == minima[known].tobytes()
    again = _fps_run(c, check=False)[0]
    assert np.array_equal(again[written], got_idx[written])  # two runs give the same indices


def test_fps_discriminates_the_tie_rule_and_the_rounding():
    """The device agrees with the restatement where the two wrong variants do not."""
    fps = _tables()[0]
    got = _fps_run(fps["lattice"])[0]
    for block in (8, 64, 256):
        other = _want("tournament", block, lambda: ref.fps_ref(fps["lattice"]["xyz"], fps["lattice"]["offset"],
                                                               fps["lattice"]["new_offset"],
                                                               pick=ref.tournament(block))[0])
        assert got[2] != other[2]
    c = fps["random_5000"]
    fused = _want("fused", 0, lambda: ref.fps_ref(c["xyz"], c["offset"], c["new_offset"], dist=ref.sqdist_fused)[1])
    got_min = _fps_run(c)[1]
    assert 0.05 < np.mean(got_min.view(np.uint32) != fused.view(np.uint32)) < 0.5


def test_fps_n_sample_and_offset_dtypes_without_a_host_read():
    import torch

    from gapro_amd import consumer_ops as ops

    c = _tables()[0]["batch3"]
    xyz = _dev(c["xyz"])
    want = ref.fps_ref(c["xyz"], c["offset"], 11 * np.arange(1, 4))
    for dtype in (torch.int32, torch.int64):
        off = _dev(c["offset"]).to(dtype)
        ops.furthestsampling_batchflat(xyz, off, n_sample=11, check=False)  # the uniform table is made once
        torch.cuda.synchronize()
        with no_host_read():
            idx, minima = ops.furthestsampling_batchflat(xyz, off, n_sample=11, check=False, return_dist=True)
        assert idx.dtype == torch.int32 and not idx.requires_grad and not minima.requires_grad
        assert np.array_equal(idx.cpu().numpy(), want[0]) and minima.cpu().numpy().tobytes() == want[1].tobytes()
    with pytest.raises(RuntimeError):  # the guard is one: the other form reads new_offset's last entry
        with no_host_read():
            ops.furthestsampling_batchflat(xyz, _dev(c["offset"]), _dev(c["new_offset"]), check=False)


def _ball_run(c, **kw):
    from gapro_amd import consumer_ops as ops

    if c["form"] == "ball_batched":
        idx, counts = ops.ball_query(c["radius"], c["nsample"], _dev(c["xyz"]), _dev(c["new_xyz"]), return_counts=True)
        return idx.cpu().numpy().reshape(-1, c["nsample"]), counts.cpu().numpy().reshape(-1)
    idx, counts = ops.ballquery_batchflat(c["radius"], c["nsample"], _dev(c["xyz"]), _dev(c["new_xyz"]),
                                          _dev(c["offset"]), _dev(c["new_offset"]), return_counts=True, **kw)
    return idx.cpu().numpy(), counts.cpu().numpy()


def _ball_want(name, c):
    if c["form"] == "ball_batched":
        B, N, _ = c["xyz"].shape
        M = c["new_xyz"].shape[1]
        return _want("ball", name, lambda: ref.ball_ref(c["radius"], c["nsample"], c["xyz"], c["new_xyz"],
                                                        np.arange(1, B + 1) * N, np.arange(1, B + 1) * M,
                                                        local_index=True))
    return _want("ball", name, lambda: ref.ball_ref(c["radius"], c["nsample"], c["xyz"], c["new_xyz"], c["offset"],
                                                    c["new_offset"]))


@pytest.mark.parametrize("name", BALL_NAMES)
def test_ball_query_case_equals_the_restatement(name):
    from gapro_amd._lib import GaproError

    c = _tables()[1][name]
    idx, counts, flags = _ball_want(name, c)
    assert flags == c["flags"]
    if flags:
        with pytest.raises(GaproError) as err:
            _ball_run(c)
        assert err.value.code == ref.status_of(flags)
    got_idx, got_counts = _ball_run(c, check=False) if flags else _ball_run(c)
    assert got_idx.dtype == np.int32 and np.array_equal(got_idx, idx)
    assert got_counts.dtype == np.int32 and np.array_equal(got_counts, counts)


def test_ball_query_defaults_and_no_host_read():
    import torch

    from gapro_amd import consumer_ops as ops

    c = _tables()[1]["no_leak"]
    xyz, off = _dev(c["xyz"]), _dev(c["offset"])
    want = _ball_want("no_leak", c)[0]
    torch.cuda.synchronize()
    with no_host_read():
        own = ops.ballquery_batchflat(c["radius"], c["nsample"], xyz, None, off, check=False)  # new_xyz=None: xyz
    assert np.array_equal(own.cpu().numpy(), want) and not own.requires_grad
    # n_sample=: 85 queries a sample, of two samples of 80 and 90 points
    q = np.concatenate([c["xyz"][:85], c["xyz"][80:165]])
    d_q = _dev(q)
    ops.ballquery_batchflat(c["radius"], 8, xyz, d_q, off, n_sample=85, check=False)
    torch.cuda.synchronize()
    with no_host_read():
        got = ops.ballquery_batchflat(c["radius"], 8, xyz, d_q, off, n_sample=85, check=False)
    assert np.array_equal(got.cpu().numpy(), ref.ball_ref(c["radius"], 8, c["xyz"], q, c["offset"], [85, 170])[0])


def test_sample_queries_is_the_three_calls():
    import torch

    from gapro_amd import consumer_ops as ops

    c = cases.sample_queries_case()
    locs, off = _dev(c["locs"]).requires_grad_(True), _dev(c["batch_offsets"])
    B, n_sample, r = c["batch_size"], c["n_sample"], c["radius"]
    args = (B, n_sample, r, c["n_neighbor"], c["n_neighbor_post"])
    ops.sample_queries(locs, off, *args)  # the uniform tables are made once
    torch.cuda.synchronize()
    with no_host_read():
        fps, near, post = ops.sample_queries(locs, off, *args)
    assert fps.shape == (B * n_sample,) and near.shape == (B * n_sample, c["n_neighbor"])
    assert post.shape == (B, n_sample, c["n_neighbor_post"])
    assert all(t.dtype == torch.int32 and not t.requires_grad for t in (fps, near, post))
    new = torch.arange(0, n_sample * (B + 1), n_sample, dtype=torch.int32, device=off.device)
    one = ops.furthestsampling_batchflat(locs, off, new)  # the reference's tables, leading 0 and all
    picked = locs.detach()[one.long()]
    two = ops.ballquery_batchflat(r, c["n_neighbor"], locs, picked, off, new)
    three = ops.ball_query(2 * r, c["n_neighbor_post"], picked.view(B, n_sample, 3), picked.view(B, n_sample, 3))
    assert torch.equal(fps, one) and torch.equal(near, two) and torch.equal(post, three)
    want = ref.fps_ref(c["locs"], c["batch_offsets"], new.cpu().numpy())[0]
    assert np.array_equal(fps.cpu().numpy(), want)
    q = c["locs"][want]
    assert np.array_equal(near.cpu().numpy(), ref.ball_ref(r, c["n_neighbor"], c["locs"], q, c["batch_offsets"],
                                                           new.cpu().numpy())[0])
    assert np.array_equal(post.cpu().numpy().reshape(B * n_sample, -1),
                          ref.ball_ref(2 * r, c["n_neighbor_post"], q, q, n_sample * np.arange(1, B + 1),
                                       n_sample * np.arange(1, B + 1), local_index=True)[0])
