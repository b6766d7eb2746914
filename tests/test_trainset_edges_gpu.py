"""The training-set assembly of the point-level fits (csrc/trainset.hip) at its kernel edges on the MI355X: every case of
tests/trainset_cases.py through gp_train_sets against the NumPy restatement (tests/fit_gp_ref.py), bit for bit -- row
counts, `sel`, order and rows with np.array_equal, no tolerance anywhere.  tests/test_trainset_edges_cpu.py asserts that
each case meets the condition it was built for; no fit is run here."""
import ctypes as C

import numpy as np
import pytest

import trainset_cases as tc

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- pool
@pytest.mark.parametrize("d", tc.POOL_WIDTHS)
def test_pool_feature_widths_and_both_accumulate_branches(d):
    """k_ts_accum: the count lane D % 8 at every residue the widths give, whole waves of one superpoint, waves whose vote
    fails at each of the eight positions, partial last waves, and 2 N entries over three rounds of the grid."""
    case = tc.pool_width_case(d)
    got = case.run()
    tc.check(case, got)
    assert got[0][1] == 1 and got[5][1] == 2  # "one n=1": one row; "other at 0 n=7": two


def test_pool_rounds_fixed_point_and_mean_ties_to_even():
    case = tc.pool_rounding_case()
    got = case.run()
    tc.check(case, got)
    x, m1, m2, s1, s2 = got[0]
    for side, sid, lo, hi, even in case.info["mean_ties"]:
        rows, sel = (x[:m1], s1) if side == 0 else (x[m1:], s2)
        assert rows[list(sel).index(sid), 1] == np.float32(even)


@pytest.mark.parametrize("s", tc.RANK_S)
def test_pool_rank_scan_at_its_round_edges(s):
    case = tc.rank_case(s)
    got = case.run()
    tc.check(case, got)
    ids = np.unique(case.spp)
    for i, ranks in enumerate(case.info["rank_sets"]):
        assert np.array_equal(got[i // 2][3 + i % 2], ids[ranks])


@pytest.mark.parametrize("n,kind", tc.HEADROOM)
def test_pool_sums_of_two_n_largest_terms(n, kind):
    case = tc.headroom_case(n, kind)
    got = case.run()
    tc.check(case, got)
    fmax = np.float32(case.info["fmax"])
    assert np.array_equal(got[0][0][0, :2], [fmax, -fmax])


def test_pool_ragged_batch_of_three_hundred_problems():
    case = tc.ragged_case()
    tc.check(case, case.run())


# ---------------------------------------------------------------------------------------------- nearest
def test_nearest_every_radix_pass_decides_and_bins_0_and_255_are_chosen():
    case = tc.radix_case()
    tc.check(case, case.run())


@pytest.mark.parametrize("k", [1024, 100])
def test_nearest_tie_groups_across_wave_and_collect_round_edges(k):
    case = tc.tie_case(k)
    tc.check(case, case.run())


@pytest.mark.parametrize("k", tc.SIZE_K)
def test_nearest_sizes_long_and_copied_sides(k):
    case = tc.size_case(k)
    got = case.run()
    tc.check(case, got)
    assert [(g[1], g[2]) for g in got] == [(min(a, k), min(b, k)) for a, b in case.info["kinds"]]


@pytest.mark.parametrize("scale", tc.CENTROID_SCALES)
def test_nearest_centroid_grids_wrap_and_scales(scale):
    case = tc.centroid_case(scale)
    tc.check(case, case.run())


def test_nearest_distance_is_not_contracted():
    """Pairs that tie only when every operation of (dx dx + dy dy) + dz dz is rounded on its own: a fused multiply-add
    anywhere in the distance swaps rows or changes the row on the cut (asserted on the CPU for every way of fusing)."""
    case = tc.contraction_case()
    tc.check(case, case.run())


# ---------------------------------------------------------------------------------------------- host refusals of the fill
BAD_ARG, WORKSPACE = -1, -7


def _fill_arguments():
    """A legal nearest-mode gapro_trainset_fill of two problems at k = 4 and N = 12, every buffer on the device."""
    from gapro_amd import _lib
    from gapro_amd.gaussian_process_utils import _pipeline
    import torch

    pipe = _pipeline(torch.device("cuda:0"), 50)
    be, lib = pipe.be, pipe.lib
    n, d, k = 12, 3, 4
    rng = np.random.default_rng(12)
    sizes = [(6, 3, 2), (2, 9, 1)]
    descs = (_lib.TrainsetDesc * 2)()
    io = rows = 0
    for ds, (n1, n2, t) in zip(descs, sizes):
        ds.idx_offset, ds.n1, ds.n2, ds.t = io, n1, n2, t
        ds.m1, ds.m2, ds.row_offset = min(n1, k), min(n2, k), rows
        io += n1 + n2 + t
        rows += ds.m1 + ds.m2
    ws_bytes = int(lib.gapro_trainset_workspace_bytes(_lib.TRAINSET_NEAREST, C.cast(descs, C.c_void_p), 2, 1, d))
    assert ws_bytes == tc.workspace_layout(sizes, 1, d, pool=False)
    # the index array is long enough for the longest list any refused variant names: nothing is launched, but nothing
    # could leave the arrays either
    bufs = dict(coords=be.from_numpy(rng.normal(size=(n, 3))), feats=be.from_numpy(rng.normal(size=(n, d)).astype(np.float32)),
                spp=be.from_numpy(np.zeros(n, np.int64)), spp_inv=be.from_numpy(np.zeros(n, np.int32)),
                idx=be.from_numpy(rng.integers(0, n, 4 * n + io).astype(np.int32)), ws=be.empty(ws_bytes),
                d_descs=be.empty(2 * C.sizeof(_lib.TrainsetDesc)), train=be.empty(4 * (rows + 8) * d),
                sel=be.empty(8 * (rows + 8)), status=be.empty(8))
    return pipe, descs, bufs, dict(n=n, d=d, k=k, rows=rows, ws_bytes=ws_bytes, mode=_lib.TRAINSET_NEAREST)


def _fill(pipe, descs, bufs, a):
    from gapro_amd.fit_runner import _ptr

    return pipe.lib.gapro_trainset_fill(
        pipe.ctx.handle, pipe._sh(), a["mode"], 2, a["d"], C.cast(descs, C.c_void_p), _ptr(bufs["d_descs"]), a["n"], 1,
        _ptr(bufs["coords"]), _ptr(bufs["feats"]), _ptr(bufs["spp"]), _ptr(bufs["spp_inv"]), 0, a["k"], _ptr(bufs["idx"]),
        _ptr(bufs["ws"]), a["ws_bytes"], a["rows"], _ptr(bufs["train"]), _ptr(bufs["sel"]), _ptr(bufs["status"]))


def _edit(field, value, problem=0):
    def apply(descs, a):
        setattr(descs[problem], field, value)
    return apply


def _arg(name, value):
    def apply(descs, a):
        a[name] = value
    return apply


REFUSALS = [
    ("npoint_nearest 0", _arg("k", 0), BAD_ARG),
    ("npoint_nearest 1025", _arg("k", 1025), BAD_ARG),
    ("m1 below min(n1, k)", _edit("m1", 3), BAD_ARG),
    ("m1 above min(n1, k)", _edit("m1", 5), BAD_ARG),
    ("m2 of a copied side", _edit("m2", 4, problem=0), BAD_ARG),
    ("a row_offset that leaves the table", _edit("row_offset", 8, problem=1), BAD_ARG),  # 8 + 2 + 4 > 13
    ("a negative row_offset", _edit("row_offset", -1), BAD_ARG),
    ("a list of 2 N + 1 entries", _edit("n2", 25, problem=1), BAD_ARG),
    ("an intersection of 2 N + 1 entries", _edit("t", 25, problem=1), BAD_ARG),
    ("T = 0 with a long side", _edit("t", 0), BAD_ARG),
    ("a workspace one byte short", lambda descs, a: a.__setitem__("ws_bytes", a["ws_bytes"] - 1), WORKSPACE),
]


@pytest.mark.parametrize("name,change,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_fill_refuses_on_the_host_with_a_message(name, change, code):
    """Each of these is refused before anything is launched; the context holds a message that names the call."""
    pipe, descs, bufs, a = _fill_arguments()
    with pipe.be.device_ctx():
        assert _fill(pipe, descs, bufs, a) == 0  # the unchanged call is legal ...
        pipe.be.current_stream().synchronize()
        from gapro_amd.fit_runner import _host

        assert not _host(bufs["status"]).view(np.int32).any()
        change(descs, a)
        assert _fill(pipe, descs, bufs, a) == code, name
        msg = (pipe.lib.gapro_last_error(pipe.ctx.handle) or b"").decode()
        assert "gapro_trainset_fill" in msg, (name, msg)
        if code == WORKSPACE:
            assert "workspace" in msg
