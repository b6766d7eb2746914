"""Superpoint pooling without a device: the restatement tests/spp_pool_ref.py against hand-checked answers, every wrong
convention against the case that catches it, the restatement against torch's CPU statement and a float64 run within
the derived bound of two float32 sums, the header's declarations against the bindings, and every refusal the Python
layer makes before it touches a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import spp_pool_cases as cases
import spp_pool_ref as ref
from gapro_amd import _lib, consumer_ops as ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the restatement by hand ---------------------------------------------------------------------------------------------
def test_restatement_against_hand_checked_answers():
    index = np.array([2, 0, 2, 2, 0, 4], dtype=np.int64)
    x = np.array([[1, 10], [2, 20], [3, 30], [5, 50], [4, 40], [-7, 0.5]], dtype=F32)
    mean, none = ref.pool_forward_ref(x, index, 6)
    assert none is None and _same(mean, np.array([[3, 30], [0, 0], [3, 30], [0, 0], [-7, 0.5], [0, 0]], dtype=F32))
    best, arg = ref.pool_forward_ref(x, index, 6, "max")
    assert _same(best, np.array([[4, 40], [0, 0], [5, 50], [0, 0], [-7, 0.5], [0, 0]], dtype=F32))
    assert arg.dtype == np.int64 and arg.tolist() == [[4, 4], [6, 6], [3, 3], [6, 6], [5, 5], [6, 6]]
    g = np.array([[2, 4], [9, 9], [3, 6], [9, 9], [1, 1], [9, 9]], dtype=F32)
    assert _same(ref.pool_backward_ref(g, index, 6), np.array([[1, 2], [1, 2], [1, 2], [1, 2], [1, 2], [1, 1]], dtype=F32))
    want = np.zeros((6, 2), dtype=F32)
    want[[4, 3, 5]] = g[[0, 2, 4]]
    assert _same(ref.pool_backward_ref(g, index, 6, "max", arg), want)
    # through a map: rows 0 and 2 are read, row 1 by nobody, row 2 by points of the segments 2 and 4
    pm = np.array([0, 0, 2, 2, 0, 2], dtype=np.int64)
    rows = np.array([[8], [99], [2]], dtype=F32)
    mapped, _ = ref.pool_forward_ref(rows, index, 6, point_map=pm)
    assert mapped[:, 0].tolist() == [8, 0, 4, 0, 2, 0]  # segment 2 reads rows 0, 2, 2
    back = ref.pool_backward_ref(g[:, :1], index, 6, point_map=pm, R=3)
    assert back[:, 0].tolist() == [3, 0, 3]  # rows: 1 + 1 + 1, nothing, 1 + 1 + 1
    plan = ref.plan_ref(index, 6, pm, 3, batch_offsets=[0, 2, 2, 6])
    assert plan["seg_off"].tolist() == [0, 2, 2, 5, 5, 6, 6] and plan["seg_pts"].tolist() == [1, 4, 0, 2, 3, 5]
    assert plan["counts"].tolist() == [2, 0, 3, 0, 1, 0] and plan["seg_rows"].tolist() == [0, 0, 0, 2, 2, 2]
    assert plan["row_off"].tolist() == [0, 3, 3, 6] and plan["row_pts"].tolist() == [0, 1, 4, 2, 3, 5]
    assert plan["spp_batch_offsets"].tolist() == [0, 2, 2, 3] and plan["flags"] == 0  # first points 1, 0 | - | 5
    assert plan["spp_batch_offsets"].dtype == np.int64 and plan["seg_off"].dtype == np.int32
    z = cases.pool_cases()["negative_zero"]
    out, _ = ref.pool_forward_ref(z["src"], z["index"], z["S"])
    assert not np.signbit(out[:3]).any() and out.tolist() == [0, 0, 0, 1]


def test_a_flagged_point_is_left_out_of_everything():
    for name, case in cases.bad_cases().items():
        pm, R, S = case.get("point_map"), case.get("R"), case["S"]
        plan = ref.plan_ref(case["index"], S, pm, R)
        bad = np.flatnonzero(~ref._listed(case["index"], S, pm, R))
        assert len(bad) == 1 and plan["flags"] == (ref.FLAG_MAP if pm is not None else ref.FLAG_INDEX), name
        assert plan["seg_off"][-1] == len(case["index"]) - 1 and plan["seg_pts"][-1] == bad[0]
        assert plan["counts"].sum() == len(case["index"]) - 1
        grad = ref.pool_backward_ref(cases.upstream(case), case["index"], S, point_map=pm, R=R)
        if pm is None:
            assert not grad[bad[0]].any() and grad[bad[0] - 1].any()


# ---- each wrong convention against the case that catches it -------------------------------------------------------------
def test_every_wrong_convention_is_caught_by_its_case():
    c = cases.pool_cases()["three_way"]
    got = {k: ref.pool_forward_ref(c["src"], c["index"], 1, convention=k)[0].tobytes()
           for k in (None, "reversed", "tree", "reciprocal")}
    assert len(set(got.values())) == 4
    m = cases.pool_cases()["max_edges"]
    right = ref.pool_forward_ref(m["src"], m["index"], m["S"], "max")
    assert right[1][:, 0].tolist() == [0, 4, 6, 8, 10, 12, 15, 17, 16]
    assert np.isnan(right[0][[4, 6], 0]).all() and right[0][5, 0] == 1 and not np.signbit(right[0][2, 0])
    assert np.signbit(right[0][3, 0]) and (right[1][7] == len(m["index"])).all() and not right[0][7].any()
    tie = ref.pool_forward_ref(m["src"], m["index"], m["S"], "max", convention="last_tie")[1]
    assert tie[:4, 0].tolist() == [2, 5, 7, 9]  # the highest index of every tie, +0.0 against -0.0 included
    nan = ref.pool_forward_ref(m["src"], m["index"], m["S"], "max", convention="nan")
    assert nan[1][5, 0] == 13 and np.isnan(nan[0][5, 0])
    s = cases.shared_row_case()
    kw = dict(point_map=s["point_map"], R=s["R"])
    assert not _same(ref.pool_backward_ref(s["g"], s["index"], s["S"], **kw),
                     ref.pool_backward_ref(s["g"], s["index"], s["S"], convention="by_segment", **kw))


def test_cases_cover_what_the_issue_lists():
    cs = cases.pool_cases()
    sizes = {len(c["index"]) for c in cs.values()}
    assert {1, 63, 64, 65, 255, 256, 257, cases.TILE - 1, cases.TILE, cases.TILE + 1} <= sizes
    assert cases.TILE == _lib.SPP_SORT_TILE
    chans = {(c["src"].shape[1] if c["src"].ndim == 2 else 0) for c in cs.values()}
    assert {0, 1, 3, 6, 32, 33} <= chans
    counts = np.bincount(cs["segment_lengths"]["index"], minlength=len(cases.LENGTHS))
    assert tuple(counts) == cases.LENGTHS and np.bincount(cs["segment_70000"]["index"]).max() >= 70000
    assert cs["third_pass"]["index"].max() >= 65536 and set(cs["second_byte"]["index"] & 255) == {3}
    e = cs["empty_segments"]
    assert e["S"] > e["index"].max() + 1 and 1 not in e["index"]
    u = cs["map_unread_rows"]
    assert len(np.unique(u["point_map"])) < u["R"]
    sh = cs["map_shared_rows"]
    assert any(len(set(sh["index"][sh["point_map"] == r])) > 1 for r in range(sh["R"]))
    assert (np.diff(cs["batch_empty_sample"]["batch_offsets"]) == 0).any()
    assert any(c.get("i32") for c in cs.values()) and not all(c.get("i32") for c in cs.values())


# ---- against torch on the CPU and a float64 run --------------------------------------------------------------------------
_CPU_NAMES = ("n257", "segment_lengths", "n4097", "map_shared_rows", "map_repeats", "empty_segments")


def _torch_statement(case, dtype):
    """scatter_mean as the reference states it: scatter_add_ / index_add_, the count clamped to 1, a true division, the
    gradient by autograd."""
    S, pm = case["S"], case.get("point_map")
    x = torch.from_numpy(case["src"]).to(dtype).requires_grad_(True)
    idx = torch.from_numpy(case["index"])
    rows = x if pm is None else x[torch.from_numpy(pm)]
    sums = torch.zeros((S, x.shape[1]), dtype=dtype).index_add_(0, idx, rows)
    out = sums / torch.bincount(idx, minlength=S).clamp(min=1)[:, None].to(dtype)
    out.backward(torch.from_numpy(cases.upstream(case)).to(dtype))
    return out.detach().numpy(), x.grad.numpy()


@pytest.mark.parametrize("name", _CPU_NAMES)
def test_restatement_against_torch_float32_and_float64(name):
    case = cases.pool_cases()[name]
    S, pm, R = case["S"], case.get("point_map"), case.get("R")
    g = cases.upstream(case)
    out, _ = ref.pool_forward_ref(case["src"], case["index"], S, point_map=pm)
    back = ref.pool_backward_ref(g, case["index"], S, point_map=pm, R=R)
    bound = ref.sum_bound(case["src"], case["index"], S, pm)
    # the gradient: d_point = g / n, one rounding on either side; through a map a row's sum of those
    n = np.maximum(np.bincount(case["index"], minlength=S), 1)
    d_abs = np.abs(g.astype(np.float64)) / n[:, None]
    if pm is None:
        back_bound = 2 * 2.0 ** -24 * d_abs[case["index"]]
    else:
        back_bound = ref.sum_bound(d_abs[case["index"]].astype(F32), pm, R) * np.maximum(np.bincount(pm, minlength=R), 1)[:, None]
        back_bound += 4 * 2.0 ** -24 * np.abs(back)
    for dtype in (torch.float32, torch.float64):
        t_out, t_back = _torch_statement(case, dtype)
        err = np.abs(out.astype(np.float64) - t_out.astype(np.float64))
        berr = np.abs(back.astype(np.float64) - t_back.astype(np.float64))
        print("%s %s: forward bits equal %s, largest error / bound %.3g; backward bits equal %s"
              % (name, dtype, _same(out, t_out), (err / np.maximum(bound, 1e-300)).max(), _same(back, t_back)))
        assert (err <= bound).all() and (berr <= back_bound).all(), dtype


# ---- the bindings --------------------------------------------------------------------------------------------------------
def test_header_declarations_match_the_bindings():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "gapro_hip.h")).read()
    assert "Superpoint pooling" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)  # the declarations without their comments
    names = ("gapro_spp_plan_workspace_bytes", "gapro_spp_plan_build", "gapro_spp_pool_forward",
             "gapro_spp_pool_backward")
    for n in names:
        assert hasattr(lib, n) and n in _lib.SIGNATURES
        decl = re.search(r"\b%s\(([^;]*)\);" % n, code).group(1)
        params = [p for p in decl.split(",") if p.strip()]
        assert len(params) == len(_lib.SIGNATURES[n][1]), n
        for p, t in zip(params, _lib.SIGNATURES[n][1]):
            if "*" in p:
                assert t is C.c_void_p, (n, p)
            else:
                want = {"int64_t": C.c_int64, "int32_t": C.c_int32, "size_t": C.c_size_t}[p.split()[0]]
                assert t is want, (n, p)
    for macro, value in (("SORT_TILE", _lib.SPP_SORT_TILE), ("MAX_BATCHES", _lib.SPP_MAX_BATCHES),
                         ("STATUS_WORDS", _lib.SPP_STATUS_WORDS), ("FLAG_INDEX", _lib.SPP_FLAG_INDEX),
                         ("FLAG_MAP", _lib.SPP_FLAG_MAP), ("MEAN", _lib.SPP_MEAN), ("MAX", _lib.SPP_MAX)):
        assert int(re.search(r"#define GAPRO_SPP_%s (\d+)" % macro, text).group(1)) == value, macro
    assert re.search(r"#define GAPRO_SPP_MAX_SEGMENTS \(1 << 24\)", text) and _lib.SPP_MAX_SEGMENTS == 1 << 24
    body = re.search(r"typedef struct gapro_spp_plan \{(.*?)\} gapro_spp_plan;", text, re.S).group(1)
    fields = [f.split()[-1] for f in re.sub(r"/\*.*?\*/", "", body).split(";") if f.strip()]
    assert fields == [f[0] for f in _lib.SppPlan._fields_]
    assert C.sizeof(_lib.SppPlan) == 3 * 8 + 2 * 8 + 2 * 4 + 6 * 8
    import gapro_amd
    for n in ("superpoint_plan", "superpoint_pool", "scatter_mean", "scatter_max", "custom_scatter_mean",
              "isbnet_spp_pool", "spformer_pool"):
        assert n in gapro_amd.__all__ and getattr(gapro_amd, n) is getattr(ops, n)


def test_workspace_bytes_and_the_library_bounds():
    lib = _lib.load()
    small, large = lib.gapro_spp_plan_workspace_bytes(1, 0), lib.gapro_spp_plan_workspace_bytes(2400000, 12)
    assert 0 < small < large and small % 256 == 0 and large % 256 == 0
    assert lib.gapro_spp_plan_workspace_bytes(2 ** 31 - 1, 0) > 3 * 4 * (2 ** 31 - 1)
    for bad in ((0, 0), (-1, 0), (2 ** 31, 0), (10, -1), (10, _lib.SPP_MAX_BATCHES + 1)):
        assert lib.gapro_spp_plan_workspace_bytes(*bad) == 0, bad
    # a null context or a plan beyond the bounds is refused before anything is touched
    assert lib.gapro_spp_plan_build(None, None, None, 0, None, 0, None, None, 0, None, None) == _lib.GAPRO_ERR_BAD_ARG


# ---- the refusals that need no device ------------------------------------------------------------------------------------
def test_superpoint_plan_refuses_before_a_device_is_touched():
    idx = torch.zeros(5, dtype=torch.int64)

    def r(match, *a, **kw):
        with pytest.raises(ValueError, match=match):
            ops.superpoint_plan(*a, **kw)

    for bad in (idx.float(), idx[:, None], [0, 1], idx.bool()):
        r("superpoints must be a 1-D integer tensor", bad, n_spps=3)
    for bad in (0, -1, 1.0, True):
        r("n_spps must be a positive int", idx, n_spps=bad)
    r("beyond the library's bounds", idx, n_spps=2 ** 24 + 1)
    r("beyond the library's bounds", idx, n_spps=3, point_map=idx, n_rows=2 ** 24 + 1)
    r("point_map must be a 1-D integer tensor", idx, n_spps=3, point_map=idx.float(), n_rows=4)
    r("point_map has 4 entries, expected 5", idx, n_spps=3, point_map=idx[:4], n_rows=4)
    r("n_rows must be a positive int", idx, n_spps=3, point_map=idx)
    r("n_rows must be a positive int", idx, n_spps=3, point_map=idx, n_rows=0)
    r("needs point_map", idx, n_spps=3, n_rows=4)
    r("batch_offsets must be a 1-D integer tensor", idx, n_spps=3, batch_offsets=[0, 5])
    r("at least two entries", idx, n_spps=3, batch_offsets=idx[:1])
    r("check must be a bool", idx, n_spps=3, check=1)
    r("n_spps is needed", idx[:0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.superpoint_plan(idx, n_spps=3)


def test_pools_and_drop_ins_refuse_before_a_device_is_touched():
    idx, x = torch.zeros(5, dtype=torch.int64), torch.zeros((5, 3))
    plan = ops._empty_plan(torch.device("cpu"), 4, 0, 0)
    plan.n_points = 5

    def r(fn, match, *a, **kw):
        with pytest.raises(ValueError, match=match):
            fn(*a, **kw)

    r(ops.superpoint_pool, "plan must come from superpoint_plan", x, None)
    r(ops.superpoint_pool, "reduce must be 'mean' or 'max'", x, plan, "sum")
    r(ops.superpoint_pool, "return_arg", x, plan, "mean", return_arg=True)
    r(ops.superpoint_pool, "through_map", x, plan, through_map=True)
    for bad in (x.double(), x[:4], x[:, :0], x[:, :, None], None):
        r(ops.superpoint_pool, "x must be a float32 tensor", bad, plan)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.superpoint_pool(x, plan)
    for fn in (ops.scatter_mean, ops.scatter_max):
        r(fn, "not built", x, idx, dim=1)
        r(fn, "not built", x[:, :, None], idx)
        r(fn, "not built", x, idx[:, None].expand(5, 3).contiguous())
        r(fn, "not built", x, idx[:4])
        r(fn, "index must be an integer tensor", x, idx.float())
        r(fn, "only a float32 src is built", x.double(), idx)
        r(fn, "dim_size must be a positive int", x, idx, dim_size=0)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x, idx, dim_size=2)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x, idx[:, None].expand_as(x), 0, 2)
    r(ops.custom_scatter_mean, "float32, half or bfloat16", x.double(), idx)
    r(ops.custom_scatter_mean, "output_type must be a torch.dtype", x, idx, output_type="half")
    assert ops.custom_scatter_mean(x, idx, pool=False) is x
    off = torch.tensor([0, 5])
    r(ops.isbnet_spp_pool, "voxel_box_preds must be", x, x, x.long(), idx, off)
    r(ops.isbnet_spp_pool, "voxel_output_feats has 4 rows", x, x[:4], x, idx, off)
    r(ops.isbnet_spp_pool, "use_spp_pool must be a bool", x, x, x, idx, off, use_spp_pool=None)
    r(ops.isbnet_spp_pool, "n_spps must be a positive int", x, x, x, idx, off, n_spps=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.isbnet_spp_pool(x, x, x, idx, off, n_spps=2)
    vox, lab = torch.zeros((4, 3)), torch.zeros(5)
    r(ops.spformer_pool, "x must be a float32 tensor", vox.double(), vox, vox, idx, idx)
    r(ops.spformer_pool, "coords_float must be a float32 tensor of shape \\[4, D\\]", vox, x, vox, idx, idx)
    r(ops.spformer_pool, "pool must be 'mean' or 'max'", vox, vox, vox, idx, idx, pool="sum")
    r(ops.spformer_pool, "comes with mu_labels", vox, vox, vox, idx, idx, lab)
    r(ops.spformer_pool, "mu_labels must be a float32 tensor of shape \\[5\\]", vox, vox, vox, idx, idx, lab, lab[:4], lab)
    r(ops.spformer_pool, "point_map has 4 entries", vox, vox, vox, idx, idx[:4])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.spformer_pool(vox, vox, vox, idx, idx, n_spps=2)
