"""gapro_spf_predict_count / gapro_spf_predict_fill on the MI355X: consumer_ops.spformer_instances and spformer_predict
against the NumPy restatement tests/spf_predict_ref.py on the edge cases of tests/spf_predict_cases.py and on the golden
fixtures, and against what the real reference returned (tests/golden/spf_predict_*.npz).

Labels, queries, order, stage counts, boxes, masks, run offsets and runs are integer work or bit copies: compared bit
for bit.  ``conf`` is within one float32 ulp of the restatement, a bound that is derived, not measured: both sides round
one float64 expression once; a float64 sum of at most 2^20 terms in [0, 1] in another order and a last-place difference
between the device's ``exp`` and NumPy's move the float64 value by far less than half a float32 ulp, so the rounded
values differ only at a rounding boundary.  Against the reference's float32 chain the tolerance is four times the
deviation tests/golden/make_golden_spf_predict.py measured (3.49e-7).
"""
import types

import numpy as np
import pytest

import spf_predict_cases as cases
import spf_predict_ref as ref

pytestmark = pytest.mark.gpu

CONF_TOL_REFERENCE = 4 * 3.49e-7
CASES = dict(cases.cases())
_PARAMS = ("num_class", "topk_insts", "score_thr", "npoint_thr")
_BYTES = ("conf", "label_id", "box", "query", "run_offsets", "runs", "masks")


def _dev(a, dtype=None):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    return t if dtype is None else t.to(dtype)


def _tensors(c, index_dtype=None):
    return (_dev(c["labels"]), _dev(c["pred_scores"]), _dev(c["masks"]), _dev(c["superpoints"], index_dtype),
            _dev(c["coords_float"]))


def _call(c, index_dtype=None, **kw):
    from gapro_amd import consumer_ops as ops

    par = {k: c[k] for k in _PARAMS}
    par.update(kw)
    return ops.spformer_instances("scene", *_tensors(c, index_dtype), **par)


def _predict(c, **kw):
    """The reference's call: a batch of one, scores [1, Q, 1], masks a list, test_cfg as the model holds it."""
    from gapro_amd import consumer_ops as ops

    labels, scores, masks, spp, xyz = _tensors(c)
    out = {"labels": labels[None], "scores": scores[None, :, None], "masks": [masks]}
    cfg = types.SimpleNamespace(topk_insts=c["topk_insts"], score_thr=c["score_thr"], npoint_thr=c["npoint_thr"])
    insts = [types.SimpleNamespace(gt_instances="the ground truth")]
    return ops.spformer_predict(["scene", "another"], out, spp, insts, xyz, num_class=c["num_class"], test_cfg=cfg,
                                topk_insts=1, score_thr=1.0e9, npoint_thr=0, **kw)


def _host(arrays):
    out = {k: getattr(arrays, k).cpu().numpy() for k in _BYTES}
    out["n_runs"] = np.array(arrays.n_runs)
    h = arrays.header
    out["stages"] = (h.n_candidates, h.n_after_score, h.n_rows)
    assert h.total_runs == len(out["runs"]) // 2
    return out


def _ulp_apart(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _check(got, want, n_points):
    assert want["status"] == ref.OK
    k = len(want["conf"])
    assert got["stages"] == want["stages"]
    assert np.array_equal(got["label_id"], want["label_id"]) and got["label_id"].dtype == np.int32
    assert np.array_equal(got["query"], want["query"])
    assert got["box"].shape == (k, 6) and got["box"].tobytes() == want["box"].astype(np.float32).tobytes()
    assert got["conf"].shape == (k,) and (_ulp_apart(got["conf"], want["conf"]) <= 1).all()
    assert got["masks"].shape == (k, n_points) and np.array_equal(got["masks"], want["masks"].astype(np.uint8))
    lens = np.array([len(x) // 2 for x in want["counts"]], np.int64)
    assert np.array_equal(got["n_runs"], lens)
    assert np.array_equal(got["run_offsets"], np.concatenate([[0], np.cumsum(lens)]))
    flat = np.concatenate(want["counts"]) if k else np.zeros(0, np.int64)
    assert got["runs"].dtype == np.int64 and np.array_equal(got["runs"], flat)


def _check_dict(res, want, n_points):
    assert sorted(res) == ["gt_instances", "pred_instances", "scan_id"]
    assert res["scan_id"] == "scene" and res["gt_instances"] == "the ground truth"
    got = res["pred_instances"]
    assert isinstance(got, list) and len(got) == len(want["conf"])
    for g, label, conf, box, counts in zip(got, want["label_id"], want["conf"], want["box"], want["counts"]):
        assert sorted(g) == ["box", "conf", "label_id", "pred_mask", "scan_id"] and g["scan_id"] == "scene"
        assert isinstance(g["label_id"], np.int64) and g["label_id"] == label
        assert isinstance(g["conf"], np.float32) and _ulp_apart(g["conf"], conf) <= 1
        assert sorted(g["pred_mask"]) == ["counts", "length"] and g["pred_mask"]["length"] == n_points
        assert g["pred_mask"]["counts"].dtype == np.int64 and np.array_equal(g["pred_mask"]["counts"], counts)
        assert g["box"].dtype == np.float32 and g["box"].shape == (6,) and g["box"].tobytes() == box.tobytes()
    return got


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_equals_the_restatement(name):
    c = CASES[name]
    want = ref.predict_ref(**c)
    n = len(c["superpoints"])
    got = _host(_call(c, return_arrays=True, return_masks=True))
    _check(got, want, n)
    again = _host(_call(c, return_arrays=True, return_masks=True))  # two runs give the same bytes
    assert all(got[k].tobytes() == again[k].tobytes() for k in _BYTES)
    _check_dict(_predict(c), want, n)


def test_int32_and_int64_indices_give_the_same_bytes():
    import torch

    c = CASES["points_2049"]
    a = _host(_call(c, return_arrays=True, return_masks=True, index_dtype=torch.int64))
    b = _host(_call(c, return_arrays=True, return_masks=True, index_dtype=torch.int32))
    assert all(a[k].tobytes() == b[k].tobytes() for k in _BYTES)


def test_zero_rows_give_an_empty_list_and_empty_arrays():
    c = CASES["zero_rows"]
    assert _call(c) == []
    out = _call(c, return_arrays=True)
    assert out.conf.shape == (0,) and out.runs.shape == (0,) and out.run_offsets.tolist() == [0] and out.masks is None
    assert out.box.shape == (0, 6) and out.header.n_candidates == 15


@pytest.mark.parametrize("name", ref.FIXTURES)
def test_fixture_equals_the_restatement_and_the_reference(name):
    kw, (label, conf, counts, box) = ref.load_fixture(name)
    want = ref.predict_ref(**kw)
    n = len(kw["superpoints"])
    _check(_host(_call(kw, return_arrays=True, return_masks=True)), want, n)
    got = _check_dict(_predict(kw), want, n)  # the dict, as the reference's caller gets it, in the defined order
    ours = {"status": ref.OK, "label_id": [g["label_id"] for g in got], "conf": [g["conf"] for g in got],
            "counts": [g["pred_mask"]["counts"] for g in got], "box": [g["box"] for g in got]}
    worst = ref.compare_with_reference(ours, label, conf, counts, box)
    print("%s: largest relative deviation of conf from the reference %.3g" % (name, worst))
    assert worst <= CONF_TOL_REFERENCE


def _header_spy(seen):
    """spformer_instances raises before a caller could see the header: read it through the ABI."""
    import ctypes as C

    import torch

    from gapro_amd import _lib
    from gapro_amd import consumer_ops as ops

    def run(c):
        labels, scores, masks, spp, xyz = keep = _tensors(c)
        inputs = _lib.SpfPredictInputs(
            n_queries=labels.shape[0], n_spps=masks.shape[1], n_points=spp.shape[0], labels=labels.data_ptr(),
            pred_scores=scores.data_ptr(), masks=masks.data_ptr(), superpoints=spp.data_ptr(),
            coords_float=xyz.data_ptr(), superpoints_i64=1)
        params = _lib.SpfPredictParams(num_class=c["num_class"], topk_insts=c["topk_insts"],
                                       npoint_thr=c["npoint_thr"], score_thr=c["score_thr"])
        ctx, stream = ops._ctx_stream(labels)
        lib, pin, ppar = ctx.lib, C.byref(inputs), C.byref(params)
        ws = torch.empty(int(lib.gapro_spf_predict_workspace_bytes(pin, ppar)), dtype=torch.uint8, device="cuda:0")
        d_hdr = torch.full((int(lib.gapro_spf_predict_header_bytes(pin, ppar)),), 0xAB, dtype=torch.uint8,
                           device="cuda:0")
        ctx.check(lib.gapro_spf_predict_count(ctx.handle, stream, pin, ppar, ws.data_ptr(), ws.numel(),
                                              d_hdr.data_ptr(), None))
        seen.update(hdr=_lib.SpfPredictHeader.from_buffer_copy(d_hdr.cpu().numpy().tobytes()), ctx=ctx, stream=stream,
                    inputs=inputs, params=params, ws=ws, d_hdr=d_hdr, keep=keep)
        return seen["hdr"]

    return run


@pytest.mark.parametrize("name, case, status, flags", list(cases.refusals()), ids=[r[0] for r in cases.refusals()])
def test_refusals_of_the_data(name, case, status, flags):
    import torch

    from gapro_amd._lib import GaproError

    with pytest.raises(GaproError) as e:
        _call(case)
    assert e.value.code == status
    cause = {ref.FLAG_SCORE: "labels or scores", ref.FLAG_MASK: "masks entry", ref.FLAG_COORDS: "coords_float",
             ref.FLAG_SPP: "superpoint id"}[flags & -flags]  # the first cause in the order of precedence
    assert cause in str(e.value)
    with pytest.raises(GaproError):
        _predict(case)
    seen = {}
    h = _header_spy(seen)(case)  # the flags name every cause; nothing is counted
    assert (h.status, h.flags, h.n_candidates, h.n_after_score, h.n_rows, h.total_runs) == (status, flags, 0, 0, 0, 0)
    # and the fill writes nothing
    conf = torch.full((4,), -7.0, dtype=torch.float32, device="cuda:0")
    off = torch.full((5,), -7, dtype=torch.int64, device="cuda:0")
    out = torch.full((64,), -7, dtype=torch.int64, device="cuda:0")
    m = torch.full((4, len(case["superpoints"])), 7, dtype=torch.uint8, device="cuda:0")
    s = seen
    s["ctx"].check(s["ctx"].lib.gapro_spf_predict_fill(
        s["ctx"].handle, s["stream"], C_byref(s["inputs"]), C_byref(s["params"]), s["ws"].data_ptr(), s["ws"].numel(),
        conf.data_ptr(), None, None, None, 4, off.data_ptr(), out.data_ptr(), 32, m.data_ptr(), None))
    assert (conf == -7).all() and (off == -7).all() and (out == -7).all() and (m == 7).all()


def C_byref(x):
    import ctypes

    return ctypes.byref(x)


def test_a_bad_mask_value_outside_the_candidates_is_no_refusal():
    from gapro_amd._lib import GaproError

    bad, fine = cases.mask_refusal()
    with pytest.raises(GaproError) as e:
        _call(bad)
    assert e.value.code == ref.ERR_NOT_FINITE
    _check(_host(_call(fine, return_arrays=True, return_masks=True)), ref.predict_ref(**fine), len(fine["superpoints"]))


def test_too_small_outputs_are_refused_and_nothing_is_written():
    import torch

    from gapro_amd import _lib

    c = CASES["points_1025"]
    seen = {}
    h = _header_spy(seen)(c)
    rows, runs = h.n_rows, h.total_runs
    assert h.status == 0 and rows > 1 and runs > 1
    ctx, stream, ws, d_hdr = seen["ctx"], seen["stream"], seen["ws"], seen["d_hdr"]
    lib, pin, ppar = ctx.lib, C_byref(seen["inputs"]), C_byref(seen["params"])
    for cap_rows, cap_runs in ((rows - 1, runs), (rows, runs - 1)):
        ctx.check(lib.gapro_spf_predict_count(ctx.handle, stream, pin, ppar, ws.data_ptr(), ws.numel(),
                                              d_hdr.data_ptr(), None))
        conf = torch.full((rows,), -7.0, dtype=torch.float32, device="cuda:0")
        off = torch.full((rows + 1,), -7, dtype=torch.int64, device="cuda:0")
        out = torch.full((2 * runs,), -7, dtype=torch.int64, device="cuda:0")
        ctx.check(lib.gapro_spf_predict_fill(ctx.handle, stream, pin, ppar, ws.data_ptr(), ws.numel(), conf.data_ptr(),
                                             None, None, None, cap_rows, off.data_ptr(), out.data_ptr(), cap_runs, None,
                                             d_hdr.data_ptr()))
        got = _lib.SpfPredictHeader.from_buffer_copy(d_hdr.cpu().numpy().tobytes())
        assert got.status == ref.ERR_WORKSPACE
        assert (conf == -7).all() and (off == -7).all() and (out == -7).all()
    # a workspace one byte short is refused before anything is launched
    assert lib.gapro_spf_predict_count(ctx.handle, stream, pin, ppar, ws.data_ptr(), ws.numel() - 1, d_hdr.data_ptr(),
                                       None) == ref.ERR_WORKSPACE


def test_arguments_refused_before_anything_is_launched():
    """By the library (GAPRO_ERR_BAD_ARG / a workspace size of 0) and by the Python layer (ValueError)."""
    c = CASES["scores_below_topk"]
    seen = {}
    _header_spy(seen)(c)
    ctx, stream, ws, d_hdr = seen["ctx"], seen["stream"], seen["ws"], seen["d_hdr"]
    lib = ctx.lib
    for field, value in (("topk_insts", 0), ("topk_insts", 1025), ("npoint_thr", -1), ("score_thr", float("nan")),
                         ("score_thr", float("inf")), ("num_class", 0), ("num_class", (1 << 20) // 5 + 1)):
        params = type(seen["params"]).from_buffer_copy(bytes(seen["params"]))
        setattr(params, field, value)
        assert lib.gapro_spf_predict_workspace_bytes(C_byref(seen["inputs"]), C_byref(params)) == 0, (field, value)
        assert lib.gapro_spf_predict_count(ctx.handle, stream, C_byref(seen["inputs"]), C_byref(params), ws.data_ptr(),
                                           ws.numel(), d_hdr.data_ptr(), None) == ref.ERR_BAD_ARG, (field, value)
    for field, value in (("n_spps", 1 << 31), ("n_points", 1 << 31), ("n_points", 0), ("n_queries", 0)):
        inputs = type(seen["inputs"]).from_buffer_copy(bytes(seen["inputs"]))
        setattr(inputs, field, value)
        assert lib.gapro_spf_predict_workspace_bytes(C_byref(inputs), C_byref(seen["params"])) == 0, (field, value)
    for bad in (dict(topk_insts=0), dict(topk_insts=1025), dict(topk_insts=2.0), dict(npoint_thr=-1),
                dict(score_thr=float("nan")), dict(score_thr="0"), dict(num_class=2), dict(num_class=0)):
        with pytest.raises(ValueError):
            _call(c, **bad)


def test_host_tensors_and_wrong_shapes_are_refused_per_argument():
    import torch

    from gapro_amd import consumer_ops as ops

    c = CASES["scores_below_topk"]
    par = {k: c[k] for k in _PARAMS}
    good = list(_tensors(c))
    for i, name in enumerate(("pred_labels", "pred_scores", "pred_masks", "superpoints", "coords_float")):
        args = list(good)
        args[i] = args[i].cpu()
        with pytest.raises(RuntimeError, match="device"):
            ops.spformer_instances("scene", *args, **par)
        args[i] = good[i].to(torch.float64)
        with pytest.raises(ValueError, match=name):
            ops.spformer_instances("scene", *args, **par)
        args[i] = good[i][:-1]
        with pytest.raises(ValueError):
            ops.spformer_instances("scene", *args, **par)
    with pytest.raises(ValueError, match="out must be a dict"):
        ops.spformer_predict(["scene"], {"labels": good[0][None]}, good[3], [None], good[4])
