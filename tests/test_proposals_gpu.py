"""gapro_proposals_count / gapro_proposals_fill on the MI355X: consumer_ops.get_instance, mask_nms and
rle_encode_gpu_batch against the NumPy restatement tests/proposals_ref.py on the edge cases of tests/proposals_cases.py
and on the golden fixtures, and get_instance against what the real reference returned (tests/golden/proposals_*.npz).

Labels, queries, order, boxes, masks and runs are integer work or bit copies: compared bit for bit.  ``conf`` is a
float64 expression rounded once on both sides; the device's float64 exp and NumPy's may differ in the last place, which
moves the rounded float32 by at most one ulp: that is the tolerance against the restatement.  Against the reference's
float32 chain the tolerance is the one tests/test_proposals_cpu.py derives (four times the measured 2.18e-7).
"""
import types

import numpy as np
import pytest

import proposals_cases as cases
import proposals_ref as ref

pytestmark = pytest.mark.gpu

CONF_TOL_REFERENCE = 4 * 2.18e-7
CASES = dict(cases.cases())
_PARAMS = ("logit_thresh", "npoint_thresh", "type_nms", "topk", "nms_threshold", "sem2ins_classes", "pre_topk")


def _dev(a, dtype=None):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    return t if dtype is None else t.to(dtype)


def _call(c, index_dtype=None, **kw):
    from gapro_amd import consumer_ops as ops

    par = {k: c[k] for k in _PARAMS if k in c}
    par["dataset_name"] = {1: "scannetv2", 3: "s3dis"}[c.get("label_shift", 1)]
    par.update(kw)
    vs = c.get("voxel_spps")
    return ops.get_instance("scene", _dev(c["cls_logits"]), _dev(c["mask_logits"]), _dev(c["conf_logits"]),
                            _dev(c["box_preds"]), _dev(c["v2p_map"], index_dtype), _dev(c["semantic_preds"], index_dtype),
                            _dev(c["spps"], index_dtype), instance_classes=c["instance_classes"],
                            voxel_spps=None if vs is None else _dev(vs, index_dtype), n_spps=c["n_spps"], **par)


def _host(arrays):
    out = {k: getattr(arrays, k).cpu().numpy() for k in ("conf", "label_id", "box", "query", "run_offsets", "runs")}
    out["masks"] = None if arrays.masks is None else arrays.masks.cpu().numpy()
    out["n_runs"] = np.array(arrays.n_runs)
    out["stages"] = (arrays.header.n_candidates, arrays.header.n_after_npoints, arrays.header.n_after_nms,
                     arrays.header.n_after_refine)
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
    assert got["box"].tobytes() == want["box"].astype(np.float32).tobytes()
    assert got["conf"].shape == (k,) and (_ulp_apart(got["conf"], want["conf"]) <= 1).all()
    assert got["masks"].shape == (k, n_points) and np.array_equal(got["masks"], want["masks"].astype(np.uint8))
    lens = np.array([len(x) // 2 for x in want["counts"]], np.int64)
    assert np.array_equal(got["n_runs"], lens)
    assert np.array_equal(got["run_offsets"], np.concatenate([[0], np.cumsum(lens)]))
    flat = np.concatenate(want["counts"]) if k else np.zeros(0, np.int64)
    assert got["runs"].dtype == np.int64 and np.array_equal(got["runs"], flat)


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_equals_the_restatement(name):
    c = CASES[name]
    want = ref.get_instance_ref(**c)
    got = _host(_call(c, return_arrays=True, return_masks=True))
    _check(got, want, len(c["v2p_map"]))
    again = _host(_call(c, return_arrays=True, return_masks=True))  # two runs give the same bytes
    assert all(got[k].tobytes() == again[k].tobytes() for k in ("conf", "label_id", "box", "query", "runs", "masks"))
    if c.get("voxel_spps") is not None:  # the other form of mask_logits gives the same bytes
        wide = dict(c, mask_logits=np.ascontiguousarray(c["mask_logits"][:, c["voxel_spps"]]), voxel_spps=None)
        other = _host(_call(wide, return_arrays=True, return_masks=True, index_dtype=None))
        assert all(got[k].tobytes() == other[k].tobytes() for k in ("conf", "label_id", "box", "query", "runs", "masks"))


def test_int32_indices_give_the_same_bytes():
    import torch

    c = CASES["sem2ins_with_rows"]
    a = _host(_call(c, return_arrays=True, return_masks=True))
    b = _host(_call(c, return_arrays=True, return_masks=True, index_dtype=torch.int32))
    assert all(a[k].tobytes() == b[k].tobytes() for k in ("conf", "label_id", "query", "runs", "masks"))


def test_zero_rows_give_an_empty_list_and_empty_arrays():
    c = CASES["all_below_npoint"]
    assert _call(c) == []
    out = _call(c, return_arrays=True)
    assert out.conf.shape == (0,) and out.runs.shape == (0,) and out.run_offsets.tolist() == [0] and out.masks is None


@pytest.mark.parametrize("name", ref.FIXTURES)
def test_fixture_equals_the_restatement_and_the_reference(name):
    kw, (label, conf, counts) = ref.load_fixture(name)
    want = ref.get_instance_ref(**kw)
    _check(_host(_call(kw, return_arrays=True, return_masks=True)), want, len(kw["v2p_map"]))
    # the list, as the reference's caller gets it; test_cfg as the reference passes it
    cfg = types.SimpleNamespace(type_nms=kw["type_nms"], topk=kw["topk"], nms_threshold=kw["nms_threshold"])
    got = _call(kw, test_cfg=cfg, type_nms="standard" if kw["type_nms"] == "matrix" else "matrix", topk=3)
    n_sem = len(kw["sem2ins_classes"])
    assert all(g["scan_id"] == "scene" and g["pred_mask"]["length"] == len(kw["v2p_map"]) for g in got)
    assert all(g["conf"] == 1.0 and isinstance(g["conf"], float) for g in got[:n_sem])
    assert all(isinstance(g["conf"], np.float32) for g in got[n_sem:])
    assert all(g["pred_mask"]["counts"].dtype == np.int64 for g in got)
    ours = {"status": ref.OK, "label_id": [g["label_id"] for g in got], "conf": [g["conf"] for g in got],
            "counts": [g["pred_mask"]["counts"] for g in got]}
    assert ref.compare_with_reference(ours, label, conf, counts) <= CONF_TOL_REFERENCE
    assert [int(g["label_id"]) for g in got] == [int(v) for v in want["label_id"]]  # and in the defined order


@pytest.mark.parametrize("name, case, status, flags", list(cases.refusals()), ids=[r[0] for r in cases.refusals()])
def test_refusals_of_the_data(name, case, status, flags):
    from gapro_amd._lib import GaproError

    with pytest.raises(GaproError) as e:
        _call(case)
    assert e.value.code == status
    assert ref.get_instance_ref(**case)["flags"] == flags


def test_the_flags_name_every_cause():
    """The header's flags, read through the ABI: get_instance raises before a caller could see them."""
    import ctypes as C

    import torch

    from gapro_amd import _lib
    from gapro_amd import consumer_ops as ops

    seen = {}
    run = ops._predict_run

    def spy(who, chain, anchor, inputs, params, keep, n_points, **kw):
        ctx, stream = ops._ctx_stream(anchor)
        lib, pin, ppar = ctx.lib, C.byref(inputs), C.byref(params)
        ws = torch.empty(int(lib.gapro_proposals_workspace_bytes(pin, ppar)), dtype=torch.uint8, device=anchor.device)
        n = int(lib.gapro_proposals_header_bytes(pin, ppar))
        d_hdr = torch.full((n,), 0xAB, dtype=torch.uint8, device=anchor.device)
        ctx.check(lib.gapro_proposals_count(ctx.handle, stream, pin, ppar, ws.data_ptr(), ws.numel(), d_hdr.data_ptr(),
                                            None))
        seen["hdr"] = _lib.ProposalsHeader.from_buffer_copy(d_hdr.cpu().numpy().tobytes())
        return run(who, chain, anchor, inputs, params, keep, n_points, **kw)

    ops._predict_run = spy
    try:
        for name, case, status, flags in cases.refusals():
            with pytest.raises(_lib.GaproError):
                _call(case)
            h = seen["hdr"]
            assert (h.status, h.flags, h.n_rows, h.total_runs) == (status, flags, 0, 0), name
        bad, fine = cases.mask_refusal()
        with pytest.raises(_lib.GaproError) as e:
            _call(bad)
        assert e.value.code == ref.ERR_NOT_FINITE and seen["hdr"].flags == ref.FLAG_MASK
        _check(_host(_call(fine, return_arrays=True, return_masks=True)), ref.get_instance_ref(**fine),
               len(fine["v2p_map"]))
    finally:
        ops._predict_run = run


def test_too_small_outputs_are_refused_and_nothing_is_written():
    import ctypes as C

    import torch

    from gapro_amd import _lib
    from gapro_amd import consumer_ops as ops

    c = CASES["run_shapes"]
    captured = {}
    run = ops._predict_run

    def grab(who, chain, anchor, inputs, params, keep, n_points, **kw):
        captured.update(inputs=inputs, params=params, keep=keep, anchor=anchor)
        return run(who, chain, anchor, inputs, params, keep, n_points, **kw)

    ops._predict_run = grab
    try:
        full = _call(c, return_arrays=True)
    finally:
        ops._predict_run = run
    rows, runs = int(full.header.n_rows), int(full.header.total_runs)
    ctx, stream = ops._ctx_stream(captured["anchor"])
    lib, pin, ppar = ctx.lib, C.byref(captured["inputs"]), C.byref(captured["params"])
    ws = torch.empty(int(lib.gapro_proposals_workspace_bytes(pin, ppar)), dtype=torch.uint8, device="cuda:0")
    d_hdr = torch.zeros(int(lib.gapro_proposals_header_bytes(pin, ppar)), dtype=torch.uint8, device="cuda:0")
    for cap_rows, cap_runs in ((rows - 1, runs), (rows, runs - 1)):
        ctx.check(lib.gapro_proposals_count(ctx.handle, stream, pin, ppar, ws.data_ptr(), ws.numel(), d_hdr.data_ptr(),
                                            None))
        conf = torch.full((rows,), -7.0, dtype=torch.float32, device="cuda:0")
        off = torch.full((rows + 1,), -7, dtype=torch.int64, device="cuda:0")
        out = torch.full((2 * runs,), -7, dtype=torch.int64, device="cuda:0")
        ctx.check(lib.gapro_proposals_fill(ctx.handle, stream, pin, ppar, ws.data_ptr(), ws.numel(), conf.data_ptr(),
                                           None, None, None, cap_rows, off.data_ptr(), out.data_ptr(), cap_runs, None,
                                           d_hdr.data_ptr()))
        h = _lib.ProposalsHeader.from_buffer_copy(d_hdr.cpu().numpy().tobytes())
        assert h.status == -7  # GAPRO_ERR_WORKSPACE
        assert (conf == -7).all() and (off == -7).all() and (out == -7).all()
    # a workspace one byte short is refused before anything is launched
    assert lib.gapro_proposals_count(ctx.handle, stream, pin, ppar, ws.data_ptr(), ws.numel() - 1, d_hdr.data_ptr(),
                                     None) == -7


def test_python_side_refusals():
    c = CASES["spp_rules"]
    for bad in (dict(npoint_thresh=0), dict(pre_topk=0), dict(pre_topk=1025), dict(topk=-2)):
        with pytest.raises(ValueError):
            _call(c, **bad)
    with pytest.raises(RuntimeError):
        _call(c, type_nms="soft")


def _nms_inputs(c):
    """The candidates stage 4 sees, from the restatement, in a shuffled order (mask_nms sorts)."""
    score = ref.scores_ref(c["cls_logits"], c["conf_logits"]).reshape(-1)
    C_ = c["instance_classes"]
    cand = ref.order_ref(score, min(c.get("pre_topk", 300), len(score)))
    vs = c.get("voxel_spps")
    bits = ref.bits_ref(c["mask_logits"], c.get("logit_thresh", 0.0), vs)
    rng = np.random.default_rng(5)
    cand = cand[rng.permutation(len(cand))]
    return bits[cand // C_], (cand % C_).astype(np.int64), score[cand], np.asarray(c["box_preds"])[cand // C_]


@pytest.mark.parametrize("name", ("topk_cuts", "topk_none", "topk_beyond", "standard_scene", "identical_masks_one_class",
                                  "iou_equals_threshold", "same_query_two_classes", "tie_inside", "rows_132"))
def test_mask_nms_equals_the_restatement(name):
    import torch

    from gapro_amd import consumer_ops as ops

    c = CASES[name]
    bits, cat, score, box = _nms_inputs(c)
    kind, topk, thr = c.get("type_nms", "matrix"), c.get("topk", 100), c.get("nms_threshold", 0.2)
    cfg = types.SimpleNamespace(type_nms=kind, topk=topk, nms_threshold=thr)
    order = ref.order_ref(score, len(score))
    keep, conf = ref.nms_ref(bits[order], cat[order], score[order], kind, topk, thr)
    want = order[keep]
    m, k, s, b = ops.mask_nms(_dev(bits), _dev(cat), _dev(score), _dev(box), cfg)
    assert m.dtype == torch.bool and np.array_equal(m.cpu().numpy(), bits[want])
    assert k.dtype == torch.int64 and np.array_equal(k.cpu().numpy(), cat[want])
    assert (_ulp_apart(s.cpu().numpy(), conf) <= 1).all() and s.shape == (len(want),)
    assert b.cpu().numpy().tobytes() == box[want].tobytes()
    m2, _, s2, _ = ops.mask_nms(_dev(bits), _dev(cat), _dev(score), _dev(box), cfg)
    assert torch.equal(m, m2) and s.cpu().numpy().tobytes() == s2.cpu().numpy().tobytes()


def test_mask_nms_of_nothing_and_of_empty_masks():
    import torch

    from gapro_amd import consumer_ops as ops

    cfg = types.SimpleNamespace(type_nms="standard", topk=-1, nms_threshold=0.2)
    none = ops.mask_nms(torch.zeros((0, 50), dtype=torch.bool, device="cuda:0"), _dev(np.zeros(0, np.int64)),
                        _dev(np.zeros(0, np.float32)), _dev(np.zeros((0, 6), np.float32)), cfg)
    assert none[0].shape == (0, 50)
    m, k, s, b = ops.mask_nms(torch.zeros((3, 50), dtype=torch.bool, device="cuda:0"), _dev(np.zeros(3, np.int64)),
                              _dev(np.array([0.3, 0.5, 0.4], np.float32)), _dev(np.zeros((3, 6), np.float32)), cfg)
    assert s.tolist() == [0.5, 0.4000000059604645, 0.30000001192092896]  # an empty union has iou 0: nothing suppressed


@pytest.mark.parametrize("name", ("run_shapes", "rows_132", "spp_rules", "all_below_npoint"))
def test_rle_encode_gpu_batch_equals_the_restatement(name):
    from gapro_amd import consumer_ops as ops

    masks = ref.get_instance_ref(**CASES[name])["masks"]
    if name == "all_below_npoint":
        masks = np.zeros((3, 64), bool)  # rows without a run
    got = ops.rle_encode_gpu_batch(_dev(masks))
    assert len(got) == len(masks)
    for g, m in zip(got, masks):
        assert g["length"] == masks.shape[1] and g["counts"].dtype == np.int64
        assert np.array_equal(g["counts"], ref.rle_ref(m))


def test_rle_encode_gpu_batch_beyond_one_call_and_across_chunks():
    """1100 rows (more than one call takes) of 2500 points (three chunks of points), runs that cross the chunk edges."""
    from gapro_amd import consumer_ops as ops

    rng = np.random.default_rng(11)
    masks = np.repeat(rng.random((1100, 250)) < 0.5, 10, axis=1)
    masks[:, 830:840] = True
    masks[5] = True
    masks[6] = False
    got = ops.rle_encode_gpu_batch(_dev(masks))
    assert len(got) == 1100
    for g, m in zip(got, masks):
        assert np.array_equal(g["counts"], ref.rle_ref(m))
