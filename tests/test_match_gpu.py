"""gapro_match_cost on the MI355X: consumer_ops.match_cost against the NumPy float64 restatement tests/match_ref.py at
the kernel's tile, chunk and batch edges and on edge data, its refusals, its repeatability, and match_cost /
hungarian_match on the outputs of the real reference (tests/golden/match_*.npz) and on get_spp_gt's own output.

Tolerances (tests/match_ref.py): device against the restatement 1 float32 ulp of the value plus 1e-9; device against a
fixture 4 x the fixture's own ref_dev; assignments equal as sorted (row, col % I) pairs.
"""
import ctypes as C

import numpy as np
import pytest

import match_ref as ref

pytestmark = pytest.mark.gpu

N_CLASSES = 5


def _dev(a, dtype=None):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    return t if dtype is None else t.to(dtype)


def _sample(rng, Q, I, S):
    lo = rng.uniform(-3, 3, (I, 3))
    return {"mask_logits": rng.normal(0, 3, (Q, S)).astype(np.float32),
            "mask": (rng.random((I, S)) < 0.4).astype(np.float32),
            "cls": rng.integers(0, N_CLASSES, I).astype(np.int64),
            "box": np.concatenate([lo, lo + rng.uniform(0.2, 3, (I, 3))], 1).astype(np.float32)}


def _batch(seed, Q, shapes):
    """shapes: per sample (I, S) or None."""
    rng = np.random.default_rng(seed)
    B = len(shapes)
    lo = rng.uniform(-3, 3, (B, Q, 3))
    return {"cls_logits": rng.normal(0, 2, (B, Q, N_CLASSES)).astype(np.float32),
            "conf_logits": rng.normal(0, 1, (B, Q)).astype(np.float32),
            "box_preds": np.concatenate([lo, lo + rng.uniform(0.2, 3, (B, Q, 3))], 2).astype(np.float32),
            "samples": [None if s is None else _sample(rng, Q, *s) for s in shapes]}


def _want(d, weights=ref.WEIGHTS):
    return [None if s is None else ref.cost(d["cls_logits"][b], s["mask_logits"], d["conf_logits"][b],
                                            d["box_preds"][b], s["mask"], s["cls"], s["box"], weights=weights)
            for b, s in enumerate(d["samples"])]


def _args(d, cls_dtype=None):
    import torch

    dc = [None if s is None else {"mask": _dev(s["mask"]), "cls": _dev(s["cls"], cls_dtype or torch.int64),
                                  "box": _dev(s["box"])} for s in d["samples"]]
    logits = [None if s is None else _dev(s["mask_logits"]) for s in d["samples"]]
    return [_dev(d["cls_logits"]), logits, _dev(d["conf_logits"]), _dev(d["box_preds"]), dc]


def _check(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g is None) == (w is None)
        if g is not None:
            assert g.is_cuda and not g.requires_grad
            assert ref.close(g.cpu().numpy(), w)
    return True


# Q, I and S on both sides of the tile (16 x 16), of a lane's four columns, of a chunk (16) and of the four waves' round
# (64), one and several tiles, one and several chunks per wave
EDGE_SHAPES = [(1, 1, 1), (15, 15, 3), (16, 16, 4), (17, 17, 5), (33, 33, 63), (1, 33, 64), (33, 1, 65), (16, 17, 257),
               (17, 16, 1), (15, 33, 5), (33, 15, 257), (16, 1, 63), (1, 16, 65), (17, 15, 64)]


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=lambda s: "Q%d-I%d-S%d" % s)
def test_edge_shapes_equal_the_restatement(shape):
    from gapro_amd import consumer_ops as ops

    Q, I, S = shape
    d = _batch(sum(shape), Q, [(I, S)])
    assert _check(ops.match_cost(*_args(d)), _want(d))


@pytest.mark.parametrize("shapes", [
    [(17, 65), (1, 3), (33, 257), (16, 64)],
    [None, (5, 20), None, None, (18, 70), None],
    [(3, 9), None],
    [None, (40, 130)],
], ids=["different", "nones-around", "none-last", "none-first"])
def test_batches_with_different_samples_and_nones(shapes):
    import torch
    from gapro_amd import consumer_ops as ops

    d = _batch(len(shapes), 19, shapes)
    got = ops.match_cost(*_args(d))
    assert _check(got, _want(d))
    kept = [g for g in got if g is not None]
    assert len({g.untyped_storage().data_ptr() for g in kept}) == 1  # views into one allocation
    assert all(g.dtype == torch.float32 and tuple(g.shape) == (19, s[0]) for g, s in zip(kept, [s for s in shapes if s]))


def test_all_none_batch_returns_nones():
    from gapro_amd import consumer_ops as ops

    d = _batch(0, 8, [None, None, None])
    assert ops.match_cost(*_args(d)) == [None] * 3
    gt, aux = ops.hungarian_match(*_args(d), dup_gt=2)
    assert all(v == [None] * 3 for v in list(gt.values()) + list(aux.values()))


def test_edge_data_equals_the_restatement():
    """A mask row and a mask column of zeros, logits of +-100 and 0, zero-volume and inverted boxes; then a NaN logit, an
    infinite conf and NaN boxes, which take whole rows and columns to 100000."""
    from gapro_amd import consumer_ops as ops

    d = _batch(77, 20, [(18, 70), (6, 33)])
    s0, s1 = d["samples"]
    s0["mask"][4, :] = 0.0
    s0["mask"][:, 9] = 0.0
    s0["mask"][17, :] = 1.0
    s0["mask_logits"][2, :] = 100.0
    s0["mask_logits"][3, :] = -100.0
    s0["mask_logits"][5, :] = 0.0
    s0["mask_logits"][6, ::2] = 100.0
    s0["mask_logits"][6, 1::2] = -100.0
    s0["box"][1, 3:] = s0["box"][1, :3]                      # zero volume
    s0["box"][2] = s0["box"][2][[3, 4, 5, 0, 1, 2]]          # inverted
    d["box_preds"][0, 7, 3:] = d["box_preds"][0, 7, :3]
    d["box_preds"][0, 8] = d["box_preds"][0, 8][[3, 4, 5, 0, 1, 2]]
    d["box_preds"][0, 9] = s0["box"][1]                      # both of zero volume, and equal
    want = _want(d)
    assert np.isfinite(want[0]).all() and (want[0] != 100000.0).all()
    assert _check(ops.match_cost(*_args(d)), want)

    s0["mask_logits"][11, 37] = np.nan
    d["conf_logits"][0, 12] = np.inf
    d["conf_logits"][0, 13] = -np.inf
    d["box_preds"][0, 14, 2] = np.nan
    s0["box"][5, 4] = np.nan
    d["cls_logits"][1, 3, 1] = np.nan
    s1["mask_logits"][19, 32] = np.nan                        # the last row and column of its sample
    want = _want(d)
    for q in (11, 12, 13, 14):
        assert (want[0][q] == 100000.0).all()
    assert (want[0][:, 5] == 100000.0).all() and (want[1][3] == 100000.0).all() and (want[1][19] == 100000.0).all()
    assert (want[0] == 100000.0).sum() == 4 * 18 + 20 - 4 and (want[1] == 100000.0).sum() == 2 * 6
    got = ops.match_cost(*_args(d))
    assert _check(got, want)
    for g, w in zip(got, want):  # exactly 100000 where the restatement has it, and nowhere else
        assert np.array_equal(g.cpu().numpy() == 100000.0, w == 100000.0)


def test_cls_dtypes_a_transposed_view_custom_weights_and_another_stream():
    import torch
    from gapro_amd import consumer_ops as ops

    d = _batch(5, 21, [(9, 37), (17, 18)])
    want = _want(d)
    assert _check(ops.match_cost(*_args(d, torch.int32)), want)
    args = _args(d)
    args[1][0] = _dev(d["samples"][0]["mask_logits"].T.copy()).t()       # [Q, S] with strides (1, Q)
    wide = _dev(np.concatenate([d["samples"][1]["mask_logits"]] * 2, 1))
    args[1][1] = wide[:, :18]                                           # row stride 36: read in place
    assert not args[1][0].is_contiguous() and not args[1][1].is_contiguous()
    assert _check(ops.match_cost(*args), want)
    for weights in ((2.0, 0.0, 0.25, 3.0, 1.5), {"class": 0.0, "dice": 1.0, "bce": 0.0, "conf": 0.0, "giou": 0.0},
                    (0.0, 0.0, 0.0, 0.0, 1.0)):
        w = tuple(weights[k] for k in ("class", "dice", "bce", "conf", "giou")) if isinstance(weights, dict) else weights
        assert _check(ops.match_cost(*_args(d), weights=weights), _want(d, w))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = ops.match_cost(*_args(d))
    s.synchronize()
    assert _check(got, want)
    g = _args(d)
    g[0].requires_grad_(True)
    g[1][0].requires_grad_(True)
    assert _check(ops.match_cost(*g), want)  # no autograd: plain tensors come back


def test_two_calls_give_equal_bytes():
    from gapro_amd import consumer_ops as ops

    d = _batch(11, 40, [(35, 300), (7, 1500), (20, 66)])
    args = _args(d)
    a = [g.cpu().numpy().tobytes() for g in ops.match_cost(*args)]
    b = [g.cpu().numpy().tobytes() for g in ops.match_cost(*args)]
    assert a == b
    assert _check(ops.match_cost(*args), _want(d))


def _raw_call(d, dc, logits, cost, *, n_classes=N_CLASSES, ws_cut=0, offsets=None, weights=None, cost_floats=None):
    """gapro_match_cost at the C ABI on a cost buffer the caller owns; returns (rc, status words)."""
    import torch
    from gapro_amd import _lib

    ctx = _lib.Context.get(0)
    lib = ctx.lib
    B, Q = d["cls_logits"].shape[:2]
    tasks = (_lib.MatchTask * B)()
    off = tot_i = tot_s = 0
    for b, e in enumerate(dc):
        if e is None:
            continue
        n_inst, n_cols = e["mask"].shape
        tasks[b] = _lib.MatchTask(logits[b].data_ptr(), logits[b].stride(0), e["mask"].data_ptr(), e["cls"].data_ptr(),
                                  e["box"].data_ptr(), n_inst, n_cols, off if offsets is None else offsets[b])
        off += Q * n_inst
        tot_i += n_inst
        tot_s += n_cols
    ws_bytes = int(lib.gapro_match_cost_workspace_bytes(B, Q, tot_i, tot_s))
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda:0")
    status = torch.full((4,), 77, dtype=torch.int32, device="cuda:0")
    keep = [_dev(d["cls_logits"]), _dev(d["conf_logits"]), _dev(d["box_preds"])]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.gapro_match_cost(ctx.handle, stream, C.cast(tasks, C.c_void_p), B, Q, n_classes, _lib.GAPRO_LABEL_I64,
                              keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(),
                              C.byref(_lib.MatchWeights(*weights)) if weights else None, ws.data_ptr(),
                              ws_bytes - ws_cut, cost.data_ptr(), cost.numel() if cost_floats is None else cost_floats,
                              None, status.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, status.cpu().numpy().tolist()


@pytest.mark.parametrize("cause", ["class too large", "class negative", "mask 0.5", "mask NaN"])
def test_refusals_of_the_data_write_nothing(cause):
    import torch
    from gapro_amd import _lib
    from gapro_amd import consumer_ops as ops

    d = _batch(21, 18, [(17, 40), None, (5, 70)])
    s = d["samples"][2]
    if cause == "class too large":
        s["cls"][4] = N_CLASSES
    elif cause == "class negative":
        s["cls"][0] = -1
    elif cause == "mask 0.5":
        s["mask"][3, 69] = 0.5
    else:
        s["mask"][0, 0] = np.nan
    flag, text = (1, "class label") if cause.startswith("class") else (2, "mask value")
    args = _args(d)
    for fn in (ops.match_cost, ops.hungarian_match):
        with pytest.raises(_lib.GaproError) as e:
            fn(*args)
        assert e.value.code == _lib.GAPRO_ERR_BAD_ARG and text in str(e.value) and "sample 2" in str(e.value), e.value
    cost = torch.full((18 * 22,), 77.0, dtype=torch.float32, device="cuda:0")
    rc, status = _raw_call(d, args[4], args[1], cost)
    assert rc == 0 and status == [_lib.GAPRO_ERR_BAD_ARG, 2, flag, 0]  # enqueued: the refusal is the status word's
    assert bool((cost == 77.0).all())


def test_refusals_before_anything_is_launched():
    import torch
    from gapro_amd import _lib

    d = _batch(22, 10, [(4, 12), (3, 9)])
    args = _args(d)
    cost = torch.full((10 * 7 + 5,), 77.0, dtype=torch.float32, device="cuda:0")
    untouched = [77, 77, 77, 77]
    rc, status = _raw_call(d, args[4], args[1], cost)
    assert rc == 0 and status == [0, -1, 0, 0]
    want = _want(d)
    got = cost.cpu().numpy()
    assert ref.close(got[:40].reshape(10, 4), want[0]) and ref.close(got[40:70].reshape(10, 3), want[1])
    assert (got[70:] == 77.0).all()
    # blocks in another order and with a gap
    cost.fill_(77.0)
    rc, status = _raw_call(d, args[4], args[1], cost, offsets=[35, 0])
    got = cost.cpu().numpy()
    assert rc == 0 and ref.close(got[35:75].reshape(10, 4), want[0]) and ref.close(got[:30].reshape(10, 3), want[1])
    assert (got[30:35] == 77.0).all()
    cost.fill_(77.0)
    for kw in (dict(offsets=[0, 39]), dict(offsets=[29, 0]), dict(offsets=[0, 46]), dict(offsets=[-1, 40]),
               dict(cost_floats=69), dict(cost_floats=0), dict(n_classes=0), dict(weights=(1, 1, 1, 1, -0.5)),
               dict(weights=(1, 1, float("nan"), 1, 1)), dict(weights=(float("inf"), 1, 1, 1, 1))):
        rc, status = _raw_call(d, args[4], args[1], cost, **kw)
        assert rc == _lib.GAPRO_ERR_BAD_ARG and status == untouched, kw
    rc, status = _raw_call(d, args[4], args[1], cost, ws_cut=1)
    assert rc == _lib.GAPRO_ERR_WORKSPACE and status == untouched
    assert bool((cost == 77.0).all())


def _fixture_args(z, samples):
    dc = [None if s is None else {k: _dev(s[k]) for k in ("mask", "cls", "box")} for s in samples]
    logits = [None if s is None else _dev(s["mask_logits"]) for s in samples]
    return [_dev(z["cls_logits"]), logits, _dev(z["conf_logits"]), _dev(z["box_preds"]), dc]


@pytest.mark.parametrize("name", ref.FIXTURES)
def test_fixture_equals_the_reference(name):
    from gapro_amd import consumer_ops as ops

    z, samples = ref.fixture(name)
    ref_dev, dup = float(z["ref_dev"]), int(z["dup_gt"])
    args = _fixture_args(z, samples)
    got = ops.match_cost(*args)
    gt, aux = ops.hungarian_match(*args, dup_gt=dup)
    for b, s in enumerate(samples):
        if s is None:
            assert got[b] is None and all(v[b] is None for v in list(gt.values()) + list(aux.values()))
            continue
        c = got[b].cpu().numpy()
        err = np.abs(c.astype(np.float64) - s["ref_cost"].astype(np.float64)).max()
        print("%s sample %d: max |device - reference| %.3g, ref_dev %.3g" % (name, b, err, ref_dev))
        assert c.dtype == np.float32 and err <= 4 * ref_dev
        assert ref.close(c, ref.cost(z["cls_logits"][b], s["mask_logits"], z["conf_logits"][b], z["box_preds"][b],
                                     s["mask"], s["cls"], s["box"]))
        n_inst = len(s["cls"])
        for out, d, row, col in ((gt, 1, s["row"], s["col"]), (aux, dup, s["aux_row"], s["aux_col"])):
            rows = out["row_indices"][b]
            assert isinstance(rows, np.ndarray) and rows.dtype == np.int64 and np.array_equal(rows, np.sort(row))
            assert len(rows) == min(int(z["n_queries"]), d * n_inst)
            # the gathered targets are the reference's: its rows are ascending too, so the order is the same
            order = np.argsort(row)
            want_col = (col % n_inst)[order]
            assert np.array_equal(out["inst_labels"][b].cpu().numpy(), s["mask"][want_col])
            assert np.array_equal(out["cls_labels"][b].cpu().numpy(), s["cls"][want_col])
            assert np.array_equal(out["box_labels"][b].cpu().numpy(), s["box"][want_col])
            assert all(out[k][b].is_cuda for k in ("inst_labels", "cls_labels", "box_labels"))


def test_hungarian_match_on_the_output_of_get_spp_gt():
    import spp_gt_ref
    from gapro_amd import consumer_ops as ops

    z, _ = spp_gt_ref.fixture("second_empty")
    B = int(z["batch_size"])
    dc = ops.get_spp_gt(_dev(z["labels"]), _dev(z["spps"]), _dev(z["cls"]), _dev(z["box"]), _dev(z["offsets"]), B)
    assert [e is None for e in dc] == [False, True, False]
    Q, n_classes = 12, int(z["cls"].max()) + 1
    rng = np.random.default_rng(4)
    lo = rng.uniform(-8, 8, (B, Q, 3))
    cls_logits = rng.normal(0, 2, (B, Q, n_classes)).astype(np.float32)
    conf = rng.normal(0, 1, (B, Q)).astype(np.float32)
    box_preds = np.concatenate([lo, lo + rng.uniform(0.5, 4, (B, Q, 3))], 2).astype(np.float32)
    logits = [None if e is None else rng.normal(0, 3, (Q, e["mask"].shape[1])).astype(np.float32) for e in dc]
    args = [_dev(cls_logits), [None if x is None else _dev(x) for x in logits], _dev(conf), _dev(box_preds), dc]
    costs = ops.match_cost(*args)
    gt, aux = ops.hungarian_match(*args, dup_gt=3)
    for b, e in enumerate(dc):
        if e is None:
            assert costs[b] is None and gt["row_indices"][b] is None and aux["box_labels"][b] is None
            continue
        mask, cls, box = (e[k].cpu().numpy() for k in ("mask", "cls", "box"))
        want = ref.cost(cls_logits[b], logits[b], conf[b], box_preds[b], mask, cls, box)
        c = costs[b].cpu().numpy()
        assert ref.close(c, want)
        for out, d in ((gt, 1), (aux, 3)):
            rows, cols = ops.linear_sum_assignment(c, d)
            assert np.array_equal(out["row_indices"][b], rows) and len(rows) == min(Q, d * len(cls))
            assert np.array_equal(out["inst_labels"][b].cpu().numpy(), mask[cols])
            assert np.array_equal(out["cls_labels"][b].cpu().numpy(), cls[cols])
            assert np.array_equal(out["box_labels"][b].cpu().numpy(), box[cols])
            assert out["cls_labels"][b].dtype == e["cls"].dtype
