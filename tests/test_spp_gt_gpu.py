"""gapro_spp_gt_count / gapro_spp_gt_fill on the MI355X: consumer_ops.get_spp_gt and get_subsample_gt, exactly against
the NumPy restatement tests/spp_gt_ref.py on the edge cases of tests/spp_gt_cases.py, and against the outputs of the
real reference (tests/golden/spp_gt_*.npz).  Everything here is integer work or a bit copy: no tolerance anywhere.
"""
import ctypes as C

import numpy as np
import pytest

import spp_gt_cases as cases
import spp_gt_ref as ref

pytestmark = pytest.mark.gpu


def _dev(a, dtype=None):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    return t if dtype is None else t.to(dtype)


def _host(result):
    return [None if e is None else {k: v.cpu().numpy() for k, v in e.items()} for e in result]


def _call(d, strict=False, return_ids=True, labels=None, spps=None, offsets=None, **kw):
    from gapro_amd import consumer_ops as ops

    labels = _dev(d.labels) if labels is None else labels
    offsets = _dev(d.offsets) if offsets is None else offsets
    if d.spps is None:
        return ops.get_subsample_gt(labels, _dev(d.idxs), _dev(d.cls), _dev(d.box), offsets, d.batch_size, d.ignore,
                                    return_ids=return_ids)
    spps = _dev(d.spps) if spps is None else spps
    return ops.get_spp_gt(labels, spps, _dev(d.cls), _dev(d.box), offsets, d.batch_size, d.ignore, True,
                          n_spps=d.n_spps, strict=strict, return_ids=return_ids, **kw)


@pytest.mark.parametrize("name", cases.GOOD_NAMES)
def test_case_equals_the_restatement(name):
    d = cases.build(name)
    got = _call(d)
    assert ref.same(_host(got), cases.expected(d))
    for e in got:
        if e is not None:
            assert all(v.is_cuda for v in e.values()) and e["mask"].dtype.is_floating_point and e["mask"].dim() == 2
    # two calls on the same input give equal bytes
    again = _call(d)
    for a, b in zip(_host(got), _host(again)):
        assert (a is None) == (b is None)
        if a is not None:
            assert all(ref.bits(a[k]).tobytes() == ref.bits(b[k]).tobytes() for k in a)
    if d.spps is not None:
        assert ref.same(_host(_call(d, strict=True)), cases.expected(d, strict=True))


@pytest.mark.parametrize("name", ref.FIXTURES)
def test_fixture_equals_the_reference(name):
    from gapro_amd import consumer_ops as ops

    z, want = ref.fixture(name)
    B = int(z["batch_size"])
    args = (_dev(z["cls"]), _dev(z["box"]), _dev(z["offsets"]), B)
    if name == "subsample":
        got = ops.get_subsample_gt(_dev(z["labels"]), _dev(z["subsample_idxs"]), *args)
        ours = ref.get_subsample_gt(z["labels"], z["subsample_idxs"], z["cls"], z["box"], z["offsets"], B)
    else:
        got = ops.get_spp_gt(_dev(z["labels"]), _dev(z["spps"]), *args)  # n_spps from the data, as the reference
        ours = ref.get_spp_gt(z["labels"], z["spps"], z["cls"], z["box"], z["offsets"], B)
    assert all(e is None or sorted(e) == ["box", "cls", "mask"] for e in got)
    assert ref.same(_host(got), want) and ref.same(_host(got), ours)


@pytest.mark.parametrize("label_dtype", ["int32", "int64", "float64"])
@pytest.mark.parametrize("spp_dtype", ["int32", "int64", "int16"])
@pytest.mark.parametrize("cls_dtype", ["int64", "int32"])
def test_each_dtype(label_dtype, spp_dtype, cls_dtype):
    import torch
    from gapro_amd import consumer_ops as ops

    d = cases.build("bit-word edges")
    want = cases.expected(d)
    got = ops.get_spp_gt(_dev(d.labels, getattr(torch, label_dtype)), _dev(d.spps, getattr(torch, spp_dtype)),
                         _dev(d.cls, getattr(torch, cls_dtype)), _dev(d.box), _dev(d.offsets), d.batch_size,
                         n_spps=d.n_spps, return_ids=True)
    for e in want:
        e["cls"] = e["cls"].astype(getattr(np, cls_dtype))
    assert ref.same(_host(got), want)


def test_offsets_in_every_form_and_n_spps_from_the_data():
    import torch

    d = cases.build("a superpoint id shared by two samples")
    want = cases.expected(d)
    for off in (_dev(d.offsets, torch.int32), torch.from_numpy(d.offsets.copy()), [int(v) for v in d.offsets],
                tuple(d.offsets.tolist()), _dev(d.offsets)):
        assert ref.same(_host(_call(d, offsets=off)), want)
    from gapro_amd import consumer_ops as ops
    got = ops.get_spp_gt(_dev(d.labels), _dev(d.spps), _dev(d.cls), _dev(d.box), _dev(d.offsets), d.batch_size)
    assert ref.same(_host(got), want)
    # a strided view of the labels and another stream
    wide = _dev(np.stack([d.labels, d.labels + 1000], axis=1))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = _call(d, labels=wide[:, 0])
    s.synchronize()
    assert not wide[:, 0].is_contiguous() and ref.same(_host(got), want)


def test_return_ids_and_views_into_one_allocation():
    d = cases.build("bit-word edges")
    got = _call(d, return_ids=True)
    cls, box = _dev(d.cls), _dev(d.box)
    kept = [e for e in got if e is not None]
    assert len(kept) == 3
    for e in kept:
        ids = e["ids"]
        assert ids.dtype == cls.dtype and bool((cls[ids] == e["cls"]).all())
        assert np.array_equal(ref.bits(box[ids].cpu().numpy()), ref.bits(e["box"].cpu().numpy()))
        assert bool((ids[1:] > ids[:-1]).all())
    for k in ("mask", "cls", "box", "ids"):
        assert len({e[k].untyped_storage().data_ptr() for e in kept}) == 1, k
    assert all("ids" not in e for e in _call(d, return_ids=False) if e is not None)


@pytest.mark.parametrize("name", cases.REFUSED_NAMES)
def test_refusal_names_the_cause_and_writes_nothing(name):
    """Through the wrapper: a GaproError that names the cause and the sample.  At the C ABI, where the caller owns the
    outputs: a status in the header of the count, and a fill on that workspace writes nothing."""
    import torch
    from gapro_amd import _lib

    d = cases.build(name)
    code, flag, bad_sample = cases.REFUSALS[name[len("refused: "):]]
    with pytest.raises(_lib.GaproError) as e:
        _call(d)
    cause = {ref.FLAG_OFFSETS: "offsets", ref.FLAG_GATHER: "subsample index", ref.FLAG_LABEL: "label",
             ref.FLAG_SPP: "superpoint id"}[flag]
    assert e.value.code == code and cause in str(e.value) and "sample %d" % bad_sample in str(e.value), e.value

    ctx = _lib.Context.get(0)
    lib = ctx.lib
    sub = d.spps is None
    labels, cls, box, off = _dev(d.labels), _dev(d.cls), _dev(d.box), _dev(d.offsets)
    second = _dev(d.idxs if sub else d.spps)
    n, n_labels, B = len(d.idxs if sub else d.labels), len(d.labels), d.batch_size
    code_of = {np.dtype(np.int64): _lib.GAPRO_LABEL_I64, np.dtype(np.float64): _lib.GAPRO_LABEL_F64}[d.labels.dtype]
    ws_bytes = int(lib.gapro_spp_gt_workspace_bytes(n, B, len(d.cls), d.n_spps))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda:0")
    hdr_bytes = C.sizeof(_lib.SppGtHeader) + 8 * B
    d_hdr = torch.zeros(hdr_bytes, dtype=torch.uint8, device="cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    common = (n, n_labels, labels.data_ptr(), code_of, second.data_ptr() if sub else None,
              None if sub else second.data_ptr(), 0 if sub else 1, d.n_spps, cls.data_ptr(), _lib.GAPRO_LABEL_I64,
              len(d.cls))
    assert lib.gapro_spp_gt_count(ctx.handle, stream, *common, off.data_ptr(), B, d.ignore, ws.data_ptr(), ws_bytes,
                                  d_hdr.data_ptr(), None) == 0  # enqueued: the refusal is the header's
    cells, rows = 4096, 64
    outs = [torch.full((cells,), 77.0, dtype=torch.float32, device="cuda:0"),
            torch.full((rows,), 77, dtype=torch.int64, device="cuda:0"),
            torch.full((rows, 6), 77.0, dtype=torch.float32, device="cuda:0"),
            torch.full((rows,), 77, dtype=torch.int64, device="cuda:0")]
    assert lib.gapro_spp_gt_fill(ctx.handle, stream, *common, box.data_ptr(), off.data_ptr(), B, d.ignore, 0,
                                 ws.data_ptr(), ws_bytes, outs[0].data_ptr(), cells, outs[1].data_ptr(),
                                 outs[2].data_ptr(), outs[3].data_ptr(), rows, d_hdr.data_ptr()) == 0
    torch.cuda.synchronize()
    raw = d_hdr.cpu().numpy().tobytes()
    hdr = _lib.SppGtHeader.from_buffer_copy(raw)
    assert (hdr.status, hdr.bad_sample, hdr.batch_size) == (code, bad_sample, B) and hdr.flags & flag
    assert hdr.flags & (flag - 1) == 0  # no cause of a higher precedence
    for o in outs:
        assert bool((o == 77).all())
    # refused before anything is launched: a small workspace, an unknown label type, an unknown rule
    fill_tail = (box.data_ptr(), off.data_ptr(), B, d.ignore)
    out_tail = (outs[0].data_ptr(), cells, outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), rows, None)
    assert lib.gapro_spp_gt_count(ctx.handle, stream, *common, off.data_ptr(), B, d.ignore, ws.data_ptr(), ws_bytes - 1,
                                  d_hdr.data_ptr(), None) == -7
    assert lib.gapro_spp_gt_count(ctx.handle, stream, n, n_labels, labels.data_ptr(), 9, *common[4:], off.data_ptr(), B,
                                  d.ignore, ws.data_ptr(), ws_bytes, d_hdr.data_ptr(), None) == -1
    assert lib.gapro_spp_gt_fill(ctx.handle, stream, *common, *fill_tail, 2, ws.data_ptr(), ws_bytes, *out_tail) == -1


def test_fill_with_too_few_cells_reports_and_writes_nothing():
    import torch
    from gapro_amd import _lib

    d = cases.build("batch of one")
    want = cases.expected(d)[0]
    ctx = _lib.Context.get(0)
    lib = ctx.lib
    labels, spps, cls, box, off = (_dev(a) for a in (d.labels, d.spps, d.cls, d.box, d.offsets))
    n = len(d.labels)
    ws_bytes = int(lib.gapro_spp_gt_workspace_bytes(n, 1, len(d.cls), d.n_spps))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda:0")
    d_hdr = torch.zeros(C.sizeof(_lib.SppGtHeader) + 8, dtype=torch.uint8, device="cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    common = (n, n, labels.data_ptr(), _lib.GAPRO_LABEL_I64, None, spps.data_ptr(), 1, d.n_spps, cls.data_ptr(),
              _lib.GAPRO_LABEL_I64, len(d.cls))
    assert lib.gapro_spp_gt_count(ctx.handle, stream, *common, off.data_ptr(), 1, d.ignore, ws.data_ptr(), ws_bytes,
                                  d_hdr.data_ptr(), None) == 0
    torch.cuda.synchronize()
    hdr = _lib.SppGtHeader.from_buffer_copy(d_hdr.cpu().numpy().tobytes())
    rows, cols = want["mask"].shape
    assert (hdr.status, hdr.total_rows, hdr.total_cols, hdr.total_cells) == (0, rows, cols, rows * cols)
    assert np.frombuffer(d_hdr.cpu().numpy().tobytes(), dtype=np.int32, offset=40).tolist() == [rows, cols]
    mask = torch.full((rows * cols,), 77.0, dtype=torch.float32, device="cuda:0")
    ids = torch.full((rows,), 77, dtype=torch.int64, device="cuda:0")
    for cells_given, rows_given in ((rows * cols - 1, rows), (rows * cols, rows - 1)):
        assert lib.gapro_spp_gt_fill(ctx.handle, stream, *common, None, off.data_ptr(), 1, d.ignore, 0, ws.data_ptr(),
                                     ws_bytes, mask.data_ptr(), cells_given, None, None, ids.data_ptr(), rows_given,
                                     d_hdr.data_ptr()) == 0
        torch.cuda.synchronize()
        assert _lib.SppGtHeader.from_buffer_copy(d_hdr.cpu().numpy().tobytes()).status == -7
        assert bool((mask == 77).all()) and bool((ids == 77).all())
    # the exact sizes: the mask and the ids alone, no cls and no box wanted
    assert lib.gapro_spp_gt_fill(ctx.handle, stream, *common, None, off.data_ptr(), 1, d.ignore, 0, ws.data_ptr(),
                                 ws_bytes, mask.data_ptr(), rows * cols, None, None, ids.data_ptr(), rows, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(mask.cpu().numpy().reshape(rows, cols), want["mask"])
    assert np.array_equal(ids.cpu().numpy(), want["ids"])
