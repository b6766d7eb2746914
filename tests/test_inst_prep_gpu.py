"""gapro_inst_crop / gapro_inst_info / gapro_inst_prepare on the MI355X: consumer_ops.get_cropped_instance_label,
get_instance_info and prepare_instance_labels, bit for bit against the NumPy restatement tests/inst_prep_ref.py on the
edge cases of tests/inst_prep_cases.py, and against the outputs of the real reference (tests/golden/inst_prep_*.npz).

Everything but the centroid is integer-exact or one float32 operation: array_equal against the goldens.  The centroid
is the exact mean where the reference's float32 mean has no stated order: 4 x the largest difference
make_golden_inst_prep.py measured (inst_prep_summary.npz) is allowed against the goldens, none against the restatement.
"""
import ctypes as C

import numpy as np
import pytest

import inst_prep_cases as cases
import inst_prep_ref as ref

pytestmark = pytest.mark.gpu


def _dev(a, dtype=None):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    return t if dtype is None else t.to(dtype)


def _np(t):
    return t.cpu().numpy()


def _same(got, want):
    got = _np(got)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(ref.bits(got), ref.bits(want))


def _refused(code, fn, *args):
    from gapro_amd._lib import GaproError

    with pytest.raises(GaproError) as e:
        fn(*args)
    assert e.value.code == code, e.value


def _check_prepared(got, want):
    import torch

    assert type(got).__name__ == "InstanceLabels" and len(got) == 6
    assert got.instance_cls.dtype == torch.int64 and got.instance_pointnum.dtype == torch.int32
    for g, w in zip(got, want):
        assert g.is_cuda
        _same(g, w)


@pytest.mark.parametrize("name", cases.CASE_NAMES)
def test_case_equals_the_restatement(name):
    from gapro_amd import consumer_ops as ops

    d = cases.build(name)
    xyz, sem = _dev(d.coords), _dev(d.sem)

    # the crop, in place
    want = cases.expected(ref.get_cropped_instance_label, d.inst)
    t = _dev(d.inst)
    if isinstance(want, ref.Refused):
        _refused(want.code, ops.get_cropped_instance_label, t)
        _same(t, d.inst)
    else:
        assert ops.get_cropped_instance_label(t) is t
        _same(t, want)

    # the chain
    want = cases.expected(ref.prepare_instance_labels, d.coords, d.inst, d.sem, d.shift)
    t = _dev(d.inst)
    if isinstance(want, ref.Refused):
        _refused(want.code, ops.prepare_instance_labels, xyz, t, sem, d.shift)
    else:
        got = ops.prepare_instance_labels(xyz, t, sem, d.shift)
        _check_prepared(got, want)
        assert got.instance_labels.data_ptr() != t.data_ptr()
        # two runs give the same bits
        for g, a in zip(got, ops.prepare_instance_labels(xyz, t, sem, d.shift)):
            assert np.array_equal(ref.bits(_np(g)), ref.bits(_np(a)))
        # the fused call equals the two separate calls
        lab = ops.get_cropped_instance_label(_dev(d.inst))
        cls, box, cen, cor = ops.get_instance_info(xyz, lab, sem, d.shift)
        for g, a in zip((got.instance_labels, got.instance_cls, got.instance_box, got.centroid_offset_labels,
                         got.corners_offset_labels), (lab, cls, box, cen, cor)):
            assert g.dtype == a.dtype and np.array_equal(ref.bits(_np(g)), ref.bits(_np(a)))
    _same(t, d.inst)  # the chain works on a copy, whatever comes of it

    # get_instance_info on the labels as they are: refused where an id below the largest is empty
    want = cases.expected(ref.get_instance_info, d.coords, d.inst, d.sem, d.shift)
    if isinstance(want, ref.Refused):
        _refused(want.code, ops.get_instance_info, xyz, t, sem, d.shift)
    else:
        for g, w in zip(ops.get_instance_info(xyz, t, sem, d.shift), want):
            _same(g, w)
    _same(t, d.inst)


@pytest.mark.parametrize("name", ref.FIXTURES)
def test_fixture_equals_the_reference(name):
    import torch
    from gapro_amd import consumer_ops as ops

    z = ref.fixture(name)
    tol = ref.centroid_tolerance()
    shift = int(z["label_shift"])
    for dt in (torch.int64, torch.int32, torch.float64):
        t = _dev(z["inst"], dt)
        assert ops.get_cropped_instance_label(t) is t and t.dtype == dt
        assert np.array_equal(_np(t), z["cropped"])
        # in place against valid_idxs: the indexed copy is compacted, the given tensor stays
        t = _dev(z["inst"], dt)
        for valid in (_dev(z["valid"]), z["valid"]):
            out = ops.get_cropped_instance_label(t, valid)
            assert out.dtype == dt and np.array_equal(_np(out), z["cropped_valid"])
            assert np.array_equal(_np(t), z["inst"])
    xyz, sem = _dev(z["coords"]), _dev(z["sem"])
    got = ops.prepare_instance_labels(xyz, _dev(z["inst"]), sem, shift)
    two = ops.get_instance_info(xyz, _dev(z["cropped"]), sem, label_shift=shift)
    for labels, cls, box, cen, cor in ((got.instance_labels, got.instance_cls, got.instance_box,
                                        got.centroid_offset_labels, got.corners_offset_labels),
                                       (_dev(z["cropped"]),) + tuple(two)):
        assert np.array_equal(_np(labels), z["cropped"]) and np.array_equal(_np(cls), z["cls"])
        assert np.array_equal(_np(box), z["box"]) and np.array_equal(_np(cor), z["corners_offset"])
        cen = _np(cen).astype(np.float64)
        err = float(np.max(np.abs(cen - z["centroid_offset"].astype(np.float64))))
        print("%s: max |centroid offset - reference| = %.3g (allowed %.3g)" % (name, err, tol))
        assert np.array_equal(cen == -100.0, z["centroid_offset"] == -100.0) and err <= tol
    assert np.array_equal(_np(got.instance_pointnum), z["pointnum"])
    _check_prepared(got, ref.prepare_instance_labels(z["coords"], z["inst"], z["sem"], shift))


@pytest.mark.parametrize("label_dtype", ["int32", "int64", "float64"])
@pytest.mark.parametrize("sem_dtype", ["int32", "int64", "float64"])
def test_each_label_dtype(label_dtype, sem_dtype):
    import torch
    from gapro_amd import consumer_ops as ops

    d = cases.build("consecutive holes")
    ldt, sdt = getattr(torch, label_dtype), getattr(torch, sem_dtype)
    want = ref.prepare_instance_labels(d.coords, d.inst, d.sem, 2)
    got = ops.prepare_instance_labels(_dev(d.coords), _dev(d.inst, ldt), _dev(d.sem, sdt), 2)
    assert got.instance_labels.dtype == ldt
    _check_prepared(got, (want[0].astype(getattr(np, label_dtype)),) + want[1:])
    if label_dtype == "float64":  # NaN names no instance; a label that is no integer is refused, nothing is written
        lab = d.inst.astype(np.float64)
        lab[d.inst < 0] = np.nan
        got = ops.prepare_instance_labels(_dev(d.coords), _dev(lab), _dev(d.sem, sdt), 2)
        assert np.array_equal(np.isnan(_np(got.instance_labels)), d.inst < 0)
        for g, w in zip(got[1:], want[1:]):
            _same(g, w)
        lab = d.inst.astype(np.float64)
        lab[np.nonzero(d.inst >= 0)[0][3]] = 1.5
        t = _dev(lab)
        _refused(ref.BAD_ARG, ops.get_cropped_instance_label, t)
        _same(t, lab)


def test_strided_labels_other_stream_and_the_gen_ps_utils_name():
    import torch
    from gapro_amd import consumer_ops as ops
    from gapro_amd import gen_ps_utils

    d = cases.build("ids on both sides of the LDS table's edge")
    want = ref.prepare_instance_labels(d.coords, d.inst, d.sem, d.shift)
    # a strided view is cropped in place through a contiguous copy
    wide = _dev(np.stack([d.inst, d.inst + 1000], axis=1))
    col = wide[:, 0]
    assert not col.is_contiguous() and ops.get_cropped_instance_label(col) is col
    assert np.array_equal(_np(wide[:, 0]), want[0]) and np.array_equal(_np(wide[:, 1]), d.inst + 1000)
    # the work goes to the caller's current stream
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        xyz, inst, sem = _dev(d.coords), _dev(d.inst), _dev(d.sem)
        got = ops.prepare_instance_labels(xyz, inst, sem, d.shift)
    s.synchronize()
    _check_prepared(got, want)
    # gen_ps_utils: NumPy and host tensors go to the device and back, in place as in the reference
    a = d.inst.copy()
    assert gen_ps_utils.get_cropped_instance_label(a) is a and np.array_equal(a, want[0])
    t = torch.from_numpy(d.inst.copy())
    assert gen_ps_utils.get_cropped_instance_label(t) is t and np.array_equal(t.numpy(), want[0])
    valid = np.arange(0, len(d.inst), 3)
    a = d.inst.copy()
    out = gen_ps_utils.get_cropped_instance_label(a, valid)
    assert np.array_equal(out, ref.get_cropped_instance_label(d.inst, valid)) and np.array_equal(a, d.inst)
    g = _dev(d.inst)
    assert gen_ps_utils.get_cropped_instance_label(g) is g and np.array_equal(_np(g), want[0])


@pytest.mark.parametrize("name,entry,code", [
    ("non-finite coordinate on a labelled point", "prepare", ref.NOT_FINITE),
    ("non-finite coordinate on a labelled point", "info", ref.NOT_FINITE),
    ("consecutive holes", "info", ref.BAD_ARG),
    ("only negative labels", "prepare", ref.BAD_ARG),
    ("an id at the refusal bound", "crop", ref.BAD_ARG),
    ("ids on both sides of the id table's capacity", "prepare", -7),  # GAPRO_ERR_WORKSPACE: the caller regrows
])
def test_a_refused_call_leaves_labels_and_outputs_untouched(name, entry, code):
    """At the C ABI, where the caller owns the outputs: a status in the header, nothing written."""
    import torch
    from gapro_amd import _lib

    d = cases.build(name)
    inst = d.inst.copy()
    if name.startswith("non-finite") and entry == "info":
        inst = ref.get_cropped_instance_label(inst)  # no hole: the coordinate alone is the reason
    ctx = _lib.Context.get(0)
    lib = ctx.lib
    cap, n = cases.ID_TABLE, len(inst)
    xyz, lab, sem = _dev(d.coords), _dev(inst), _dev(d.sem)
    ws_bytes = int(lib.gapro_inst_prep_workspace_bytes(cap))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda:0")
    outs = [torch.full((cap,), 77, dtype=torch.int64, device="cuda:0"),
            torch.full((cap, 6), 77.0, dtype=torch.float32, device="cuda:0"),
            torch.full((cap,), 77, dtype=torch.int32, device="cuda:0"),
            torch.full((n, 3), 77.0, dtype=torch.float32, device="cuda:0"),
            torch.full((n, 6), 77.0, dtype=torch.float32, device="cuda:0")]
    d_hdr = torch.zeros(C.sizeof(_lib.InstPrepHeader), dtype=torch.uint8, device="cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if entry == "crop":
        rc = lib.gapro_inst_crop(ctx.handle, stream, n, lab.data_ptr(), _lib.GAPRO_LABEL_I64, cap, ws.data_ptr(), ws_bytes,
                                 d_hdr.data_ptr(), None)
    else:
        fn = lib.gapro_inst_prepare if entry == "prepare" else lib.gapro_inst_info
        rc = fn(ctx.handle, stream, n, xyz.data_ptr(), lab.data_ptr(), _lib.GAPRO_LABEL_I64, sem.data_ptr(),
                _lib.GAPRO_LABEL_I64, d.shift, cap, ws.data_ptr(), ws_bytes, *(o.data_ptr() for o in outs),
                d_hdr.data_ptr(), None)
    assert rc == 0  # enqueued: the refusal is the header's
    torch.cuda.synchronize()
    hdr = _lib.InstPrepHeader.from_buffer_copy(_np(d_hdr).tobytes())
    assert hdr.status == code
    assert hdr.max_id == min(int(inst.max()), _lib.INST_PREP_MAX_IDS) and hdr.n_ids <= cap
    assert np.array_equal(_np(lab), inst)
    for o in outs:
        assert bool((o == 77).all())
    # a workspace that is too small, or an id table beyond the bound, is refused before anything is launched
    assert lib.gapro_inst_crop(ctx.handle, stream, n, lab.data_ptr(), _lib.GAPRO_LABEL_I64, cap, ws.data_ptr(),
                               ws_bytes - 1, d_hdr.data_ptr(), None) == -7
    assert lib.gapro_inst_crop(ctx.handle, stream, n, lab.data_ptr(), 9, cap, ws.data_ptr(), ws_bytes, d_hdr.data_ptr(),
                               None) == -1
    assert lib.gapro_inst_crop(ctx.handle, stream, n, lab.data_ptr(), _lib.GAPRO_LABEL_I64, _lib.INST_PREP_MAX_IDS + 1,
                               ws.data_ptr(), ws_bytes, d_hdr.data_ptr(), None) == -1
