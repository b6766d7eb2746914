"""The heuristic labelers (gapro_label_heuristic) and getInstanceInfo (gapro_instance_info) at their kernel edges, integer
for integer and bit for bit against the oracle: occupancy words past the first, the first-wins and threshold rules, the
rank scan of "dist", the rounding of its squared distance, the grid-stride loops, the id tables, and every refusal.

The inputs come from labeler_cases.py; test_labeler_edges_cpu.py proves on the CPU that each is what it claims and that
the oracle's answers are those of a literal per-point reference, so that nothing here passes vacuously."""
import ctypes as C

import numpy as np
import pytest

import labeler_cases as lc

pytestmark = pytest.mark.gpu

BAD_ARG, WORKSPACE = -1, -7
CANARY = 0x5A5A5A5A


# ------------------------------------------------------------------------------------------ the labelers
def _run(case, labeler, dataset_name):
    from gapro_amd.gen_ps_utils import gen_pseudo_label, gen_pseudo_label_box2mask

    if labeler == "box2mask":
        sem, inst = gen_pseudo_label_box2mask(*lc.args_of(case), dataset_name=dataset_name)
    else:
        sem, inst = gen_pseudo_label(*lc.args_of(case), dataset_name=dataset_name, heuristic_rule=labeler)
    return sem.cpu().numpy(), inst.cpu().numpy()


@pytest.mark.parametrize("name", lc.LABELER_CASE_NAMES)
def test_labelers_equal_the_oracle(name):
    """No tolerance, no left-out point, no tie allowance: the kernels are integer-exact by contract."""
    case, ref = lc.labeler_case(name), lc.oracle_labels(name)
    wrong = []
    for labeler in case.labelers:
        for ds in lc.DATASETS:
            sem, inst = _run(case, labeler, ds)
            assert sem.dtype == inst.dtype == np.int32 and sem.shape == inst.shape == (len(case.coords),)
            bad_sem, bad_inst = int((sem != ref[labeler, ds][0]).sum()), int((inst != ref[labeler, ds][1]).sum())
            if bad_sem or bad_inst:
                wrong.append("%s/%s: %d sem and %d inst of %d points differ" % (labeler, ds, bad_sem, bad_inst, len(sem)))
    assert not wrong, wrong


def test_257_boxes_are_refused_by_the_python_entry_points():
    from gapro_amd._lib import GaproError
    from gapro_amd.gen_ps_utils import gen_pseudo_label, gen_pseudo_label_box2mask

    most = lc.labeler_case("boxes_256")
    assert len(most.box) == lc.LAB_MAX_BOXES
    box, vol, cls = (np.concatenate([a, a[:1]]) for a in (most.box, most.vol, most.cls))
    for ds in lc.DATASETS:
        for rule in ("volume", "dist", "none"):
            out = None
            with pytest.raises(GaproError) as e:
                out = gen_pseudo_label(most.coords, most.spp, cls, box, vol, dataset_name=ds, heuristic_rule=rule)
            assert e.value.code == BAD_ARG and out is None
        with pytest.raises(GaproError) as e:
            out = gen_pseudo_label_box2mask(most.coords, most.spp, cls, box, vol, dataset_name=ds)
        assert e.value.code == BAD_ARG and out is None


def _context():
    from gapro_amd._lib import Context

    return Context.get(0)


def test_label_heuristic_refusals_leave_the_outputs_untouched():
    """include/gapro_hip.h: a non-positive or oversized argument is GAPRO_ERR_BAD_ARG, a short workspace
    GAPRO_ERR_WORKSPACE; nothing is launched.  Every buffer is sized for 257 boxes, whatever the call claims."""
    import torch

    ctx = _context()
    lib, dev = ctx.lib, torch.device("cuda", 0)
    n, nb = 100, 3
    rng = np.random.default_rng(0)
    coords = torch.from_numpy(rng.uniform(0, 1, size=(n, 3))).to(dev)
    box = torch.zeros((257, 6), dtype=torch.float32, device=dev)
    box[:, 3:] = 1.0
    vol = torch.ones(257, dtype=torch.float32, device=dev)
    cls = torch.zeros(257, dtype=torch.int64, device=dev)
    spp_inv = torch.zeros(n, dtype=torch.int32, device=dev)
    full = int(lib.gapro_label_heuristic_workspace_bytes(n, 1, 257))
    ws = torch.empty(full, dtype=torch.uint8, device=dev)
    need = int(lib.gapro_label_heuristic_workspace_bytes(n, 1, nb))
    assert 0 < need <= full
    sem = torch.full((n,), CANARY, dtype=torch.int32, device=dev)
    inst = torch.full((n,), CANARY, dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call(n_points=n, n_boxes=nb, rule=0, align=1, spp=spp_inv.data_ptr(), ws_bytes=need):
        rc = lib.gapro_label_heuristic(ctx.handle, stream, n_points, coords.data_ptr(), spp, 1, n_boxes, box.data_ptr(),
                                       vol.data_ptr(), cls.data_ptr(), rule, align, 18, ws.data_ptr(), ws_bytes,
                                       sem.data_ptr(), inst.data_ptr())
        torch.cuda.synchronize()
        return rc

    refused = [(dict(n_boxes=0), BAD_ARG), (dict(n_boxes=257, ws_bytes=full), BAD_ARG), (dict(rule=-1), BAD_ARG),
               (dict(rule=4), BAD_ARG), (dict(n_points=0), BAD_ARG), (dict(align=1, spp=None), BAD_ARG),
               (dict(ws_bytes=need - 1), WORKSPACE)]
    for kw, want in refused:
        assert call(**kw) == want, kw
        assert bool((sem == CANARY).all()) and bool((inst == CANARY).all()), kw
    # the same buffers are accepted as they stand, also without superpoints when nothing is aligned
    assert call(align=0, spp=None) == 0
    assert bool((inst.cpu() == 0).all()) and bool((sem.cpu() == 0).all())  # every point inside box 0, the first of three
    assert call() == 0


def test_instance_info_refusals_leave_the_outputs_untouched():
    import torch

    from gapro_amd._lib import InstanceHeader

    ctx = _context()
    lib, dev = ctx.lib, torch.device("cuda", 0)
    n, cap = 64, 16
    rng = np.random.default_rng(1)
    coords = torch.from_numpy(rng.uniform(0, 1, size=(n, 3))).to(dev)
    inst = torch.from_numpy((np.arange(n) % 4).astype(np.float64)).to(dev)
    sem = torch.full((n,), 5.0, dtype=torch.float64, device=dev)
    need = int(lib.gapro_instance_info_workspace_bytes(cap))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    outs = [torch.full(shape, -7.5, dtype=dt, device=dev) for shape, dt in
            (((cap, 6), torch.float64), ((cap,), torch.float64), ((cap,), torch.float64), ((n, 6), torch.float32))]
    d_hdr = torch.full((C.sizeof(InstanceHeader),), 0x5A, dtype=torch.uint8, device=dev)
    h_hdr = torch.full((C.sizeof(InstanceHeader),), 0x5A, dtype=torch.uint8).pin_memory()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call(max_instances=cap, ws_bytes=need):
        rc = lib.gapro_instance_info(ctx.handle, stream, n, coords.data_ptr(), inst.data_ptr(), sem.data_ptr(),
                                     max_instances, 1, ws.data_ptr(), ws_bytes, outs[0].data_ptr(), outs[1].data_ptr(),
                                     outs[2].data_ptr(), outs[3].data_ptr(), d_hdr.data_ptr(), h_hdr.data_ptr())
        torch.cuda.synchronize()
        return rc

    for kw, want in ((dict(max_instances=0), BAD_ARG), (dict(ws_bytes=need - 1), WORKSPACE)):
        assert call(**kw) == want, kw
        assert all(bool((o == -7.5).all()) for o in outs), kw
        assert bool((d_hdr == 0x5A).all()) and bool((h_hdr == 0x5A).all()), kw
    assert call() == 0
    hdr = InstanceHeader.from_buffer_copy(h_hdr.numpy().tobytes())
    assert (hdr.instance_num, hdr.n_boxes, hdr.status) == (4, 4, 0)


# ------------------------------------------------------------------------------------------ getInstanceInfo
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize("dataset_name", ["scannetv2", "other"])
@pytest.mark.parametrize("name", lc.INSTANCE_CASE_NAMES)
def test_instance_info_equals_the_oracle(name, dataset_name):
    """Boxes, classes, volumes (float64) and corner labels (float32) are the oracle's values exactly (a zero may carry
    either sign: NumPy's minimum of -0.0 and +0.0 depends on their order).  The second call follows one that met ids
    beyond its first table in the regrow cases, and must see nothing of it: the same bits again."""
    from gapro_amd.gen_ps_utils import getInstanceInfo_device

    case = lc.instance_case(name)
    ref = lc.oracle_instance_info(name, dataset_name == "scannetv2")
    got = getInstanceInfo_device(case.xyz, case.inst, case.sem, dataset_name=dataset_name, return_corners=True)
    assert got[0] == ref[0]
    for a, b in zip(got[1:4], ref[1:4]):
        assert a.dtype == np.float64
        np.testing.assert_array_equal(a, b)
    assert got[4].dtype == np.float32 and got[4].shape == (len(case.xyz), 6)
    np.testing.assert_array_equal(got[4], ref[4])
    again = getInstanceInfo_device(case.xyz, case.inst, case.sem, dataset_name=dataset_name, return_corners=True)
    assert again[0] == got[0]
    for a, b in zip(again[1:], got[1:]):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    plain = getInstanceInfo_device(case.xyz, case.inst, case.sem, dataset_name=dataset_name)
    assert plain[4] is None
    for a, b in zip(plain[1:4], got[1:4]):
        np.testing.assert_array_equal(_bits(a), _bits(b))
