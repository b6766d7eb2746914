"""csrc/proposals.hip on the MI355X beyond the first trip of its loops: get_instance, mask_nms and rle_encode_gpu_batch
against the NumPy restatement on ``scale_cases()`` of tests/proposals_cases.py (DESIGN.md 4.8 lists loop -> case;
tests/test_proposals_scale_cpu.py shows that each case tells a first-trip-only kernel from the definition).

The comparison is that of tests/test_proposals_gpu.py, whose helpers are used: everything bit for bit, ``conf`` within
one float32 ulp of the float64 expression rounded once.
"""
import functools
import types

import numpy as np
import pytest

import proposals_cases as cases
import proposals_ref as ref
from test_proposals_gpu import _call, _check, _dev, _host, _ulp_apart

pytestmark = pytest.mark.gpu

_BYTES = ("conf", "label_id", "box", "query", "runs", "masks")
LARGE_N = tuple(n for n in cases.SCALE_NAMES if n.startswith("points_"))
FULL_SORTS = tuple(n for n in cases.SCALE_NAMES if n.startswith(("p1024_", "nms_victims_")))


@pytest.mark.parametrize("name", cases.SCALE_NAMES)
def test_case_equals_the_restatement(name):
    c, want = cases.scale_case(name), cases.scale_reference(name)
    got = _host(_call(c, return_arrays=True, return_masks=True))
    _check(got, want, len(c["v2p_map"]))
    again = _host(_call(c, return_arrays=True, return_masks=True))  # two runs give the same bytes
    assert all(got[k].tobytes() == again[k].tobytes() for k in _BYTES)
    if c.get("voxel_spps") is not None:  # the other form of mask_logits gives the same bytes
        wide = dict(c, mask_logits=np.ascontiguousarray(c["mask_logits"][:, c["voxel_spps"]]), voxel_spps=None)
        other = _host(_call(wide, return_arrays=True, return_masks=True))
        assert all(got[k].tobytes() == other[k].tobytes() for k in _BYTES)


@pytest.mark.parametrize("name", LARGE_N + FULL_SORTS)
def test_the_list_equals_the_restatement(name):
    c, want = cases.scale_case(name), cases.scale_reference(name)
    got = _call(c)
    n_sem = len(c.get("sem2ins_classes", ()))
    assert len(got) == len(want["conf"]) > 0
    assert [int(g["label_id"]) for g in got] == want["label_id"].tolist()
    assert all(g["conf"] == 1.0 and isinstance(g["conf"], float) for g in got[:n_sem])
    assert (_ulp_apart(np.array([g["conf"] for g in got], np.float32), want["conf"]) <= 1).all()
    for g, counts in zip(got, want["counts"]):
        assert g["pred_mask"]["length"] == len(c["v2p_map"]) and g["pred_mask"]["counts"].dtype == np.int64
        assert np.array_equal(g["pred_mask"]["counts"], counts)


def test_one_score_beyond_the_cap_is_refused():
    import torch

    from gapro_amd import consumer_ops as ops

    Q = cases.MAX_SCORES + 1
    zeros = functools.partial(torch.zeros, device="cuda:0")
    with pytest.raises(ValueError, match="beyond the library's bounds"):
        ops.get_instance("scene", zeros((Q, 2)), zeros((Q, 1)), zeros(Q), zeros((Q, 6)), zeros(4, dtype=torch.int64),
                         None, zeros(4, dtype=torch.int64), instance_classes=1, voxel_spps=zeros(4, dtype=torch.int64),
                         n_spps=1, npoint_thresh=1)


@functools.lru_cache(maxsize=None)
def _nms_1024():
    """The 1024 proposals in a shuffled order (mask_nms sorts) and what ``nms_ref`` keeps of them in stage order."""
    bits, cat, score, box = cases.nms_1024_inputs()
    order = ref.order_ref(score, len(score))
    want = {}
    for kind in ("matrix", "standard"):
        keep, conf = ref.nms_ref(bits[order], cat[order], score[order], kind, -1, 0.2)
        want[kind] = (order[keep], conf)
    return bits, cat, score, box, want


@pytest.mark.parametrize("kind", ("matrix", "standard"))
def test_mask_nms_of_1024_proposals_equals_the_restatement(kind):
    import torch

    from gapro_amd import consumer_ops as ops

    bits, cat, score, box, want = _nms_1024()
    rows, conf = want[kind]
    cfg = types.SimpleNamespace(type_nms=kind, topk=-1, nms_threshold=0.2)
    m, k, s, b = ops.mask_nms(_dev(bits), _dev(cat), _dev(score), _dev(box), cfg)
    assert m.dtype == torch.bool and np.array_equal(m.cpu().numpy(), bits[rows])
    assert k.dtype == torch.int64 and np.array_equal(k.cpu().numpy(), cat[rows])
    assert s.shape == (len(rows),) and (_ulp_apart(s.cpu().numpy(), conf) <= 1).all()
    assert b.cpu().numpy().tobytes() == box[rows].tobytes()
    m2, _, s2, _ = ops.mask_nms(_dev(bits), _dev(cat), _dev(score), _dev(box), cfg)
    assert torch.equal(m, m2) and s.cpu().numpy().tobytes() == s2.cpu().numpy().tobytes()


@pytest.mark.parametrize("n_points", cases.RLE_POINTS)
def test_rle_encode_gpu_batch_at_and_beyond_the_chunk_cap(n_points):
    """The rows of the large scene: all ones, alternating every point, runs that start and end next to every chunk."""
    from gapro_amd import consumer_ops as ops

    want = cases.scale_reference("points_%d" % n_points)
    got = ops.rle_encode_gpu_batch(_dev(want["masks"]))
    assert len(got) == len(want["masks"]) == 4
    for g, m, counts in zip(got, want["masks"], want["counts"]):
        assert g["length"] == n_points and g["counts"].dtype == np.int64
        assert np.array_equal(g["counts"], counts)
    again = ops.rle_encode_gpu_batch(_dev(want["masks"]))
    assert all(np.array_equal(a["counts"], g["counts"]) for a, g in zip(again, got))
