"""gapro_spp_vote on the MI355X: gen_ps_utils.spp_align_label / spp_major_voting against the reference's recorded outputs
(tests/golden/votes_<scene>.npz) and, bit for bit, against the NumPy restatement tests/vote_ref.py.

Labels are integer arithmetic: array_equal.  The probabilities are exact int64 sums followed by float64 operations in a
stated order, rounded once: bit-equal to the restatement.  Against the reference, which sums float32 in scatter order,
the tolerance is 4 x the largest difference make_golden_votes.py measured (votes_SUMMARY.json)."""
import ctypes as C

import numpy as np
import pytest

import vote_ref
from vote_ref import SCENES, fixture, prob_tolerance

pytestmark = pytest.mark.gpu


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check(spp, label, prob, occ, n_classes, occ_spp=None, label_arg=None):
    """Both functions on the device against the restatement: labels equal, probabilities the same bits."""
    import torch
    from gapro_amd.gen_ps_utils import spp_align_label, spp_major_voting

    label_arg = label if label_arg is None else label_arg
    lab, p = spp_major_voting(spp, label_arg, prob, occ, n_classes)
    w_lab, w_p = vote_ref.spp_major_voting(spp, label, prob, occ, n_classes)
    assert lab.dtype == torch.int64 and p.dtype == torch.float32 and lab.is_cuda and p.is_cuda
    assert np.array_equal(_np(lab), w_lab)
    assert np.array_equal(_bits(_np(p)), _bits(w_p))
    got = spp_align_label(spp, label_arg, n_classes)
    assert got.dtype == torch.int64 and np.array_equal(_np(got), vote_ref.spp_align_label(spp, label, n_classes))
    lab, p = spp_align_label(spp, label_arg, n_classes, occ_spp, prob)
    w_lab, w_p = vote_ref.spp_align_label(spp, label, n_classes, occ_spp, prob)
    assert np.array_equal(_np(lab), w_lab) and np.array_equal(_bits(_np(p)), _bits(w_p))
    return _np(lab), _np(p)


@pytest.mark.parametrize("name", SCENES)
def test_fixtures(name):
    import torch
    from gapro_amd.gen_ps_utils import spp_align_label, spp_major_voting

    d = fixture(name)
    n_classes = d["occ"].shape[1] + 1
    tol = prob_tolerance()
    rng = np.random.default_rng(5)
    S = int(d["ids"].max()) + 1
    # any ids, not ranks (ascending with the rank: the columns of bb_occupancy_spp follow the ascending ids)
    sparse = (np.sort(rng.choice(900000, S, replace=False)).astype(np.int64) + (1 << 40))[d["ids"]]
    for spp in (d["ids"], sparse):
        for label in (d["label"].astype(np.int64), d["label"].astype(np.int32)):
            lab, prob = spp_major_voting(spp, label, d["prob"], d["occ"], n_classes)
            assert np.array_equal(_np(lab), d["major_label"])
            assert np.max(np.abs(_np(prob).astype(np.float64) - d["major_prob"])) <= tol
            assert np.array_equal(_np(spp_align_label(spp, label)), d["align_label"])  # n_classes = -1
            assert np.array_equal(_np(spp_align_label(spp, label, n_classes, d["occ_spp"])), d["align_gated_label"])
            lab, prob = spp_align_label(spp, label, n_classes, prob_label=d["prob"])
            assert np.array_equal(_np(lab), d["align_label"])
            assert np.max(np.abs(_np(prob).astype(np.float64) - d["align_prob"])) <= tol
        _check(spp, d["label"], d["prob"], d["occ"], n_classes, d["occ_spp"])
    # device tensors in, the same out
    dev = torch.device("cuda", 0)
    lab, prob = spp_major_voting(torch.from_numpy(d["ids"]).to(dev), torch.from_numpy(d["label"]).to(dev),
                                 torch.from_numpy(d["prob"]).to(dev), torch.from_numpy(d["occ"]).to(dev), n_classes)
    assert np.array_equal(_np(lab), d["major_label"])


def _random_case(rng, n, S, C):
    spp = rng.integers(0, S, n) * 7 - 3
    label = rng.integers(0, C, n)
    prob = rng.random(n).astype(np.float32)
    occ = rng.random((n, C - 1)) < 0.8
    # half of the superpoints lie wholly inside every box, so that gates open as well
    occ[np.isin(spp, np.unique(spp)[::2])] = True
    occ_spp = rng.random((C - 1, len(np.unique(spp)))) < 0.6
    return spp, label, prob, occ, occ_spp


@pytest.mark.parametrize("n,S,C", [(1, 1, 1), (1, 1, 3), (63, 5, 4), (64, 5, 4), (65, 5, 4), (300, 7, 1), (300, 7, 64),
                                   (300, 7, 65), (300, 7, 66), (1000, 300, 2)])
def test_edge_shapes(n, S, C):
    rng = np.random.default_rng(100 * n + C)
    spp, label, prob, occ, occ_spp = _random_case(rng, n, S, C)
    _check(spp, label, prob, occ, C, occ_spp)
    _check(spp, label, prob, occ, C, occ_spp, label_arg=label.astype(np.int32))


def test_ids_of_any_range():
    """Ids that span far more than 4 N and 2^20 (the partition's rank table would refuse them), negative ones and the
    int64 extremes: the functions rank them like np.unique."""
    from gapro_amd.gen_ps_utils import spp_align_label

    lab = spp_align_label(np.array([0, 5_000_000]), np.array([1, 2]))
    assert _np(lab).tolist() == [1, 2]
    rng = np.random.default_rng(9)
    pool = np.array([-2 ** 63, -5_000_000_000, -1, 0, 7, 2 ** 20, 5_000_000, 2 ** 40, 2 ** 62, 2 ** 63 - 1], np.int64)
    n, C = 300, 5
    spp = pool[rng.integers(0, len(pool), n)]
    label, prob = rng.integers(0, C, n), rng.random(n).astype(np.float32)
    occ = rng.random((n, C - 1)) < 0.8
    occ[np.isin(spp, pool[::2])] = True
    occ_spp = rng.random((C - 1, len(np.unique(spp)))) < 0.6
    assert len(np.unique(spp)) == len(pool)
    _check(spp, label, prob, occ, C, occ_spp)


def test_ties_masks_and_single_points():
    # superpoint 5: an exact 2 : 2 tie between classes 1 and 2 -> 1;  9: every box class masked -> 0;  2: one point
    spp = np.array([5, 5, 5, 5, 9, 9, 2])
    label = np.array([2, 1, 2, 1, 1, 1, 2])
    prob = np.array([.25, .5, .75, 1, 0, .125, .0625], np.float32)
    occ = np.ones((7, 2), bool)
    occ[4, 0] = False  # a point of superpoint 9 outside box 0: its class 1 votes are masked
    gate = np.array([[1, 1, 0], [1, 1, 0]], bool)
    lab, _ = _check(spp, label, prob, occ, 3, gate)
    assert lab.tolist() == [1, 1, 1, 1, 0, 0, 2]
    from gapro_amd.gen_ps_utils import spp_major_voting
    lab, p = spp_major_voting(spp, label, prob, occ, 3)
    assert _np(lab).tolist() == [1, 1, 1, 1, 0, 0, 2]
    assert _np(p)[4] == 0 and _np(p)[6] == np.float32((0.0625 / (1 + 1e-4)) * 1.0)


def _raw(mode, ids, label, prob, gate, S, n_classes):
    """gapro_spp_vote itself on sentinel-filled outputs: (status, labels, probabilities)."""
    import torch
    from gapro_amd._lib import Context

    ctx = Context.get(0)
    lib = ctx.lib
    dev = torch.device("cuda", 0)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    n = len(ids)
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) if a is not None else None
         for a in (ids.astype(np.int32), label, prob, gate)]
    nbytes = int(lib.gapro_spp_vote_workspace_bytes(n, S, n_classes))
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out_l = torch.full((n + 4,), -7, dtype=torch.int64, device=dev)
    out_p = torch.full((n + 4,), -7.0, dtype=torch.float32, device=dev)
    status = torch.full((1,), 99, dtype=torch.int32, device=dev)
    ptr = [x.data_ptr() if x is not None else None for x in t]
    args = (ctx.handle, stream, mode, n, S, n_classes, ptr[0], ptr[1], 1 if label.dtype == np.int64 else 0, ptr[2], ptr[3],
            ws.data_ptr())
    tail = (out_l.data_ptr(), out_p.data_ptr() if prob is not None else None, status.data_ptr())
    assert lib.gapro_spp_vote(*args, nbytes - 1, *tail) == -7  # GAPRO_ERR_WORKSPACE, before anything is launched
    ctx.check(lib.gapro_spp_vote(*args, nbytes, *tail))
    torch.cuda.synchronize()
    return int(status.item()), _np(out_l), _np(out_p)


def test_refusals_are_statuses():
    from gapro_amd._lib import GaproError
    from gapro_amd.gen_ps_utils import spp_align_label, spp_major_voting

    rng = np.random.default_rng(2)
    n, S, Cn = 200, 9, 4
    ids = np.r_[np.arange(S), rng.integers(0, S, n - S)]
    label = rng.integers(0, Cn, n)
    prob = rng.random(n).astype(np.float32)
    occ = (rng.random((n, Cn - 1)) < 0.9).astype(np.uint8)
    st, lab, p = _raw(1, ids, label, prob, occ, S, Cn)
    w_lab, w_p = vote_ref.spp_major_voting(ids, label, prob, occ, Cn)
    assert st == 0 and np.array_equal(lab[:n], w_lab) and np.array_equal(_bits(p[:n]), _bits(w_p))
    assert (lab[n:] == -7).all() and (p[n:] == -7).all()

    def refused(mode, label, prob, want, ids=ids):
        st, lab, p = _raw(mode, ids, label, prob, occ if mode == 1 else None, S, Cn)
        assert st == want and (lab == -7).all() and (p == -7).all()  # nothing was written

    bad = label.copy()
    bad[77] = Cn
    for mode in (0, 1):
        refused(mode, bad, prob, -1)
        refused(mode, bad.astype(np.int32), prob, -1)
    neg = label.copy()
    neg[0] = -1
    refused(0, neg, None, -1)
    wide = label.copy()
    wide[3] = 2 ** 32 + 1  # not a class, whatever its low 32 bits say
    refused(0, wide, None, -1)
    nan, inf, big = prob.copy(), prob.copy(), prob.copy()
    nan[199], inf[5], big[64] = np.nan, np.inf, 1.5
    for mode in (0, 1):
        refused(mode, label, nan, -4)
        refused(mode, label, inf, -4)
    refused(1, label, big, -1)
    refused(1, bad, nan, -4)  # GAPRO_ERR_NOT_FINITE wins
    far = ids.copy()
    far[10] = S
    refused(0, label, None, -1, ids=far)
    # spp_align_label takes any finite prob_label (the reference asserts [0, 1] in spp_major_voting alone)
    st, lab, p = _raw(0, ids, label, big, None, S, Cn)
    assert st == 0 and np.array_equal(_bits(p[:n]), _bits(vote_ref.spp_align_label(ids, label, Cn, None, big)[1]))
    # the Python functions raise
    for call in (lambda: spp_major_voting(ids, bad, prob, occ, Cn), lambda: spp_align_label(ids, label, Cn, None, nan),
                 lambda: spp_major_voting(ids, label, big, occ, Cn)):
        with pytest.raises(GaproError):
            call()
    with pytest.raises(ValueError):
        spp_align_label(ids, label[:-1])
    with pytest.raises(ValueError):
        spp_major_voting(ids, label, prob, occ[:, :2], Cn)
    with pytest.raises(ValueError):
        spp_align_label(ids, label, Cn, np.ones((Cn - 1, S + 1), bool))
