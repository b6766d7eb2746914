"""Inputs for the predicted-instance chain (get_instance, mask_nms, rle_encode_gpu_batch): random scenes and the edge
cases, shared by tests/test_proposals_cpu.py, tests/test_proposals_gpu.py, the golden generator and the benchmark.  NumPy
only.  A case is ``(name, kwargs of proposals_ref.get_instance_ref)``; every case is tiny (Q <= 40, V, N <= 1100).
"""
import numpy as np

KEYS = ("cls_logits", "mask_logits", "conf_logits", "box_preds", "v2p_map", "semantic_preds", "spps")


def make_scene(seed, Q=40, C=18, V=1000, N=1100, S=90, n_inst=9, n_sem_classes=4, spp_form=True):
    """A scene like the consumer's: superpoints are runs of voxels, instances are sets of superpoints, a query aims at
    one instance with noisy logits, a few per cent of the points sit in a neighbouring superpoint (the quantization error
    the refinement is there for), and superpoint ids are in no order along the points."""
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.permutation(np.arange(1, V))[:S - 1])
    voxel_spps = np.repeat(np.arange(S), np.diff(np.r_[0, cuts, V])).astype(np.int64)
    owner = rng.integers(0, n_inst, S)
    target = rng.integers(0, n_inst, Q)
    logits = np.where(owner[None, :] == target[:, None], 2.0, -2.0) + rng.normal(0, 1.5, (Q, S))
    logits[rng.random(Q) < 0.15] -= 3.0                        # queries that found nothing
    v2p = np.sort(rng.choice(np.nonzero(rng.random(V) < 0.97)[0], N)).astype(np.int64)  # some voxels have no point
    point_spp = voxel_spps[v2p].copy()
    noise = rng.random(N) < 0.06
    point_spp[noise] = np.clip(point_spp[noise] + rng.choice([-1, 1], int(noise.sum())), 0, S - 1)
    perm = rng.permutation(S)
    cls = rng.normal(0, 1.0, (Q, C + 1))
    cls[np.arange(Q), rng.integers(0, C, Q)] += rng.uniform(1, 5, Q)
    out = dict(cls_logits=cls.astype(np.float32), mask_logits=logits.astype(np.float32),
               conf_logits=rng.uniform(-0.1, 1.2, Q).astype(np.float32),
               box_preds=rng.uniform(-4, 4, (Q, 6)).astype(np.float32), v2p_map=v2p,
               semantic_preds=rng.integers(0, n_sem_classes, V).astype(np.int64), spps=perm[point_spp].astype(np.int64),
               voxel_spps=voxel_spps, n_spps=S, instance_classes=C)
    if not spp_form:
        out["mask_logits"] = np.ascontiguousarray(out["mask_logits"][:, voxel_spps])
        out["voxel_spps"] = None
    return out


def explicit(bits, scores, *, v2p=None, spps=None, n_spps=None, **params):
    """Inputs with chosen voxel bits bool[Q, V] and chosen scores [Q, C] (each row's squares sum below 1): the logits of
    a set bit are +1, of a clear one -1; conf is 1 and the class logits are the logs of the squared scores."""
    bits, scores = np.asarray(bits, bool), np.asarray(scores, np.float64)
    Q, V = bits.shape
    p = scores ** 2
    rest = 1.0 - p.sum(axis=1, keepdims=True)
    assert (rest > 0).all() and (p > 0).all()
    v2p = np.arange(V) if v2p is None else np.asarray(v2p)
    spps = np.arange(len(v2p)) if spps is None else np.asarray(spps)
    out = dict(cls_logits=np.log(np.concatenate([p, rest], axis=1)).astype(np.float32),
               mask_logits=np.where(bits, 1.0, -1.0).astype(np.float32), conf_logits=np.ones(Q, np.float32),
               box_preds=np.arange(Q * 6, dtype=np.float32).reshape(Q, 6), v2p_map=v2p.astype(np.int64),
               semantic_preds=np.zeros(V, np.int64), spps=spps.astype(np.int64),
               n_spps=int(spps.max()) + 1 if n_spps is None else n_spps, instance_classes=scores.shape[1],
               logit_thresh=0.0, npoint_thresh=1, type_nms="standard", topk=100, nms_threshold=1.0)
    out.update(params)
    return out


def _falling(Q, C=1, hi=0.6, lo=0.2):
    """Distinct scores, falling with the flat index."""
    return np.linspace(hi, lo, Q * C).reshape(Q, C) / np.sqrt(C)


def _rows(V, *ranges):
    bits = np.zeros((len(ranges), V), bool)
    for q, r in enumerate(ranges):
        for lo, hi in (r if isinstance(r, list) else [r]):
            bits[q, lo:hi] = True
    return bits


def tail_case(V):
    """Rows whose successor in memory starts with set values: a word filled past V would pick them up."""
    rng = np.random.default_rng(V)
    bits = rng.random((6, V)) < 0.4
    bits[:, :60] |= rng.random((6, 60)) < 0.8
    bits[:, V - 3:] = False
    return explicit(bits, _falling(6, 2, 0.6, 0.3), v2p=np.r_[np.arange(V), rng.integers(0, V, 7)], npoint_thresh=5,
                    spps=rng.integers(0, 9, V + 7), n_spps=9, type_nms="matrix", voxel_spps=None)


def tie_case(pre_topk):
    """q2 and q3 have the same class row and conf, so bit-identical scores; their masks differ and overlap."""
    s = _falling(6)
    s[3] = s[2]
    bits = _rows(40, (0, 8), (8, 16), (16, 30), (20, 36), (30, 40), (36, 40))
    return explicit(bits, s, pre_topk=pre_topk, type_nms="matrix", topk=-1)


def npoint_case(which):
    bits = _rows(64, (0, 9), (10, 20), (20, 29), (30, 39))
    if which == "all_below":
        return explicit(bits, _falling(4), npoint_thresh=11)
    return explicit(bits, _falling(4), npoint_thresh=10)  # q1 sits at the threshold, the others one below


def class_case(same_query):
    if same_query:  # one query, high under both classes: IoU 1, two classes
        bits = _rows(32, (0, 12), (20, 30))
        return explicit(bits, [[0.6, 0.5], [0.3, 0.2]], nms_threshold=0.2)
    bits = _rows(32, (0, 12), (0, 12), (20, 30))  # two queries, one mask, one class
    return explicit(bits, _falling(3), nms_threshold=0.2)


def iou_quarter_case():
    """|A| = |B| = 5, |A & B| = 2: iou = 2 / 8 = 0.25 exactly, not above a threshold of 0.25."""
    return explicit(_rows(16, (0, 5), (3, 8)), _falling(2), nms_threshold=0.25)


def many_rows_case(Q):
    """Q * 4 candidates that all survive into stage 5 (a threshold of 1 suppresses nothing)."""
    rng = np.random.default_rng(Q)
    bits = np.repeat(rng.random((Q, 30)) < 0.4, 10, axis=1) ^ (rng.random((Q, 300)) < 0.1)
    v2p = np.sort(rng.integers(0, 300, 400))
    return explicit(bits, _falling(Q, 4, 0.9, 0.1), pre_topk=Q * 4, npoint_thresh=20, v2p=v2p, spps=v2p // 10)


def spp_case():
    """Superpoint 0: 2 c == n (4 points, 2 set); 1: c == 0; 2: all set; 3: no point carries it; 4: 1 of 3; 5: 2 of 3.
    The ids are unsorted along the points and voxels 10 and 11 have no point."""
    bits = _rows(12, [(0, 2), (4, 5), (6, 8), (10, 12)], (4, 10))
    v2p = [0, 2, 6, 8, 9, 1, 3, 4, 5, 7, 5, 6, 9]
    spps = [0, 0, 2, 1, 1, 0, 0, 4, 4, 5, 4, 5, 5]
    return explicit(bits, _falling(2), v2p=v2p, spps=spps, n_spps=7)


def lose_gain_case():
    """npoint_thresh = 6.  q0 has 6 voxels but its points are minorities of their superpoints: refined to 0 points.
    q1 has 6 voxels of which 3 carry points, 5 in all, below the threshold; they are the majority (or exactly half) of
    their superpoints: refined to 8 points."""
    bits = _rows(40, (0, 6), [(10, 13), (30, 33)])
    v2p = np.r_[np.arange(0, 6), np.repeat(20, 18), 10, 10, 11, 11, 12, 21, 22, 23]
    spps = np.r_[np.arange(0, 6), np.repeat(np.arange(0, 6), 3), 6, 6, 7, 7, 8, 6, 7, 8]
    return explicit(bits, _falling(2), v2p=v2p, spps=spps, npoint_thresh=6)


def runs_case():
    """Masks that start at point 0, end at N - 1, are all ones, alternate every point, and cross every 64-point
    boundary; every point is its own superpoint, so the masks are the voxel bits."""
    N = 200
    alt = np.zeros(N, bool)
    alt[::2] = True
    alt_odd = ~alt
    bits = np.stack([_rows(N, (0, 5))[0], _rows(N, (190, N))[0], np.ones(N, bool), alt, alt_odd,
                     _rows(N, [(60, 70), (120, 130), (191, 193)])[0], _rows(N, [(63, 65), (127, 129), (0, 1), (199, 200)])[0]])
    return explicit(bits, _falling(7, 1, 0.35, 0.1))


def sem2ins_case(ordinary):
    c = make_scene(77, Q=12, C=3, V=260, N=300, S=24, n_inst=4, n_sem_classes=3)
    c.update(sem2ins_classes=(0, 2), label_shift=3, npoint_thresh=20 if ordinary else 100000, type_nms="matrix",
             topk=-1)
    return c


def cases():
    for V in (63, 64, 65, 129):
        yield "tail_v%d" % V, tail_case(V)
    for name, pre in (("qc_below", 200), ("qc_equal", 144), ("qc_above", 100)):
        c = make_scene(31, Q=8, C=18, V=300, N=350, S=30, n_inst=4)
        c.update(pre_topk=pre, npoint_thresh=15, type_nms="matrix", topk=100)
        yield name, c
    yield "tie_across_cut", tie_case(3)
    yield "tie_inside", tie_case(6)
    yield "all_below_npoint", npoint_case("all_below")
    yield "npoint_at_and_below", npoint_case("at")
    yield "same_query_two_classes", class_case(True)
    yield "identical_masks_one_class", class_case(False)
    d = class_case(False)
    d.update(type_nms="matrix", topk=-1)
    yield "identical_masks_matrix", d
    yield "iou_equals_threshold", iou_quarter_case()
    yield "rows_68", many_rows_case(17)
    yield "rows_132", many_rows_case(33)
    for name, topk in (("topk_beyond", 100), ("topk_none", -1), ("topk_cuts", 5)):
        c = make_scene(32, Q=20, C=6, V=500, N=600, S=40, n_inst=5)
        c.update(npoint_thresh=25, type_nms="matrix", topk=topk)
        yield name, c
    c = make_scene(33, Q=20, C=6, V=500, N=600, S=40, n_inst=5)
    c.update(npoint_thresh=25, type_nms="standard", nms_threshold=0.2)
    yield "standard_scene", c
    yield "spp_rules", spp_case()
    yield "lose_and_gain", lose_gain_case()
    yield "run_shapes", runs_case()
    yield "sem2ins_with_rows", sem2ins_case(True)
    yield "sem2ins_alone", sem2ins_case(False)


def refusals():
    """(name, kwargs, status, flags): every refusal of the data."""
    from proposals_ref import (ERR_BAD_ARG, ERR_NOT_FINITE, ERR_SPP_RANGE, FLAG_MASK, FLAG_SCORE, FLAG_SPP, FLAG_V2P,
                               FLAG_VOXEL_SPP)

    def base():
        c = make_scene(34, Q=6, C=3, V=130, N=150, S=12, n_inst=3)
        c.update(npoint_thresh=5, pre_topk=4)
        return c

    for name, key, at, value in (("cls_nan", "cls_logits", (2, 1), np.nan), ("cls_inf", "cls_logits", (0, 3), np.inf),
                                 ("conf_inf", "conf_logits", (5,), -np.inf)):
        c = base()
        c[key][at] = value
        yield name, c, ERR_NOT_FINITE, FLAG_SCORE
    c = base()
    c["v2p_map"][7] = 130
    yield "v2p_high", c, ERR_BAD_ARG, FLAG_V2P
    c = base()
    c["v2p_map"][0] = -1
    yield "v2p_negative", c, ERR_BAD_ARG, FLAG_V2P
    c = base()
    c["voxel_spps"][129] = 12
    yield "voxel_spps_high", c, ERR_BAD_ARG, FLAG_VOXEL_SPP
    c = base()
    c["spps"][149] = 12
    yield "spps_high", c, ERR_SPP_RANGE, FLAG_SPP
    c = base()
    c["spps"][3] = -100
    yield "spps_ignore_label", c, ERR_SPP_RANGE, FLAG_SPP
    c = base()
    c["spps"][3] = -1
    c["v2p_map"][9] = 1 << 20
    c["conf_logits"][1] = np.nan
    yield "precedence", c, ERR_NOT_FINITE, FLAG_SCORE | FLAG_V2P | FLAG_SPP


def mask_refusal():
    """A non-finite mask value in the row of a candidate is refused; in a row no candidate reads it is not.  Returns
    (kwargs refused, kwargs accepted)."""
    from proposals_ref import scores_ref, order_ref
    c = make_scene(34, Q=6, C=3, V=130, N=150, S=12, n_inst=3)
    c.update(npoint_thresh=5, pre_topk=4)
    cand_q = order_ref(scores_ref(c["cls_logits"], c["conf_logits"]).reshape(-1), 4) // 3
    unread = [q for q in range(6) if q not in set(cand_q.tolist())]
    assert unread
    bad, fine = dict(c), dict(c)
    bad["mask_logits"] = c["mask_logits"].copy()
    bad["mask_logits"][cand_q[-1], 5] = np.nan
    fine["mask_logits"] = c["mask_logits"].copy()
    fine["mask_logits"][unread[0], 5] = np.inf
    return bad, fine
