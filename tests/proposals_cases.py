"""Inputs for the predicted-instance chain (get_instance, mask_nms, rle_encode_gpu_batch): random scenes and the edge
cases, shared by tests/test_proposals_cpu.py, tests/test_proposals_gpu.py, the golden generator and the benchmark.  NumPy
only.  A case is ``(name, kwargs of proposals_ref.get_instance_ref)``; every case of ``cases()`` is tiny (Q <= 40,
V, N <= 1100).

``scale_cases()`` holds the cases at the sizes where the loops of csrc/proposals.hip take their second trip (DESIGN.md
4.8 lists loop -> case).  Each has one deliberate large dimension and keeps the others small; none is random where a
size or a score matters.  Every one passes ``_guard``: on the restatement's numbers any two scores, and for matrix NMS
any two updated scores, are bit-identical or more than 4 float32 ulp apart, and with ``topk = -1`` no updated score lies
within 4 ulp of ``final_score_thresh``: a last-place difference of an ``exp`` cannot change an order or a cut.
"""
import functools

import numpy as np

# The constants of csrc/proposals.hip and of csrc/select_runs.h (kThreads, kMinChunk, kMaxChunks, kMaxTopk, kMaxScores:
# shared with csrc/spf_predict.hip) that no public header exposes, mirrored: a change there is a change here.
PACK_WORDS = 32                     # kPackWords: the words (of 64 voxels) of a wave's run of `pack`
PACK_PASS_WAVES = 2048 * 4          # GAPRO_PROPOSALS_GRID_CAP * (kThreads / 64) waves: tasks of one pass of `pack`
INTER_PASS_WORDS = 64               # `inter`: a word a lane, 64 words a trip
GRID_PASS_ITEMS = 2048 * 256        # GAPRO_PROPOSALS_GRID_CAP * kThreads: one pass of `score` (queries), `points`
TALLY_PASS_POINTS = 256 * 256       # kTallyGridX * kThreads: points of a row in one pass of `tally`
SCAN_CHUNKS = 64                    # `chunks`: a chunk a lane, 64 chunks a step of the scan
MIN_CHUNK, MAX_CHUNKS = 1024, 1024  # kMinChunk, kMaxChunks
NMS_PASS = 256                      # kThreads: the places behind a pivot in one trip of the standard NMS loop
MAX_TOPK, MAX_SEM = 1024, 8         # GAPRO_PROPOSALS_MAX_PRE_TOPK (kMaxTopk), GAPRO_PROPOSALS_MAX_SEM2INS (kMaxSem)
FINISH_PASS_ROWS = 256 * 4          # kThreads * (kRowsPer - 1): `finish` needs its fifth row a thread beyond this
MAX_SCORES = 1 << 20                # kMaxScores: Q * C at most


def chunking(N):
    """(nchunks, chunk_len) of N points: ``chunking`` of csrc/select_runs.h, which both chains' make_dims call."""
    nchunks = min((N + 1 + MIN_CHUNK - 1) // MIN_CHUNK, MAX_CHUNKS)
    return nchunks, (N + 1 + nchunks - 1) // nchunks


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


def many_rows_case(Q, seed=None):
    """Q * 4 candidates that all survive into stage 5 (a threshold of 1 suppresses nothing)."""
    rng = np.random.default_rng(Q if seed is None else seed)
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


# ---- the cases at workload size --------------------------------------------------------------------------------------
def explicit_cols(colbits, scores, voxel_spps, **params):
    """``explicit`` in the ``voxel_spps`` form: chosen bits of the mask columns bool[Q, S_v]; voxel v reads column
    ``voxel_spps[v]``.  Every voxel has one point and every point is its own superpoint unless given."""
    voxel_spps = np.asarray(voxel_spps, np.int64)
    params.setdefault("v2p", np.arange(len(voxel_spps)))
    c = explicit(colbits, scores, **params)
    c.update(voxel_spps=voxel_spps, semantic_preds=np.zeros(len(voxel_spps), np.int64))
    return c


def _two_columns(Q):
    """Column bits of Q queries over two mask columns: the second, the first, both, in turn."""
    q = np.arange(Q)
    return np.stack([q % 3 != 0, q % 3 != 1], axis=1)


def pack_run_case(V):
    """Six rows of V voxels; voxel V - 1 is set in four of them.  At V = 2049 it is the only voxel of the second run of
    `pack`, at V = 4097 the only bit of the 65th word.  Row 5 has exactly ``npoint_thresh`` voxels with it."""
    rng = np.random.default_rng(V)
    bits = rng.random((6, V)) < np.array([0.45, 0.45, 0.4, 0.4, 0.4, 0.3])[:, None]
    bits[:, V - 1] = [1, 1, 0, 1, 0, 1]
    v2p = np.r_[np.arange(V), rng.integers(0, V, 7)]
    return explicit(bits, _falling(6), v2p=v2p, spps=v2p // 4, npoint_thresh=int(bits[5].sum()), type_nms="matrix",
                    topk=-1)


def pack_grid_case(Q):
    """Q rows of 70 voxels, one (row, run) task each; the 16 best scores are the last rows: at Q = 8200 eight of them
    are tasks of the second pass of `pack`."""
    return explicit_cols(_two_columns(Q), _falling(Q)[::-1], np.arange(70) >= 33, pre_topk=16)


def tie_block_case(n, lo, hi, n_higher, pre_topk):
    """n scores, C = 1: the scores [lo, hi) are bit-identical (identical class rows); the last ``n_higher`` are above
    them and every other one below, before and behind the block.  ``pre_topk`` cuts inside the block: the candidates are
    the ``n_higher`` and the lowest indices of the block."""
    s = np.linspace(0.2, 0.4, n)
    s[lo:hi] = 0.5
    s[n - n_higher:] = np.linspace(0.6, 0.55, n_higher)
    assert hi <= n - n_higher and n_higher < pre_topk < n_higher + hi - lo
    return explicit_cols(_two_columns(n), s.reshape(n, 1), np.arange(70) >= 33, pre_topk=pre_topk)


def score_count_case(Q, C):
    """Q * C distinct scores in no order, pre_topk = 1024."""
    rng = np.random.default_rng(Q * C)
    s = _falling(Q, C).reshape(-1)[rng.permutation(Q * C)].reshape(Q, C)
    return explicit(rng.random((Q, 70)) < 0.5, s, pre_topk=MAX_TOPK)


def score_cap_case():
    """Q = 2^20, the most the select takes, C = 1.  Seven low levels in turn (ties by the hundred thousand), a block of
    600 bit-identical scores around index 0xC0000 and the 200 best at the very end; pre_topk = 512 cuts 312 into the
    block, 12 beyond the index whose third byte changes.  Half the queries are beyond one pass of `score`."""
    n = MAX_SCORES
    s = np.linspace(0.2, 0.3, 7)[np.arange(n) % 7]
    s[0xC0000 - 300:0xC0000 + 300] = 0.5
    s[n - 200:] = np.linspace(0.55, 0.6, 200)
    return explicit_cols(_two_columns(n), s.reshape(n, 1), np.arange(8) % 2, pre_topk=512)


def full_sorts_case(kind, seed=None):
    """P = 1024 candidates (256 queries, 4 classes) that all pass ``npoint_thresh``: every thread of `filter` and `nms`
    owns four, the LDS sorts have no padding.  With the eight sem2ins classes R = 1032: the fifth row of a thread of
    `finish`."""
    c = many_rows_case(256, seed)
    if kind == "matrix_none":
        c.update(type_nms="matrix", topk=-1)
    elif kind == "matrix_topk":
        c.update(type_nms="matrix", topk=MAX_TOPK)
    if kind != "matrix_none":
        c.update(sem2ins_classes=tuple(range(MAX_SEM)), semantic_preds=np.arange(300) // 10 % MAX_SEM)
    return c


def nms_far_case(distance):
    """1024 candidates of one class, standard NMS at 0.5.  A mask is three of thirty runs of ten voxels (the superpoints
    of 400 points), a different three for every candidate: two masks share at most two runs, an IoU of 0.5 at most, and
    nothing is suppressed -- but candidate q + distance has the mask of candidate q for q < 200.  At distance 256 the
    victim is the last place of the pivot's first trip, at 257 the first of its second."""
    import itertools

    rng = np.random.default_rng(257)
    triples = np.array(list(itertools.combinations(range(30), 3)))[rng.permutation(4060)[:MAX_TOPK]]
    on = np.zeros((MAX_TOPK, 30), bool)
    on[np.arange(MAX_TOPK)[:, None], triples] = True
    on[distance:distance + 200] = on[:200]
    v2p = np.sort(rng.integers(0, 300, 400))
    return explicit(np.repeat(on, 10, axis=1), _falling(MAX_TOPK), pre_topk=MAX_TOPK, npoint_thresh=20, v2p=v2p,
                    spps=v2p // 10, nms_threshold=0.5)


def boundary_case(N):
    """N points, four rows, 68 voxels.  The points come in segments that start and end at b - 1, b and b + 1 for every
    chunk boundary b of ``chunking(N)`` (so for every 64-chunk group) and for 64 .. 512; a segment's even and odd points
    are two superpoints.  A point's voxel is 4 * superpoint + its kind: p % 3 == 0 (E) or not (F) among the first
    TALLY_PASS_POINTS points, then 300 000 points L1, then L2.  Row 0 has every voxel: all ones.  Row 1 has the voxels of
    the even points: it alternates every point.  Row 3 has whole segments.  Row 2 has E, L1 and L2 of some segments (a
    third of the early points, so the majority comes from the points of the later passes of `tally`), only L1 of others
    (fewer than half their points, and more than half of those among the first GRID_PASS_ITEMS: n(s) needs the later
    pass of `points`), and everything of others.  Beyond TALLY_PASS_POINTS points a superpoint of three points has its
    second set point there."""
    S0, T = 8, TALLY_PASS_POINTS
    nchunks, chunk = chunking(N)
    cuts = {1, N - 1}
    for b in [64, 128, 256, 512] + [chunk * i for i in range(1, nchunks + 1)]:
        cuts.update((b - 1, b, b + 1))
    cuts = np.array(sorted(p for p in cuts if 0 < p < N))
    p = np.arange(N)
    seg = np.searchsorted(cuts, p, side="right")
    own = (5 * seg + 3) % S0
    spps = 2 * own + (p & 1)
    kind = np.where(p < T, np.where(p % 3 == 0, 0, 1), np.where(p < T + 300000, 2, 3))
    v2p = 4 * spps + kind
    if N > T:
        three = np.array([10, 20, T + 40 if N > T + 40 else T])
        spps[three], v2p[three] = 2 * S0, [64, 65, 66]
    voxel_own, voxel_kind, voxel_odd = np.arange(68) // 8, np.arange(68) % 4, np.arange(68) // 4 % 2
    extra = np.arange(68) >= 64
    bits = np.stack([
        np.ones(68, bool),
        np.where(extra, True, voxel_odd == 0),
        np.where(extra, voxel_kind != 1, (np.isin(voxel_own, (1, 4)) & (voxel_kind != 1))
                 | ((voxel_own == 2) & (voxel_kind == 2)) | (voxel_own == 6)),
        np.where(extra, False, voxel_own % 2 == 1)])  # every second segment: a transition at every cut
    return explicit(bits, _falling(4), v2p=v2p, spps=spps, n_spps=2 * S0 + 1)


def nms_1024_inputs(seed=4100):
    """For mask_nms: 1024 masks of 4097 voxels (65 words), 64 prototypes with a few per cent of their bits flipped; a
    prototype's sixteen masks have one class, so a pivot's victims sit up to 960 rows behind it before the sort by the
    shuffled, distinct scores.  Returns (bits, classes, scores, boxes)."""
    rng = np.random.default_rng(seed)
    proto = rng.random((64, 4097)) < 0.3
    i = np.arange(MAX_TOPK)
    bits = proto[i % 64] ^ (rng.random((MAX_TOPK, 4097)) < 0.03)
    bits[:, 4096] = i % 3 != 0
    score = np.linspace(0.9, 0.15, MAX_TOPK)[rng.permutation(MAX_TOPK)].astype(np.float32)
    return bits, (i % 4).astype(np.int64), score, rng.uniform(-4, 4, (MAX_TOPK, 6)).astype(np.float32)


def _ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))  # the scores are >= +0.0


def guard_values(name, values, thresh=None):
    """Any two of the values are bit-identical or more than 4 float32 ulp apart; none is within 4 ulp of ``thresh``."""
    v = np.sort(np.asarray(values, np.float32))
    gap = _ulps(v[1:], v[:-1])
    assert ((gap == 0) | (gap > 4)).all(), (name, "values within 4 ulp of each other")
    if thresh is not None:
        gap = _ulps(v, np.full(len(v), thresh, np.float32))
        assert ((gap == 0) | (gap > 4)).all(), (name, "a value within 4 ulp of the threshold")


def _guard(name, c):
    """The condition of the module's docstring, on the restatement's numbers."""
    import proposals_ref as ref

    score = ref.scores_ref(c["cls_logits"], c["conf_logits"]).reshape(-1)
    guard_values(name, score)
    if c["type_nms"] == "matrix":
        C = c["instance_classes"]
        cand = ref.order_ref(score, min(c.get("pre_topk", 300), len(score)))
        bits = ref.bits_ref(c["mask_logits"], c["logit_thresh"], c.get("voxel_spps"))[cand // C]
        keep = bits.sum(axis=1) >= c["npoint_thresh"]
        _, new = ref.nms_ref(bits[keep], (cand % C)[keep], score[cand][keep], "matrix", int(keep.sum()))
        guard_values(name, new, 0.1 if c["topk"] == -1 else None)
    return c


_SCALE = {
    "pack_v2048": lambda: pack_run_case(2048),  # control: one run of words
    "pack_v2049": lambda: pack_run_case(2049),
    "pack_v4097": lambda: pack_run_case(4097),
    "pack_grid_q8192": lambda: pack_grid_case(8192),  # control: one pass of tasks
    "pack_grid_q8200": lambda: pack_grid_case(8200),
    "tie_across_65536": lambda: tie_block_case(66000, 65300, 65800, 100, 400),
    "tie_across_256": lambda: tie_block_case(2000, 100, 1300, 100, MAX_TOPK),
    "scores_1024": lambda: score_count_case(256, 4),
    "scores_1025": lambda: score_count_case(205, 5),
    "scores_at_the_cap": score_cap_case,
    "p1024_standard_all": lambda: full_sorts_case("standard_all"),
    "p1024_matrix_none": lambda: full_sorts_case("matrix_none"),
    "p1024_matrix_topk": lambda: full_sorts_case("matrix_topk"),
    "nms_victims_256_behind": lambda: nms_far_case(256),  # control: the last place of the first trip
    "nms_victims_257_behind": lambda: nms_far_case(257),
    "points_65535": lambda: boundary_case(65535),  # control: 64 chunks, one pass of `tally`
    "points_65536": lambda: boundary_case(65536),  # 65 chunks; control: one pass of `tally`
    "points_65537": lambda: boundary_case(65537),
    "points_1048575": lambda: boundary_case(1048575),  # 1024 chunks of 1024
    "points_1048576": lambda: boundary_case(1048576),  # chunks of 1025
    "points_1300001": lambda: boundary_case(1300001),  # chunks of 1270
}
SCALE_NAMES = tuple(_SCALE)
RLE_POINTS = (65535, 65536, 1048575, 1048576, 1300001)


@functools.lru_cache(maxsize=None)
def scale_case(name):
    """The case of that name, built once and guarded."""
    return _guard(name, _SCALE[name]())


@functools.lru_cache(maxsize=None)
def scale_reference(name):
    """``get_instance_ref`` of the case, computed once; shared and not to be changed."""
    import proposals_ref as ref

    return ref.get_instance_ref(**scale_case(name))


def scale_cases():
    for name in SCALE_NAMES:
        yield name, scale_case(name)
