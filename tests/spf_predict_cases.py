"""Scenes and edge cases of SPFormer's predicted-instance chain (include/gapro_hip.h, "SPFormer's predicted instances"),
at the smallest shapes that can still go wrong.  A case is the keyword dict of ``spf_predict_ref.predict_ref``.

Every case passes ``_checked``: on the restatement's numbers any two class scores, and any two conf values of the
candidates, are bit-identical or more than 4 float32 ulp apart, so a tie occurs only where it is built from identical
rows and a last-place difference of an ``exp`` cannot change an order or a threshold test.
"""
import numpy as np

import spf_predict_ref as ref

INPUTS = ref.INPUTS


def make_scene(seed, Q=40, C=18, S=130, N=5000, n_inst=12, used=None, max_run=40, negative=0, amp=4.0, grid=False):
    """A scene of ``n_inst`` blobs of superpoints; every query looks at one of them.  ``used``: the superpoint ids that
    have points (the rest stay empty); the ids come in runs of random length, unsorted.  ``grid``: coordinates on
    multiples of 1/32 and mask logits on multiples of 1/8, so that a fixture compresses."""
    rng = np.random.default_rng(seed)
    used = S if used is None else used
    ids = rng.permutation(S)[:used]
    spp, at = np.zeros(N, np.int64), 0
    while at < N:
        n = int(rng.integers(1, max_run + 1))
        spp[at:at + n] = ids[rng.integers(0, used)]
        at += n
    coords = rng.uniform(-3.0, 3.0, (N, 3)).astype(np.float32)
    if grid:
        coords = (np.round(coords * 32) / 32).astype(np.float32)
    coords[rng.integers(0, N, max(N // 50, 1)), rng.integers(0, 3, max(N // 50, 1))] = -0.0
    inst_of = rng.integers(0, n_inst, S)
    inst_cls = rng.integers(0, C, n_inst)
    labels = rng.normal(0.0, 1.5, (Q, C + 1)).astype(np.float32)
    masks = np.zeros((Q, S), np.float32)
    for q in range(Q):
        i = int(rng.integers(0, n_inst))
        labels[q, inst_cls[i]] += np.float32(3.0)
        x = np.where(inst_of == i, amp, -amp) + rng.normal(0.0, 2.0, S)
        x = np.round(x * 8) / 8 if grid else x
        x = np.where(np.abs(x) < 1e-3, 0.5, x)  # nothing near zero but what a case puts there
        masks[q] = x.astype(np.float32)
    scores = rng.uniform(0.2, 1.0, Q).astype(np.float32)
    if negative:
        scores[rng.permutation(Q)[:negative]] *= np.float32(-1.0)
    return dict(labels=labels, pred_scores=scores, masks=masks, superpoints=spp, coords_float=coords, num_class=C)


def _ulps(a, b):
    a, b = np.asarray(a, np.float32) + np.float32(0), np.asarray(b, np.float32) + np.float32(0)

    def image(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)

    return np.abs(image(a) - image(b))


def _checked(name, c):
    s = np.sort(ref.class_scores64(c["labels"], c["pred_scores"]).reshape(-1).astype(np.float32))
    gap = _ulps(s[1:], s[:-1])
    assert ((gap == 0) | (gap > 4)).all(), (name, "class scores within 4 ulp")
    out = ref.predict_ref(**dict(c, score_thr=-3.0e38, npoint_thr=0))
    if out["status"] == ref.OK and len(out["conf"]) > 1:
        v = np.sort(out["conf"])
        gap = _ulps(v[1:], v[:-1])
        assert ((gap == 0) | (gap > 4)).all(), (name, "conf within 4 ulp")
        thr = np.full(len(v), c.get("score_thr", 0.0), np.float32)
        gap = _ulps(v, thr)
        assert ((gap == 0) | (gap > 4)).all(), (name, "conf within 4 ulp of score_thr")
    return name, c


def _boundary_scene(seed, N, Q=6, C=3, S=8):
    """Superpoint segments that start and end at every 64-point and chunk boundary of N points, and next to them."""
    nchunks = min((N + 1 + 1023) // 1024, 1024)
    chunk = (N + 1 + nchunks - 1) // nchunks
    cuts = {0, 1, N - 1}
    for b in [64, 128, 256, 512] + [chunk * i for i in range(1, nchunks + 1)]:
        cuts.update((b - 1, b, b + 1))
    cuts = sorted(p for p in cuts if 0 < p < N)
    c = make_scene(seed, Q=Q, C=C, S=S, N=N, n_inst=3)
    spp, seg = np.zeros(N, np.int64), 0
    for i, lo in enumerate([0] + cuts):
        hi = (cuts + [N])[i]
        spp[lo:hi] = (5 * seg + 3) % S
        seg += 1
    c["superpoints"] = spp
    for q in range(Q):  # every row a different subset of the superpoints: bit j of a counter
        pattern = np.array([((q + 1) * 37 >> (j % 6)) & 1 for j in range(S)], bool)
        c["masks"][q] = np.where(pattern, np.abs(c["masks"][q]) + 0.5, -np.abs(c["masks"][q]) - 0.5).astype(np.float32)
    c["masks"][0] = np.abs(c["masks"][0]) + 0.5  # all points: one run [1, N]
    return dict(c, topk_insts=100, score_thr=0.0, npoint_thr=0)


TIE_BLOCK = (66000, 65300, 65800, 100, 400)  # scores, the block [lo, hi), the scores above it, topk_insts


def _tie_block_scene():
    """66 000 queries of one class whose score is softmax(labels)[0]: the scores [65300, 65800) are bit-identical
    (identical rows), the last 100 are above them and every other one below, before and behind the block.  ``topk_insts``
    = 400 cuts 300 into the block, beyond flat index 65 536: the select decides among equal scores by the third byte of
    the index.  Even and odd queries have different masks of one mask score, so equal scores give equal conf."""
    n, lo, hi, higher, topk = TIE_BLOCK
    c = make_scene(293, Q=2, C=1, S=8, N=300, n_inst=2)
    p = np.linspace(0.2, 0.4, n)
    p[lo:hi] = 0.5
    p[n - higher:] = np.linspace(0.6, 0.55, higher)
    labels = np.log(np.stack([p, 1.0 - p], axis=1)).astype(np.float32)
    masks = np.where((np.arange(8)[None, :] // 3) == (np.arange(n)[:, None] % 2), 2.0, -2.0).astype(np.float32)
    return dict(c, labels=labels, pred_scores=np.ones(n, np.float32), masks=masks, topk_insts=topk, score_thr=0.0,
                npoint_thr=0)


def cases():
    """(name, case) pairs."""
    out = []
    for S in (1, 63, 64, 65, 129):  # the last word of a row; the values behind a row's end are set
        c = make_scene(100 + S, Q=6, C=3, S=S, N=300, n_inst=2, amp=1.0)
        c["masks"][:, 0] = np.float32(2.5)  # what follows every row in memory is positive
        c["masks"][:, -1] = np.float32(-1.5) if S > 1 else np.float32(2.5)
        out.append(_checked("spp_%d" % S, dict(c, topk_insts=100, score_thr=0.0, npoint_thr=0)))
    for N in (1, 63, 64, 65, 1023, 1024, 1025, 2049):
        out.append(_checked("points_%d" % N, _boundary_scene(200 + N, N)))
    # six words a row: a wave of `rows` packs two of them; 69 chunks of points: the scan of `chunks` takes two steps
    c = make_scene(290, Q=4, C=2, S=321, N=900, n_inst=3)
    out.append(_checked("spp_321", dict(c, topk_insts=100, score_thr=0.0, npoint_thr=0)))
    out.append(_checked("points_70000", _boundary_scene(291, 70000, Q=2, C=1)))
    # 1024 chunks of 1025 points, sixteen steps of the scan; the points beyond one pass of `points` (2048 * 256)
    out.append(_checked("points_1048576", _boundary_scene(292, 1048576, Q=2, C=1)))
    out.append(_checked("tie_across_65536", _tie_block_scene()))
    base = make_scene(300, Q=5, C=3, S=20, N=400, n_inst=3)
    for name, topk in (("scores_below_topk", 20), ("scores_equal_topk", 15), ("scores_above_topk", 10), ("topk_one", 1)):
        out.append(_checked(name, dict(base, topk_insts=topk, score_thr=0.0, npoint_thr=5)))
    # the cut is taken on the class scores: query 0 has the best one and the weakest mask score
    c = make_scene(305, Q=3, C=1, S=5, N=60, n_inst=1)
    c["labels"][:] = np.float32(0.0)
    c["pred_scores"][:] = np.array([1.0, 0.9, 0.8], np.float32)
    c["masks"][:] = np.array([[0.05] * 5, [5.0] * 5, [5.5] * 5], np.float32)
    out.append(_checked("topk_before_mask_score", dict(c, topk_insts=2, score_thr=0.0, npoint_thr=0)))
    c = make_scene(311, Q=60, C=18, S=20, N=200, n_inst=5, max_run=6)
    out.append(_checked("topk_1024", dict(c, topk_insts=1024, score_thr=-1.0, npoint_thr=0)))
    # bit-identical class scores: queries 1 and 4 share labels and pred_scores; their masks differ
    c = make_scene(320, Q=6, C=3, S=24, N=500, n_inst=3)
    c["labels"][4], c["pred_scores"][4] = c["labels"][1], c["pred_scores"][1]
    s = ref.class_scores64(c["labels"], c["pred_scores"]).reshape(-1).astype(np.float32)
    first = int(np.nonzero(ref.order_ref(s, len(s)) == 1 * 3 + int(np.argmax(s[3:6])))[0][0])
    out.append(_checked("tie_across_cut", dict(c, topk_insts=first + 1, score_thr=0.0, npoint_thr=0)))
    c = dict(c, masks=c["masks"].copy())
    c["masks"][4] = c["masks"][1]  # and identical masks: identical conf, written in candidate order
    out.append(_checked("tie_inside", dict(c, topk_insts=18, score_thr=0.0, npoint_thr=0)))
    c = make_scene(330, Q=4, C=5, S=16, N=300, n_inst=2)
    c["labels"][2] = np.array([4.0, -3.0, 3.5, -3.0, -3.0, -2.0], np.float32)
    out.append(_checked("one_query_two_classes", dict(c, topk_insts=6, score_thr=0.0, npoint_thr=0)))
    for rows in (68, 132):  # the run-length stage: a thread of `finish` owns four rows
        c = make_scene(340 + rows, Q=8, C=18, S=12, N=260, n_inst=3, amp=1.0)
        c["masks"][:, c["superpoints"][0]] = np.float32(1.25)  # every row has a point
        out.append(_checked("rows_%d" % rows, dict(c, topk_insts=rows, score_thr=-1.0, npoint_thr=0)))
    c = make_scene(350, Q=5, C=3, S=66, N=400, n_inst=2)
    c["masks"][:, 5::7] = np.float32(0.0)
    c["masks"][:, 6::7] = np.float32(-0.0)
    out.append(_checked("zero_logits_not_set", dict(c, topk_insts=100, score_thr=0.0, npoint_thr=0)))
    c = make_scene(360, Q=5, C=3, S=20, N=300, n_inst=2)
    c["masks"][1] = -np.abs(c["masks"][1])
    c["masks"][3] = np.float32(-0.0)
    out.append(_checked("empty_row_score_thr_zero", dict(c, topk_insts=100, score_thr=0.0, npoint_thr=0)))
    out.append(_checked("empty_row_score_thr_negative", dict(c, topk_insts=100, score_thr=-0.5, npoint_thr=0)))
    c = make_scene(370, Q=6, C=3, S=20, N=400, n_inst=2)
    conf = ref.predict_ref(**c, topk_insts=100, score_thr=0.0, npoint_thr=0)["conf"]
    out.append(_checked("conf_equals_score_thr", dict(c, topk_insts=100, score_thr=float(conf[2]), npoint_thr=0)))
    # superpoint 0 has ten points, superpoint 1 one: npoints 10 (dropped at npoint_thr 10) and 11 (kept)
    c = make_scene(380, Q=4, C=3, S=6, N=40, n_inst=2)
    c["superpoints"] = np.array([0] * 10 + [1] + [2] * 9 + [3] * 20, np.int64)
    c["masks"][:] = np.float32(-2.0)
    c["masks"][0, 0] = c["masks"][1, 0] = c["masks"][1, 1] = c["masks"][2, 1] = np.float32(1.5)
    c["masks"][3, 5] = np.float32(2.0)  # a set superpoint without points: no point, no box
    out.append(_checked("npoints_at_the_threshold", dict(c, topk_insts=100, score_thr=0.0, npoint_thr=10)))
    out.append(_checked("one_point_instance", dict(c, topk_insts=100, score_thr=0.0, npoint_thr=0)))
    c = make_scene(390, Q=8, C=3, S=20, N=400, n_inst=3, negative=3)
    out.append(_checked("negative_scores_dropped", dict(c, topk_insts=100, score_thr=0.0, npoint_thr=5)))
    out.append(_checked("negative_scores_kept", dict(c, topk_insts=100, score_thr=-10.0, npoint_thr=5)))
    out.append(_checked("negative_scores_in_the_cut", dict(c, topk_insts=20, score_thr=-10.0, npoint_thr=5)))
    c = make_scene(400, Q=6, C=3, S=70, N=500, n_inst=2, used=9)
    c["masks"][:, ::2] = np.abs(c["masks"][:, ::2])  # empty superpoints set and unset in the masks
    out.append(_checked("empty_superpoints", dict(c, topk_insts=100, score_thr=0.0, npoint_thr=3)))
    c = make_scene(410, Q=5, C=3, S=10, N=200, n_inst=2)
    c["coords_float"][::3] *= np.float32(-1.0)
    c["coords_float"][5:60:5, 1] = np.float32(-0.0)
    c["coords_float"][7:60:5, 1] = np.float32(0.0)
    c["coords_float"][:, 2] = -np.abs(c["coords_float"][:, 2])
    out.append(_checked("mixed_sign_coords", dict(c, topk_insts=100, score_thr=0.0, npoint_thr=3)))
    c = make_scene(420, Q=5, C=3, S=10, N=200, n_inst=2)
    out.append(_checked("zero_rows", dict(c, topk_insts=100, score_thr=0.0, npoint_thr=200)))
    return out


def refusals():
    """(name, case, status, flags): what the data can be refused for, and the order of precedence."""
    base = dict(make_scene(500, Q=6, C=3, S=20, N=300, n_inst=2), topk_insts=100, score_thr=0.0, npoint_thr=0)

    def variant(**edits):
        c = dict(base)
        for key, (index, value) in edits.items():
            c[key] = c[key].copy()
            c[key][index] = value
        return c

    nan, inf = np.float32("nan"), np.float32("inf")
    out = [
        ("labels_nan", variant(labels=((2, 1), nan)), ref.ERR_NOT_FINITE, ref.FLAG_SCORE),
        ("labels_inf_last_column", variant(labels=((0, 3), inf)), ref.ERR_NOT_FINITE, ref.FLAG_SCORE),
        ("scores_inf", variant(pred_scores=(5, -inf)), ref.ERR_NOT_FINITE, ref.FLAG_SCORE),
        ("mask_nan", variant(masks=((3, 19), nan)), ref.ERR_NOT_FINITE, ref.FLAG_MASK),
        ("mask_inf", variant(masks=((0, 0), inf)), ref.ERR_NOT_FINITE, ref.FLAG_MASK),
        ("coords_nan", variant(coords_float=((299, 2), nan)), ref.ERR_NOT_FINITE, ref.FLAG_COORDS),
        ("coords_inf", variant(coords_float=((0, 0), -inf)), ref.ERR_NOT_FINITE, ref.FLAG_COORDS),
        ("spp_negative", variant(superpoints=(17, -1)), ref.ERR_SPP_RANGE, ref.FLAG_SPP),
        ("spp_equals_columns", variant(superpoints=(299, 20)), ref.ERR_SPP_RANGE, ref.FLAG_SPP),
        ("coords_before_spp", variant(coords_float=((4, 1), nan), superpoints=(0, 20)), ref.ERR_NOT_FINITE,
         ref.FLAG_COORDS | ref.FLAG_SPP),
        ("mask_before_coords_and_spp", variant(masks=((1, 7), nan), coords_float=((4, 1), nan), superpoints=(0, 20)),
         ref.ERR_NOT_FINITE, ref.FLAG_MASK | ref.FLAG_COORDS | ref.FLAG_SPP),
        ("scores_before_coords_and_spp", variant(labels=((1, 0), nan), coords_float=((4, 1), nan), superpoints=(0, 99)),
         ref.ERR_NOT_FINITE, ref.FLAG_SCORE | ref.FLAG_COORDS | ref.FLAG_SPP),
    ]
    for name, c, status, flags in out:
        got = ref.predict_ref(**c)
        assert (got["status"], got["flags"]) == (status, flags), name
    return out


def mask_refusal():
    """A non-finite logit in a row no candidate reads is no refusal: (refused, accepted) with topk_insts 3."""
    c = dict(make_scene(510, Q=6, C=3, S=20, N=300, n_inst=2), topk_insts=3, score_thr=0.0, npoint_thr=0)
    s = ref.class_scores64(c["labels"], c["pred_scores"]).reshape(-1).astype(np.float32)
    cand = ref.order_ref(s, 3) // 3
    outside = next(q for q in range(6) if q not in cand)
    bad, fine = dict(c, masks=c["masks"].copy()), dict(c, masks=c["masks"].copy())
    bad["masks"][cand[2], 4] = np.float32("nan")
    fine["masks"][outside, 4] = np.float32("nan")
    return bad, fine
