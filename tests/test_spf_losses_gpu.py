"""consumer_ops.spformer_match / spformer_layer_losses / spformer_criterion on the MI355X: the table and every gradient
against the NumPy float64 restatement tests/spf_loss_ref.py at the kernels' head, batch, query, column and class edges
and on edge data; heads alone against heads together, repeatability, the host reads, the device's refusals; the real
reference's outputs (tests/golden/spf_losses_*.npz).

Tolerances: device against the restatement 1 float32 ulp of the value plus 1e-9 times the array's largest magnitude
(tests/loss_ref.py close); device against a fixture 4 x the fixture's own ref_dev of that value or gradient array.
"""
import contextlib
import itertools

import numpy as np
import pytest

import spf_loss_ref as ref
from loss_ref import close

pytestmark = pytest.mark.gpu


def _dev(a, dtype=None):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    return t if dtype is None else t.to(dtype)


@contextlib.contextmanager
def no_host_read():
    """Fails on any synchronising call torch knows of: a device-to-host copy, ``item()``, a stream synchronisation."""
    import torch

    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode(before)


def problem(seed, L1, Q, C, F, shapes):
    """shapes: per sample (n, S), n = 0 for a sample without an instance.  Label boxes around the origin hold about half
    of the columns; every head has its own logits and its own random assignment."""
    rng = np.random.default_rng(seed)
    B = len(shapes)
    N = sum(S for _, S in shapes)
    p = {"labels": [rng.normal(0, 2, (B, Q, C)).astype(np.float32) for _ in range(L1)],
         "scores": [rng.uniform(0, 1, (B, Q, 1)).astype(np.float32) for _ in range(L1)],
         "masks": [[rng.normal(0, 3, (Q, S)).astype(np.float32) for _, S in shapes] for _ in range(L1)],
         "sp_coords": rng.uniform(-1.5, 1.5, (N, 3)).astype(np.float32),
         "sp_rgb_feats": rng.uniform(0, 1, (N, F)).astype(np.float32),
         "sp_prob_labels": rng.uniform(0.05, 1, N).astype(np.float32), "gts": [], "indices": None}
    for n, S in shapes:
        glo = rng.uniform(-1.6, -0.4, (n, 3))
        p["gts"].append(None if n == 0 else ((rng.integers(0, C - 1, n)).astype(np.int64),
                                             (rng.random((n, S)) < 0.4).astype(np.float32),
                                             np.concatenate([glo, glo + rng.uniform(1.2, 2.6, (n, 3))], 1).astype(np.float32)))
    empty = np.empty(0, dtype=np.int64)
    p["indices"] = [[(empty, empty) if n == 0 else (rng.permutation(Q)[:n].astype(np.int64), rng.permutation(n).astype(np.int64))
                     for n, _ in shapes] for _ in range(L1)]
    return p


LEVELSET_ONLY = np.array([[0, 0, 0, 0, 1]], dtype=np.float32)


def clamped_case():
    """One head, one matched row alone, the members of its instance's box at -14: A = members * sigmoid(-14) lies below
    the clamp of 1e-5 and within a factor of five of it, so the clamped mean's own derivative is of the level-set
    term's size.  For min_points = 3.  Returns the members too."""
    p = problem(61, 1, 1, 4, 3, [(1, 65)])
    mem = ref.members(p["sp_coords"], p["gts"][0][2])[0]
    p["masks"][0][0][0, mem] = -14.0
    return p, mem


def insts_of(p, cls_dtype=None, mask_dtype=None):
    import torch

    out = []
    for g, x in zip(p["gts"], p["masks"][0]):
        S = x.shape[1]
        cls, mask, box = g if g is not None else (np.empty(0, np.int64), np.empty((0, S), np.float32),
                                                  np.empty((0, 6), np.float32))
        out.append({"gt_labels": _dev(cls, cls_dtype or torch.int64), "gt_spmasks": _dev(mask, mask_dtype),
                    "gt_boxes": _dev(box)})
    return out


UP = np.array([0.7, 1.3, 0.9, 1.1, 2.3], dtype=np.float32)


def upstream(L1):
    return (UP[None, :] * (1.0 + 0.25 * np.arange(L1))[:, None]).astype(np.float32)


def run(p, up=None, backward=True, requires=("labels", "scores", "masks"), masks=None, insts=None, single=False,
        guard=contextlib.nullcontext, **kw):
    """One call (and its backward): the f32[L1, 5] and the gradients as NumPy, ``None`` where none was asked for.  The
    call and its backward run inside ``guard()``; the uploads before and the downloads after do not."""
    import torch
    from gapro_amd import consumer_ops as ops

    L1 = len(p["labels"])
    labels = [_dev(a).requires_grad_("labels" in requires) for a in p["labels"]]
    scores = [_dev(a).requires_grad_("scores" in requires) for a in p["scores"]]
    masks = masks if masks is not None else [[_dev(a) for a in head] for head in p["masks"]]
    for head in masks:
        for x in head:
            x.requires_grad_("masks" in requires)
    pick = (lambda v: v[0]) if single else (lambda v: v)
    insts = insts or insts_of(p)
    rest = [_dev(p["sp_coords"]), _dev(p["sp_rgb_feats"]), _dev(p["sp_prob_labels"])]
    up = _dev(upstream(L1) if up is None else up)
    torch.cuda.synchronize()
    with guard():
        out = ops.spformer_layer_losses(pick(labels), pick(scores), pick(masks), insts, pick(p["indices"]), *rest,
                                        p.get("batch_offsets"), **kw)
        if backward and requires:
            (out * up).sum().backward()
    assert out.is_cuda and out.shape == (L1, 5) and str(out.dtype) == "torch.float32"
    grads = None
    if backward and requires:
        g = lambda a: None if a.grad is None else a.grad.cpu().numpy()  # noqa: E731
        grads = {"labels": [g(a) for a in labels], "scores": [g(a) for a in scores],
                 "masks": [[g(a) for a in head] for head in masks]}
    return out.detach().cpu().numpy(), grads


def compare(p, up=None, **kw):
    L1 = len(p["labels"])
    up = upstream(L1) if up is None else up
    got, grads = run(p, up=up, **kw)
    opts = {k: v for k, v in kw.items() if k in ("non_object_weight", "weighted_bce", "dice_div_main", "min_points")}
    want, wg = ref.layer_losses(p["labels"], p["scores"], p["masks"], p["gts"], p["indices"], p["sp_coords"],
                                p["sp_rgb_feats"], p["sp_prob_labels"], upstream=up, **opts)
    assert close(got, want)
    for h in range(L1):
        assert close(grads["labels"][h], wg["labels"][h]), h
        assert close(grads["scores"][h].reshape(wg["scores"][h].shape), wg["scores"][h]), h
        for b, w in enumerate(wg["masks"][h]):
            if w is None:
                assert grads["masks"][h][b] is None
            else:
                assert grads["masks"][h][b].shape == w.shape and close(grads["masks"][h][b], w), (h, b)
    return got, grads, want, wg


# S on both sides of a wave (64) and of the workgroup's stride (256) and one column; heads, B (with skipped samples), Q,
# C, F and the n rule (1 or Q) rotate over them
SIZES = [1, 63, 64, 65, 255, 256, 257]


@pytest.mark.parametrize("k", range(len(SIZES)))
def test_edge_shapes_equal_the_restatement(k):
    L1, Q, C, F = (1, 2, 7)[k % 3], (1, 16, 17, 130)[k % 4], (2, 19, 65)[(k // 2) % 3], (1, 3, 8)[k % 3]
    S, S2 = SIZES[k], SIZES[(k + 3) % len(SIZES)]
    shapes = [[(1, S)], [(Q, S), (1, S2)], [(1, S), (0, 5), (Q, S2), (0, S), (min(Q, 3), 65)]][k % 3]
    compare(problem(100 + k, L1, Q, C, F, shapes), weighted_bce=bool(k & 1), dice_div_main=bool(k & 2), min_points=1 + k)


@pytest.mark.parametrize("L1,Q,C", [(7, 130, 2), (1, 17, 65), (2, 1, 19), (7, 16, 19)])
def test_the_other_sizes_of_heads_queries_and_classes(L1, Q, C):
    """What the rotation above leaves out; Q = 130 is more queries than a wave of the finishing kernel has lanes."""
    compare(problem(200 + Q, L1, Q, C, 3, [(Q, 65), (0, 9), (1, 130)]), min_points=20)


def test_a_batch_where_every_sample_is_skipped():
    p = problem(8, 2, 5, 4, 2, [(0, 7), (0, 3)])
    got, grads, want, _ = compare(p)
    assert (got[:, 0] > 0).all() and not got[:, 1:].any()
    assert all(g.any() for g in grads["labels"]) and not any(g.any() for g in grads["scores"])
    assert all(g is None for head in grads["masks"] for g in head)


def boxes_problem(counts=(99, 100, 101), extra=20):
    """One sample whose instance r holds exactly counts[r] columns in its box."""
    n, S = len(counts), sum(counts) + extra
    p = problem(31, 2, n + 2, 19, 3, [(n, S)])
    lo = np.array([[4.0 * r, 0.0, 0.0] for r in range(n)])
    box = np.concatenate([lo, lo + 1.0], 1).astype(np.float32)
    coords = np.full((S, 3), 50.0)
    rng = np.random.default_rng(32)
    owner = np.repeat(np.arange(n), counts)
    coords[:len(owner)] = lo[owner] + rng.uniform(0.1, 0.9, (len(owner), 3))
    order = rng.permutation(S)
    p["sp_coords"] = coords[order].astype(np.float32)
    p["gts"][0] = (p["gts"][0][0], p["gts"][0][1], box)
    assert ref.members(p["sp_coords"], box).sum(1).tolist() == list(counts)
    return p


def test_boxes_of_99_100_and_101_members_and_min_points():
    p = boxes_problem()
    col = ref.NAMES.index("levelset_loss")
    default, _, _, _ = compare(p)                  # min_points = 100: the first box takes no part
    one, _, _, _ = compare(p, min_points=1)
    edge, _, _, _ = compare(p, min_points=101)
    none, grads, _, _ = compare(p, min_points=102)
    assert (one[:, col] > default[:, col]).all() and (default[:, col] > edge[:, col]).all() and not none[:, col].any()
    assert np.array_equal(np.delete(one, col, 1), np.delete(default, col, 1))


def test_member_logits_at_minus_fourteen_take_the_clamped_mean():
    p, mem = clamped_case()
    assert 3 <= mem.sum() <= 12 and 2e-6 <= mem.sum() / (1.0 + np.exp(14.0)) < 1e-5
    got, grads, _, _ = compare(p, up=LEVELSET_ONLY, min_points=3)
    assert got[0, ref.NAMES.index("levelset_loss")] > 0 and grads["masks"][0][0][0, mem].all()


def score_problem(kind):
    """One sample of four instances on eight columns, the logits' signs chosen per matched row."""
    p = problem(41, 1, 6, 5, 2, [(4, 8)])
    t = np.zeros((4, 8), dtype=np.float32)
    t[:, :4] = 1.0
    p["gts"][0] = (p["gts"][0][0], t, p["gts"][0][2])
    rows, cols = p["indices"][0][0]
    x = p["masks"][0][0]
    mag = np.abs(x[rows]) + 0.5
    sign = {"tie": np.ones((4, 8)), "none": -np.ones((4, 8)), "all": 2.0 * t[cols] - 1.0}[kind].copy()
    if kind == "tie":
        sign[1] = 2.0 * t[cols][1] - 1.0  # the second row is kept: iou = 1
    x[rows] = (sign * mag).astype(np.float32)
    return p


@pytest.mark.parametrize("kind,n_kept", [("tie", 1), ("none", 0), ("all", 4)])
def test_score_filter_at_the_tie_with_no_row_and_with_every_row_kept(kind, n_kept):
    """x >= 0 everywhere against a mask of 4 of 8 columns: inter = 4, union = 8, 2 inter == union, iou = 0.5 - 6e-8: out."""
    p = score_problem(kind)
    got, grads, _, _ = compare(p)
    rows = p["indices"][0][0][0]
    g = grads["scores"][0].reshape(-1)
    assert np.count_nonzero(g) == n_kept and not np.delete(g, rows).any()
    assert (got[0, ref.NAMES.index("score_loss")] > 0) == (n_kept > 0)
    if kind == "tie":
        assert g[rows[1]] != 0.0


@pytest.mark.parametrize("weighted", [False, True])
def test_a_zero_weight_sum_is_nan_as_released_and_with_the_switch(weighted):
    p = problem(51, 2, 5, 4, 2, [(2, 65), (3, 7)])
    p["sp_prob_labels"][:65] = 0.0
    got, grads, _, _ = compare(p, weighted_bce=weighted)
    col = ref.NAMES.index("mask_bce_loss")
    assert np.isnan(got[:, col]).all() and not np.isnan(np.delete(got, col, 1)).any()
    assert np.isnan(grads["masks"][0][0][p["indices"][0][0][0]]).all() and not np.isnan(grads["masks"][0][1]).any()


def test_logits_at_plus_and_minus_100():
    p = problem(52, 2, 4, 3, 2, [(2, 257), (4, 64)])
    rng = np.random.default_rng(53)
    for head in p["masks"]:
        for x in head:
            x[...] = np.where(rng.random(x.shape) < 0.5, -100.0, 100.0)
    got, grads, _, _ = compare(p, min_points=1)
    assert np.isfinite(got).all() and all(np.isfinite(g).all() for head in grads["masks"] for g in head)


def test_strided_mask_rows_int32_labels_bool_masks_and_a_single_head():
    import torch

    p = problem(54, 1, 6, 19, 3, [(3, 65), (2, 130)])
    def wide():  # every row behind five columns that are not the sample's
        return [[_dev(np.concatenate([x, np.full((x.shape[0], 5), 77.0, np.float32)], 1))[:, :x.shape[1]] for x in head]
                for head in p["masks"]]

    assert not wide()[0][0].is_contiguous()
    a = run(p)
    b = run(p, masks=wide(), insts=insts_of(p, cls_dtype=torch.int32, mask_dtype=torch.bool), single=True)
    assert a[0].tobytes() == b[0].tobytes()
    for k in ("labels", "scores"):
        assert a[1][k][0].tobytes() == b[1][k][0].tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[1]["masks"][0], b[1]["masks"][0]))
    compare(p, masks=wide())
    p["batch_offsets"] = [0, 65, 195]
    c = run(p)
    p["batch_offsets"] = _dev(np.array([0, 65, 195]))  # on the device: not read
    d = run(p, check=False, guard=no_host_read)
    assert a[0].tobytes() == c[0].tobytes() == d[0].tobytes()


@pytest.mark.parametrize("requires", [c for r in range(4) for c in itertools.combinations(("labels", "scores", "masks"), r)])
def test_every_subset_of_requires_grad(requires):
    from gapro_amd import consumer_ops as ops

    p = problem(55, 2, 5, 4, 2, [(2, 65), (0, 4), (5, 7)])
    full = run(p)
    got, grads = run(p, requires=requires)
    assert got.tobytes() == full[0].tobytes()
    if not requires:
        out = ops.spformer_layer_losses([_dev(a) for a in p["labels"]], [_dev(a) for a in p["scores"]],
                                        [[_dev(a) for a in head] for head in p["masks"]], insts_of(p), p["indices"],
                                        _dev(p["sp_coords"]), _dev(p["sp_rgb_feats"]), _dev(p["sp_prob_labels"]))
        assert not out.requires_grad
        return
    for k in ("labels", "scores"):
        for h in range(2):
            assert (grads[k][h] is None) == (k not in requires)
            assert grads[k][h] is None or grads[k][h].tobytes() == full[1][k][h].tobytes()
    for h in range(2):
        for b in range(3):
            g = grads["masks"][h][b]
            assert (g is None) == ("masks" not in requires or b == 1)
            assert g is None or g.tobytes() == full[1]["masks"][h][b].tobytes()


def test_one_mask_alone_requires_grad():
    p = problem(56, 2, 5, 4, 2, [(2, 65), (5, 7)])
    full = run(p)
    masks = [[_dev(a) for a in head] for head in p["masks"]]
    from gapro_amd import consumer_ops as ops

    masks[1][0].requires_grad_()
    out = ops.spformer_layer_losses([_dev(a) for a in p["labels"]], [_dev(a) for a in p["scores"]], masks, insts_of(p),
                                    p["indices"], _dev(p["sp_coords"]), _dev(p["sp_rgb_feats"]),
                                    _dev(p["sp_prob_labels"]))
    (out * _dev(upstream(2))).sum().backward()
    assert masks[1][0].grad.cpu().numpy().tobytes() == full[1]["masks"][1][0].tobytes()
    assert all(masks[h][b].grad is None for h, b in ((0, 0), (0, 1), (1, 1)))


def test_seven_heads_equal_seven_calls_of_one_head_bit_for_bit():
    p = problem(57, 7, 17, 19, 3, [(17, 257), (0, 6), (3, 64)])
    up = upstream(7)
    got, grads = run(p, up=up, dice_div_main=True)
    for h in range(7):
        one = {**p, "labels": [p["labels"][h]], "scores": [p["scores"][h]], "masks": [p["masks"][h]],
               "indices": [p["indices"][h]]}
        g1, gr1 = run(one, up=up[h:h + 1], dice_div_main=True)
        assert g1.tobytes() == got[h:h + 1].tobytes(), h
        assert gr1["labels"][0].tobytes() == grads["labels"][h].tobytes()
        assert gr1["scores"][0].tobytes() == grads["scores"][h].tobytes()
        assert all((x is None and y is None) or x.tobytes() == y.tobytes()
                   for x, y in zip(gr1["masks"][0], grads["masks"][h]))
    main = {**p, "labels": [p["labels"][6]], "scores": [p["scores"][6]], "masks": [p["masks"][6]],
            "indices": [p["indices"][6]]}
    assert run(main, backward=False)[0].tobytes() == run(p, backward=False)[0][6:7].tobytes()  # as released, too


def test_two_calls_give_equal_bytes():
    p = problem(58, 3, 17, 19, 8, [(17, 257), (5, 255)])
    a, b = run(p), run(p)
    assert a[0].tobytes() == b[0].tobytes()
    for k in ("labels", "scores"):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a[1][k], b[1][k]))
    assert all(x.tobytes() == y.tobytes() for ha, hb in zip(a[1]["masks"], b[1]["masks"]) for x, y in zip(ha, hb))


def test_check_false_makes_no_host_read():
    p = problem(59, 2, 6, 5, 3, [(2, 65), (0, 3), (3, 9)])
    want = run(p)
    got = run(p, check=False, guard=no_host_read)  # the forward and the backward
    assert got[0].tobytes() == want[0].tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got[1]["labels"], want[1]["labels"]))
    with pytest.raises(RuntimeError):  # the guard is one: it sees the status read of check=True
        run(p, guard=no_host_read)


@pytest.mark.parametrize("bad", ["label -1", "label num_class", "mask 0.5"])
def test_the_device_refuses_a_label_or_a_mask_value_and_writes_a_zero_backward(bad):
    from gapro_amd._lib import GaproError

    C = 5
    p = problem(60, 2, 5, C, 3, [(3, 65), (2, 63)])
    cls, mask, box = p["gts"][1]
    col = int(p["indices"][1][1][1][0])  # matched in head 1
    if bad.startswith("label"):
        cls[col] = -1 if bad == "label -1" else C - 1
        text = "a GT label outside"
    else:
        mask[col, 7] = 0.5
        text = "a GT mask value that is neither 0 nor 1"
    with pytest.raises(GaproError, match="head 0, sample 1: " + text):
        run(p, backward=False)
    got, grads = run(p, check=False)
    assert np.isnan(got).all()
    for k in ("labels", "scores"):
        assert all(g.shape == a.shape and not g.any() for g, a in zip(grads[k], p[k]))
    assert all(g.shape == a.shape and not g.any() for hg, ha in zip(grads["masks"], p["masks"]) for g, a in zip(hg, ha))


# ---- the matcher and the criterion -----------------------------------------------------------------------------------
def fixture_call(name):
    z, args = ref.fixture(name)
    p = {"labels": args["labels"], "scores": args["scores"], "masks": args["masks"], "gts": args["gts"],
         "indices": args["indices"], "sp_coords": args["sp_coords"], "sp_rgb_feats": args["sp_rgb_feats"],
         "sp_prob_labels": args["sp_prob_labels"], "batch_offsets": args["batch_offsets"].tolist()}
    p["gts"] = [None if g is None else (g[0], g[1].astype(np.float32), g[2]) for g in p["gts"]]
    return z, p


@pytest.mark.parametrize("name", ref.FIXTURES)
def test_match_finds_the_fixture_assignments_and_costs_equal_the_restatement(name):
    from gapro_amd import consumer_ops as ops

    z, p = fixture_call(name)
    insts = insts_of(p)
    labels, masks = [_dev(a) for a in p["labels"]], [[_dev(a) for a in head] for head in p["masks"]]
    found = ops.spformer_match(labels, masks, insts)
    for h, head in enumerate(found):
        for b, (r, c) in enumerate(head):
            assert str(r.dtype) == str(c.dtype) == "torch.int64" and not r.is_cuda
            want = p["indices"][h][b]
            assert sorted(zip(r.tolist(), c.tolist())) == sorted(zip(want[0].tolist(), want[1].tolist())), (h, b)
    single = ops.spformer_match(labels[0], masks[0], insts, cost_weight=(1, 1, 1))
    assert all(a[0].equal(b[0]) and a[1].equal(b[1]) for a, b in zip(single, found[0]))
    # the class / BCE / dice terms are the ISBNet matcher's: its cost with SPFormer's weights is this cost
    b = next(k for k, g in enumerate(p["gts"]) if g is not None)
    n = len(p["gts"][b][0])
    B, Q = p["labels"][0].shape[:2]
    dc = [None] * B
    dc[b] = {"mask": insts[b]["gt_spmasks"], "cls": insts[b]["gt_labels"], "box": insts[b]["gt_boxes"]}
    cost = ops.match_cost(labels[0], masks[0], _dev(np.zeros((B, Q), np.float32)), _dev(np.zeros((B, Q, 6), np.float32)), dc,
                          weights={"class": 1, "dice": 1, "bce": 1, "conf": 0, "giou": 0})[b].cpu().numpy()
    assert cost.shape == (Q, n)
    assert close(cost, ref.cost_matrix(p["labels"][0][b], p["masks"][0][b], p["gts"][b][0], p["gts"][b][1]))


@pytest.mark.parametrize("name", ref.FIXTURES)
def test_fixture_equals_the_reference(name):
    """Within 4 x ref_dev (|float32 run - float64 run| of the reference itself) of the reference's float32 values."""
    z, p = fixture_call(name)
    got, grads = run(p, up=z["upstream"].astype(np.float32))
    dev = np.abs(got.astype(np.float64) - z["ref_table32"])
    print("%s: table: device - reference\n%s\nref_dev\n%s" % (name, dev, z["ref_dev_table"]))
    assert (dev <= 4 * z["ref_dev_table"]).all()
    Q = int(z["n_queries"])
    for h in range(int(z["n_heads"])):
        worst = {k: np.abs(grads[k][h].astype(np.float64) - z["ref_g%s32_%d" % (k, h)]).max() for k in ("labels", "scores")}
        worst["masks"] = 0.0
        for b, g in enumerate(p["gts"]):
            if g is None:
                assert grads["masks"][h][b] is None
                continue
            rows = p["indices"][h][b][0]
            assert not grads["masks"][h][b][np.setdiff1d(np.arange(Q), rows)].any()
            worst["masks"] = max(worst["masks"], np.abs(grads["masks"][h][b][rows].astype(np.float64)
                                                         - z["ref_gmasks32_%d_%d" % (h, b)]).max())
        for k, v in worst.items():
            print("%s: head %d grad %s: device - reference %.3g, ref_dev %.3g" % (name, h, k, v, z["ref_dev_%s" % k][h]))
            assert v <= 4 * z["ref_dev_%s" % k][h], (h, k)


@pytest.mark.parametrize("name", ref.FIXTURES)
def test_criterion_is_the_three_calls_and_equals_the_fixture_loss(name):
    import torch
    from gapro_amd import consumer_ops as ops

    z, p = fixture_call(name)
    L1 = int(z["n_heads"])

    def pred_of():
        heads = [{"labels": _dev(p["labels"][h]).requires_grad_(), "scores": _dev(p["scores"][h]).requires_grad_(),
                  "masks": [_dev(a).requires_grad_() for a in p["masks"][h]]} for h in range(L1)]
        pred = dict(heads[-1])
        pred.update({k: _dev(z[k]) for k in ("sp_coords", "sp_rgb_feats", "sp_prob_labels", "sp_mu_labels",
                                             "sp_var_labels", "batch_offsets")})
        pred["sp_mu_preds"] = _dev(z["sp_mu_preds"]).requires_grad_()
        pred["sp_logvar_preds"] = _dev(z["sp_logvar_preds"]).requires_grad_()
        if L1 > 1:
            pred["aux_outputs"] = heads[:-1]
        return pred, heads

    insts = insts_of(p, mask_dtype=torch.uint8)
    lw = (1.0, 1.0, 1.0, 1.0, 0.5)
    pred, heads = pred_of()
    loss, out = ops.spformer_criterion(pred, insts, loss_weight=lw, cost_weight=(1.0, 1.0, 1.0))
    keys = list(ref.OUT_NAMES) + ["kl_loss"] + ["layer_%d_%s" % (i, k) for i in range(L1 - 1) for k in ref.OUT_NAMES]
    assert list(out) == keys + ["loss"]
    assert all(v.is_cuda and v.dim() == 0 and not v.requires_grad for v in out.values())
    assert loss.requires_grad and loss.dim() == 0 and float(loss) == float(out["loss"])
    loss.backward()

    # the three calls written out
    pred2, heads2 = pred_of()
    labels, scores, masks = ([h[k] for h in heads2] for k in ("labels", "scores", "masks"))
    indices = ops.spformer_match(labels, masks, insts, (1.0, 1.0, 1.0))
    table = ops.spformer_layer_losses(labels, scores, masks, insts, indices, pred2["sp_coords"], pred2["sp_rgb_feats"],
                                      pred2["sp_prob_labels"], num_class=18)
    kl = ops.kl_to_gp_loss(pred2["sp_mu_preds"], pred2["sp_logvar_preds"], pred2["sp_mu_labels"], pred2["sp_var_labels"],
                           weight=0.1)
    total = ((table.double() * _dev(np.array(lw))).sum() + kl.double()).float()
    total.backward()
    assert float(total) == float(loss) and float(kl) == float(out["kl_loss"])
    prefix = ["layer_%d_" % i for i in range(L1 - 1)] + [""]
    for h in range(L1):
        for k, name_k in enumerate(ref.NAMES):
            assert float(out[prefix[h] + name_k]) == float(table[h, k])
        assert heads[h]["labels"].grad.equal(heads2[h]["labels"].grad) and heads[h]["scores"].grad.equal(heads2[h]["scores"].grad)
        for a, b in zip(heads[h]["masks"], heads2[h]["masks"]):
            assert (a.grad is None and b.grad is None) or a.grad.equal(b.grad)
    assert pred["sp_mu_preds"].grad.equal(pred2["sp_mu_preds"].grad)

    # the reference: loss, kl and the table behind the keys
    print("%s: loss %.9g, reference %.9g (float32 run) %.12g (float64 run), ref_dev %.3g; kl %.9g, reference %.9g"
          % (name, float(loss), float(z["ref_loss32"]), float(z["ref_loss64"]), float(z["ref_dev_loss"]),
             float(out["kl_loss"]), float(z["ref_kl32"])))
    assert abs(float(loss) - float(z["ref_loss32"])) <= 4 * float(z["ref_dev_loss"])
    assert abs(float(out["kl_loss"]) - float(z["ref_kl32"])) <= 4 * float(z["ref_dev_kl"])

    # as_floats: Python floats from one host copy; check=False: the matcher's synchronisation is the call's only one
    pred3, _ = pred_of()
    loss3, floats = ops.spformer_criterion(pred3, insts, loss_weight=lw, cost_weight=(1.0, 1.0, 1.0), as_floats=True)
    assert list(floats) == list(out) and all(type(v) is float for v in floats.values())
    assert all(floats[k] == float(out[k]) for k in out)
    reads = []
    real = ops._host_read
    ops._host_read = lambda *a, **k: (reads.append(1), real(*a, **k))[1]
    try:
        torch.cuda.set_sync_debug_mode("warn")
        import warnings
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            loss4, out4 = ops.spformer_criterion(pred3, insts, loss_weight=lw, cost_weight=(1.0, 1.0, 1.0), check=False)
            loss4.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
        ops._host_read = real
    assert len(reads) == 1 and len([w for w in caught if "synchroniz" in str(w.message).lower()]) <= 1
    torch.cuda.synchronize()
    assert float(loss4) == float(loss)
