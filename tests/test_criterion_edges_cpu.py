"""The edge cases of the criterion kernels (tests/criterion_edge_cases.py) without a device: every case is what its name
says; the restatements tests/loss_ref.py and tests/point_loss_ref.py equal torch's float64 autograd ON the kinks (ties of
min / max, clamps at exactly 0, L1 differences of 0, x = 0, a sigmoid sum of exactly 0, the float32 faces of the
level-set membership); and each kink case tells the right convention from the wrong one a kernel could have, by more
than the comparison the device test uses (loss_ref.close) allows -- the evidence that tests/test_criterion_edges_gpu.py
would fail on a subtly wrong kernel.

A wrong convention is the restatement itself on inputs moved off the kink by one float64 step (or by -1e-300 at x = 0):
the values move by a rounding error, the gradients become the one-sided ones -- a tie share of 1 / 0, a clamp that
passes only above 0, sign(0) = +-1, an IoU that counts x > 0 only.  No second set of formulas is involved.

Tolerances against torch: the project's own (test_the_restatement_equals_torch_in_float64_on_an_active_clamp), values
rtol 1e-13, gradients rtol 1e-12 and atol 1e-15.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import criterion_edge_cases as cases
import loss_ref
import match_ref
import point_loss_ref
from gapro_amd import _lib, consumer_ops

UP64 = cases.UP.astype(np.float64)
BIG = 100000.0


def _restate(case, args=None, gt=None, up=UP64, empty_weight=None):
    return loss_ref.losses(gt=gt or case["gt"], upstream=up, empty_weight=case["empty_weight"] if empty_weight is None
                           else empty_weight, **(args or case["args"]))


def _beyond_close(wrong, right):
    """True where a device that returned ``wrong`` (rounded to float32) would fail loss_ref.close against ``right``."""
    with np.errstate(all="ignore"):
        w32 = np.asarray(wrong, dtype=np.float64).astype(np.float32)
    try:
        loss_ref.close(w32, right)
    except AssertionError:
        return True
    return False


def _moved(case, **edits):
    """A deep copy of the case's arguments in float64 (the restatement keeps float64 inputs as they are), edited:
    ``box=(row name, face, direction)`` moves that predicted face one float64 step, ``x_zero=value`` replaces the zeros
    of the x_zero row."""
    args = {k: (v if k == "batch_offsets" else [np.asarray(a, dtype=np.float64).copy() for a in v] if k == "mask_logits"
                else np.asarray(v, dtype=np.float64).copy()) for k, v in case["args"].items()}
    if "box" in edits:
        name, face, direction = edits["box"]
        q = case["query_of"][name]
        args["box_preds"][0, q, face] = np.nextafter(args["box_preds"][0, q, face], direction * np.inf)
    if "x_zero" in edits:
        x = args["mask_logits"][0][case["query_of"]["x_zero"]]
        assert not x.any()
        x[:] = edits["x_zero"]
    return args


# ---------------------------------------------------------------------------------------------- torch, in float64
def _torch_giou_loss(p, g):
    """1 - GIoU per row as plain tensor code: min / max for the faces, clamp(min=0) for the widths."""
    lo_i, hi_i = torch.max(p[:, :3], g[:, :3]), torch.min(p[:, 3:], g[:, 3:])
    lo_b, hi_b = torch.min(p[:, :3], g[:, :3]), torch.max(p[:, 3:], g[:, 3:])
    inter = torch.clamp(hi_i - lo_i, min=0).prod(1)
    vol_p = torch.clamp(p[:, 3:] - p[:, :3], min=0).prod(1)
    vol_g = torch.clamp(g[:, 3:] - g[:, :3], min=0).prod(1)
    union = vol_p + vol_g - inter
    bound = torch.clamp(hi_b - lo_b, min=0).prod(1)
    return 1 - (inter / (union + 1e-6) - (bound - union) / (bound + 1e-6))


def _torch_matched(case, up):
    """The seven losses of a one-sample case and the gradients of sum_k up[k] loss[k], every tensor float64; the
    membership mask alone comes from a float32 comparison, done once and passed in as a constant."""
    args, gt = case["args"], case["gt"]
    assert len(args["mask_logits"]) == 1
    t64 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    z, x, conf, box = (t64(a).requires_grad_() for a in (args["cls_logits"][0], args["mask_logits"][0],
                                                         args["conf_logits"][0], args["box_preds"][0]))
    rows = torch.as_tensor(np.asarray(gt["row_indices"][0], dtype=np.int64))
    t, box_l = t64(gt["inst_labels"][0]), t64(gt["box_labels"][0])
    w, feats = t64(args["prob_labels"]), t64(args["levelset_feats"])
    Q, C = z.shape
    n = len(rows)
    weight = t64(loss_ref.default_weight(C) if case["empty_weight"] is None else case["empty_weight"])
    member = torch.as_tensor(cases.members32(args["levelset_coords"], gt["box_labels"][0]))

    xm = x[rows]
    sig = torch.sigmoid(xm)
    dice = (1 - (2 * (sig * t).sum(1) + 1) / (sig.sum(1) + t.sum(1) + 1)).sum() / (n + 1e-6)
    bce = (F.binary_cross_entropy_with_logits(xm, t, reduction="none") * w[None, :]).sum() / w.sum() / (n + 1e-6)
    with torch.no_grad():
        binary = (sig >= 0.5).double()
        inter = (binary * t).sum(1)
        iou = inter / (binary.sum(1) + t.sum(1) - inter + 1e-6)
    iou_loss = ((conf[rows] - iou) ** 2).sum() / n
    target = torch.full((Q,), C - 1, dtype=torch.int64)
    target[rows] = torch.as_tensor(np.asarray(gt["cls_labels"][0], dtype=np.int64))
    cls_loss = F.cross_entropy(z, target, weight=weight)
    box_loss = (box[rows] - box_l).abs().sum() / n
    giou_loss = _torch_giou_loss(box[rows], box_l).sum() / n
    v = sig * member
    mean = (v @ feats) / torch.clamp(v.sum(1), min=1e-5)[:, None]
    spread = ((feats[None, :, :] - mean[:, None, :]) ** 2).sum(2)
    n_r = member.sum(1).double()
    per_box = torch.where(n_r > 0, (v * spread).sum(1) / torch.clamp(n_r, min=1), torch.zeros_like(n_r))
    levelset = per_box.sum() / (n + 1e-4)
    out = [dice, bce, cls_loss, iou_loss, box_loss, giou_loss, levelset]
    sum(float(u) * o for u, o in zip(up, out)).backward()
    return np.array([float(o.detach()) for o in out]), {"cls": z.grad.numpy()[None], "mask": [x.grad.numpy()],
                                                         "conf": conf.grad.numpy()[None], "box": box.grad.numpy()[None]}


def _equals_torch(vals, grads, t_vals, t_grads):
    assert np.allclose(vals, t_vals, rtol=1e-13, atol=0), np.abs(vals / t_vals - 1).max()
    for k in ("cls", "conf", "box"):
        assert np.allclose(grads[k], t_grads[k], rtol=1e-12, atol=1e-15), k
    assert np.allclose(grads["mask"][0], t_grads["mask"][0], rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("name", ["kinks", "faces"])
def test_matched_restatement_equals_torch_float64_autograd_on_the_kinks(name):
    case = getattr(cases, name)()
    vals, grads = _restate(case)
    assert np.isfinite(vals).all() and all(np.isfinite(g).all() for g in (grads["cls"], grads["mask"][0], grads["box"]))
    _equals_torch(vals, grads, *_torch_matched(case, UP64))


def test_matched_restatement_equals_torch_when_one_term_carries_the_gradient():
    """Each of the box and level-set terms by itself, so that a kink's share is not a small part of a sum."""
    for k in (4, 5, 6):
        up = np.zeros(7)
        up[k] = 1.0
        for case in (cases.kinks(), cases.faces()):
            _equals_torch(*_restate(case, up=up), *_torch_matched(case, up))


def _torch_point_wise(args, up):
    """The four point-wise losses on the points that have an instance, float64."""
    t64 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    z, c, conf = (t64(args[k]).requires_grad_() for k in ("semantic_scores", "corners_offset", "box_conf"))
    lab, at = t64(args["corners_offset_labels"]), t64(args["coords_float"])
    n = len(lab)
    sem = F.cross_entropy(z, torch.as_tensor(args["semantic_labels"]))
    here = torch.cat([at, at], 1)
    p, g = c + here, lab + here
    giou = _torch_giou_loss(p, g)
    with torch.no_grad():
        inter = torch.clamp(torch.min(p[:, 3:], g[:, 3:]) - torch.max(p[:, :3], g[:, :3]), min=0).prod(1)
        iou = inter / (torch.clamp(p[:, 3:] - p[:, :3], min=0).prod(1)
                       + torch.clamp(g[:, 3:] - g[:, :3], min=0).prod(1) - inter + 1e-6)
    out = [sem, (c - lab).abs().sum() / n, giou.sum() / n, ((conf - iou) ** 2).sum() / n]
    sum(float(u) * o for u, o in zip(up, out)).backward()
    return np.array([float(o.detach()) for o in out]), {"scores": z.grad.numpy(), "corners": c.grad.numpy(),
                                                         "conf": conf.grad.numpy()}


def test_point_wise_restatement_equals_torch_on_touching_identical_and_disjoint_pairs():
    args = cases.point_pairs()
    assert (args["instance_labels"] != -100).all() and (args["semantic_labels"] != -100).all()
    for up in (point_loss_ref.UPSTREAM, np.array([0.0, 1.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0, 0.0])):
        vals, grads = point_loss_ref.losses(upstream=up, **args)
        t_vals, t_grads = _torch_point_wise(args, up)
        assert np.allclose(vals[up != 0], t_vals[up != 0], rtol=1e-13, atol=0)
        for k in ("scores", "corners", "conf"):
            assert np.allclose(grads[k], t_grads[k], rtol=1e-12, atol=1e-15), k


# ---------------------------------------------------------------------------------------------- the cases are what they say
def _box_pair(case, name):
    r = case["row_of"][name]
    p = case["args"]["box_preds"][0, case["query_of"][name]]
    g = case["gt"]["box_labels"][0][r]
    assert p.dtype == g.dtype == np.float32
    return p, g


def test_kinks_preconditions():
    case = cases.kinks()
    args, gt = case["args"], case["gt"]
    assert np.array_equal(cases.UP, np.array([0.7, 1.3, 0.9, 1.1, 0.6, 1.7, 2.3], dtype=np.float32))
    assert len(set(cases.UP.tolist())) == 7
    assert args["cls_logits"].shape == (1, 16, 4) and args["mask_logits"][0].shape == (16, 16)
    assert len(gt["row_indices"][0]) == len(cases.KINK_ROWS) == 14 and len(set(gt["row_indices"][0].tolist())) == 14
    for k, face in enumerate(cases.FACES):
        p, g = _box_pair(case, "tie_" + face)
        assert p[k] == g[k], face                                      # a tie in float32
        assert (np.abs(np.delete(p, k).astype(np.float64) - np.delete(g, k)) >= 0.1).all(), face
        assert (p[3:] > p[:3]).all()
    p, g = _box_pair(case, "touching")
    assert p[0] == g[3] and float(min(p[3], g[3])) - float(max(p[0], g[0])) == 0.0
    assert (np.minimum(p[4:], g[4:]) - np.maximum(p[1:3], g[1:3]) > 0.1).all()
    p, g = _box_pair(case, "identical")
    assert np.array_equal(p, g)
    p, g = _box_pair(case, "zero_volume")
    assert p[0] == p[3] and g[0] < p[0] < g[3] and (p[4:] > p[1:3]).all()
    p, g = _box_pair(case, "inverted")
    assert p[3] < p[0] and (p[4:] > p[1:3]).all()
    p, g = _box_pair(case, "disjoint")
    assert p[0] > g[3] + 5
    x = args["mask_logits"][0]
    assert not x[case["query_of"]["x_zero"]].any() and (x[case["query_of"]["x_plus_1000"]] == 1000.0).all()
    r, q = case["row_of"]["x_minus_1000"], case["query_of"]["x_minus_1000"]
    inside = loss_ref.members(args["levelset_coords"], gt["box_labels"][0])[r]
    assert 3 <= inside.sum() < 16 and (x[q, inside] == -1000.0).all() and (np.abs(x[q, ~inside]) <= 5).all()
    assert float(torch.sigmoid(torch.as_tensor(x[q, inside].astype(np.float64))).sum()) == 0.0  # exactly, not just < 1e-5
    rest = np.ones_like(x, dtype=bool)
    rest[[case["query_of"][k] for k in ("x_zero", "x_minus_1000", "x_plus_1000")]] = False
    assert (np.abs(x[rest]) >= 0.1).all() and (np.abs(x[rest]) <= 5).all()
    # what the kinks do to the gradient, in the restatement (which equals torch there, above)
    _, grads = _restate(case, up=np.array([0, 0, 0, 0, 0, 1.0, 0]))
    assert grads["box"][0, case["query_of"]["touching"], 0] != 0.0     # the clamp passes at a width of exactly 0
    tiny = grads["box"][0, case["query_of"]["identical"]]
    assert tiny.all() and (np.abs(tiny) < 1e-6).all()                   # 0.5 A 1e-6 / (V + 1e-6)^2 per face, not zeros
    _, grads = _restate(case, up=np.array([0, 0, 0, 0, 1.0, 0, 0]))
    assert not grads["box"][0, case["query_of"]["identical"]].any()    # the L1 gradient: exact zeros


def test_identical_boxes_giou_gradient_is_the_share_of_the_two_1e_6_not_zero():
    """At box_preds == box_labels every pair is tied and inter = union = bound = V: with the 0.5 shares the derivative by
    a face is +-0.5 A 1e-6 / (V + 1e-6)^2, A the area of that face -- about 1e-8, and torch's autograd gives the same.
    It would be exact zeros only without the two 1e-6 of giou_aabb."""
    p, g = _box_pair(cases.kinks(), "identical")
    b = torch.as_tensor(g.astype(np.float64))[None]
    a = b.clone().requires_grad_()
    _torch_giou_loss(a, b).sum().backward()
    w = (g[3:] - g[:3]).astype(np.float64)
    V, A = w.prod(), np.array([w[1] * w[2], w[2] * w[0], w[0] * w[1]])
    want = 0.5 * A * 1e-6 / (V + 1e-6) ** 2
    # autograd forms it as a difference of terms near 1 / V, so it carries ~1e-16 / 3e-8 of cancellation
    assert np.allclose(a.grad.numpy()[0], np.concatenate([want, -want]), rtol=1e-6, atol=0)
    _, grad = loss_ref._giou(g[None].astype(np.float64), g[None].astype(np.float64), True)
    assert np.allclose(grad[0], a.grad.numpy()[0], rtol=1e-12, atol=1e-15)


def test_faces_preconditions_and_the_float64_membership_disagrees_on_both_sides():
    case = cases.faces()
    args, gt = case["args"], case["gt"]
    coords, box = args["levelset_coords"], gt["box_labels"][0]
    assert coords.shape == (cases.FACE_COLUMNS, 3) and coords.dtype == np.float32
    assert (box[0, :3] > -0.6).all() and (box[0, :3] < 0.3).all() and (box[0, 3:] > 1.9).all() and (box[0, 3:] < 3.5).all()
    lo, hi = (box[0, :3] - np.float32(0.005)).astype(np.float32), (box[0, 3:] + np.float32(0.005)).astype(np.float32)
    for k in range(3):
        assert coords[2 * k, k] == lo[k] and coords[2 * k + 1, k] == np.nextafter(lo[k], np.float32(-np.inf)) < lo[k]
        assert coords[6 + 2 * k, k] == hi[k] and coords[7 + 2 * k, k] == np.nextafter(hi[k], np.float32(np.inf)) > hi[k]
    m32 = loss_ref.members(coords, box)
    assert np.array_equal(m32, cases.members32(coords, box))
    assert m32[0, case["on_face"]].all() and not m32[0, case["off_face"]].any()
    assert np.isnan(coords[12]).sum() == 1 and np.isinf(coords[13]).sum() == 1
    assert not m32[0, 12] and not m32[0, 13] and m32[0, 14] and m32[0, 15] and not m32[0, 16] and not m32[0, 17]
    m64 = cases.members64(coords, box)
    differ = m32[0] != m64[0]
    assert differ[case["on_face"][:3] + case["off_face"][:3]].any(), "no cell of a lower face separates the two"
    assert differ[case["on_face"][3:] + case["off_face"][3:]].any(), "no cell of an upper face separates the two"
    assert not differ[12:].any()
    print("float32 / float64 membership differs in the columns", np.flatnonzero(differ).tolist())
    # a plain box such as 0 / 0.5 does not separate the two: the faces have to be chosen
    plain = np.array([[0, 0, 0, 0.5, 0.5, 0.5]], dtype=np.float32)
    on = np.full((6, 3), 0.25, dtype=np.float32)
    for k in range(3):
        on[k, k], on[3 + k, k] = np.float32(0.0) - np.float32(0.005), np.float32(0.5) + np.float32(0.005)
    assert np.array_equal(cases.members32(on, plain), cases.members64(on, plain))


@pytest.mark.parametrize("C", cases.CLASS_COUNTS)
def test_classes_preconditions(C):
    case = cases.classes(C)
    args, gt = case["args"], case["gt"]
    assert args["cls_logits"].shape == (1, 3, C) and args["mask_logits"][0].shape == (3, 5)
    assert gt["row_indices"][0].tolist() == [2, 0] and gt["cls_labels"][0].tolist() == [0, C - 1]
    w = case["empty_weight"]
    assert w.dtype == np.float32 and w.shape == (C,) and len(set(w.tolist())) == C and (w > 0).all()
    assert C == 1 or not np.array_equal(w, loss_ref.default_weight(C))
    assert [cases.classes(c)["cls_dtype"] for c in cases.CLASS_COUNTS] == ["int32", "int64", "int32", "int64"]
    if C in (65, 257):
        assert (C - 1) % 64 == 0 and (C - 1) % 256 in (0, 64)  # the first element of the second round of either loop
    vals, grads = _restate(case)
    assert np.isfinite(vals).all() and (C == 1 or grads["cls"].all())  # one class: softmax - onehot is 0


@pytest.mark.parametrize("name", cases.BATCHES)
def test_batches_preconditions(name):
    case = cases.batches(name)
    args, gt = case["args"], case["gt"]
    B = len(args["mask_logits"])
    kept = [b for b in range(B) if args["mask_logits"][b] is not None and gt["row_indices"][b] is not None]
    want = {"B5_last_kept": (5, [4]), "B9_wave0_skipped": (9, [1, 2, 3, 5, 6, 7]),
            "Bmax_every_third_skipped": (_lib.SPP_GT_MAX_SAMPLES, [b for b in range(_lib.SPP_GT_MAX_SAMPLES) if b % 3])}
    assert (B, kept) == want[name]
    assert args["cls_logits"].shape[:2] == (B, 2)
    sizes = np.diff(args["batch_offsets"])
    assert set(sizes[kept].tolist()) <= {1, 2, 3} and (name == "B5_last_kept" or set(sizes[kept].tolist()) == {1, 2, 3})
    skipped = [b for b in range(B) if b not in kept]
    assert name == "B5_last_kept" or {args["mask_logits"][b] is None for b in skipped} == {True, False}
    vals, grads = _restate(case)
    assert np.isfinite(vals).all() and vals.all()
    assert all((grads["mask"][b] is not None) == (b in kept) for b in range(B))
    assert not grads["cls"][skipped].any() and all(grads["cls"][b].any() for b in kept)


def test_rows_and_nan_backward_preconditions():
    case = cases.rows()
    assert case["args"]["mask_logits"][0].shape == (130, 3) and len(case["gt"]["row_indices"][0]) == 129
    assert 129 > 2 * 64 and 130 > 2 * 64  # three rounds of 64 lanes
    vals, grads = _restate(cases.nan_backward("zero_weight_sum"))
    assert np.isnan(vals[1]) and np.isfinite(np.delete(vals, 1)).all()
    rows = cases.nan_backward("zero_weight_sum")["gt"]["row_indices"][0]
    assert np.isnan(grads["mask"][0][rows]).all() and not grads["mask"][0][np.setdiff1d(np.arange(5), rows)].any()
    assert all(np.isfinite(grads[k]).all() for k in ("cls", "conf", "box"))
    case = cases.nan_backward("nan_box")
    vals, grads = _restate(case)
    assert np.isnan(vals[[4, 5]]).all() and np.isfinite(vals[[0, 1, 2, 3, 6]]).all()
    q = case["gt"]["row_indices"][0][1]
    assert np.isnan(case["args"]["box_preds"][0, q]).sum() == 1
    assert np.isnan(grads["box"][0, q]).any() and np.isfinite(np.delete(grads["box"][0], q, axis=0)).all()
    assert all(np.isfinite(g).all() for g in (grads["cls"], grads["conf"], grads["mask"][0]))


# ---------------------------------------------------------------------------------------------- each case discriminates
def _row_differs(wrong, right, q):
    """The box gradient of query q alone, with the bound of the whole array (loss_ref.close's)."""
    return _beyond_close(np.where(np.arange(right.shape[1])[None, :, None] == q, wrong, right), right)


@pytest.mark.parametrize("direction", [1, -1], ids=["pred_side", "label_side"])
def test_a_tie_share_of_one_or_zero_shows_in_every_tie_row_by_itself(direction):
    """GIoU alone: with the tied face a float64 step above (below) the label's, min / max hand the whole gradient to one
    operand -- the share 1.0 / 0.0 (0.0 / 1.0) a kernel written with `<` and `>=` would have."""
    case = cases.kinks()
    up = np.array([0, 0, 0, 0, 0, 1.7, 0])
    vals, grads = _restate(case, up=up)
    for k, face in enumerate(cases.FACES):
        w_vals, w_grads = _restate(case, args=_moved(case, box=("tie_" + face, k, direction)), up=up)
        assert not _beyond_close(w_vals, vals)              # the values cannot tell
        assert _row_differs(w_grads["box"], grads["box"], case["query_of"]["tie_" + face]), face
        assert np.array_equal(np.delete(w_grads["box"], case["query_of"]["tie_" + face], 1),
                              np.delete(grads["box"], case["query_of"]["tie_" + face], 1))
    for k in range(6):  # and at identical boxes, every face
        w_grads = _restate(case, args=_moved(case, box=("identical", k, direction)), up=up)[1]
        assert _row_differs(w_grads["box"], grads["box"], case["query_of"]["identical"]), k


def test_a_clamp_that_passes_only_above_zero_shows_at_touching_and_zero_volume_boxes():
    case = cases.kinks()
    up = np.array([0, 0, 0, 0, 0, 1.7, 0])
    vals, grads = _restate(case, up=up)
    # touching: lo_x one step up makes the intersection width negative; zero volume: hi_x one step down makes the
    # predicted width (and the intersection's) negative
    for name, face, direction in (("touching", 0, 1), ("zero_volume", 3, -1)):
        w_vals, w_grads = _restate(case, args=_moved(case, box=(name, face, direction)), up=up)
        assert not _beyond_close(w_vals, vals)
        assert _row_differs(w_grads["box"], grads["box"], case["query_of"][name]), name


def test_sign_of_zero_as_one_shows_in_every_tie_row_and_at_identical_boxes():
    case = cases.kinks()
    up = np.array([0, 0, 0, 0, 0.6, 0, 0])  # the L1 term alone
    vals, grads = _restate(case, up=up)
    for direction in (1, -1):
        for name, face in [("tie_" + f, k) for k, f in enumerate(cases.FACES)] + [("identical", k) for k in range(6)]:
            w_vals, w_grads = _restate(case, args=_moved(case, box=(name, face, direction)), up=up)
            assert not _beyond_close(w_vals, vals)
            q = case["query_of"][name]
            assert grads["box"][0, q, face] == 0.0 and w_grads["box"][0, q, face] != 0.0
            assert _row_differs(w_grads["box"], grads["box"], q), name


def test_an_iou_that_counts_x_above_zero_only_shows_in_the_x_zero_row():
    """x = -1e-300 has the sigmoid, the softplus and every gradient of x = 0 to the last bit and is not counted."""
    case = cases.kinks()
    vals, grads = _restate(case)
    w_vals, w_grads = _restate(case, args=_moved(case, x_zero=-1e-300))
    assert np.array_equal(np.delete(w_vals, 3), np.delete(vals, 3)) and _beyond_close(w_vals, vals)
    assert _beyond_close(w_grads["conf"], grads["conf"])
    assert np.array_equal(w_grads["mask"][0], grads["mask"][0]) and np.array_equal(w_grads["box"], grads["box"])


def test_a_float64_membership_shows_in_the_faces_case(monkeypatch):
    case = cases.faces()
    vals, grads = _restate(case)
    monkeypatch.setattr(loss_ref, "members", cases.members64)
    w_vals, w_grads = _restate(case)
    assert np.array_equal(w_vals[:6], vals[:6]) and _beyond_close(w_vals, vals)
    assert _beyond_close(w_grads["mask"][0], grads["mask"][0])
    monkeypatch.undo()
    kinks = cases.kinks()  # ... and not in a case whose coordinates are generic
    assert np.array_equal(cases.members64(kinks["args"]["levelset_coords"], kinks["gt"]["box_labels"][0]),
                          loss_ref.members(kinks["args"]["levelset_coords"], kinks["gt"]["box_labels"][0]))


def test_a_mean_without_its_clamp_is_nan_in_the_x_minus_1000_row():
    """A = 0 exactly: (sum v f) / A is 0 / 0 where (sum v f) / max(A, 1e-5) is 0, so a kernel that left the clamp out
    (or applied it only to a positive A) returns a NaN level-set loss and NaN gradients, which loss_ref.close refuses."""
    case = cases.kinks()
    args, gt = case["args"], case["gt"]
    r, q = case["row_of"]["x_minus_1000"], case["query_of"]["x_minus_1000"]
    inside = loss_ref.members(args["levelset_coords"], gt["box_labels"][0])[r]
    v = torch.sigmoid(torch.as_tensor(args["mask_logits"][0][q].astype(np.float64))).numpy() * inside
    a = v.sum()
    assert a == 0.0 and (v @ args["levelset_feats"].astype(np.float64) == 0.0).all()
    with np.errstate(invalid="ignore"):
        assert np.isnan((v @ args["levelset_feats"].astype(np.float64)) / a).all()
    vals, grads = _restate(case)
    wrong = vals.copy()
    wrong[6] = np.nan
    assert np.isfinite(vals[6]) and _beyond_close(wrong, vals)
    assert np.isfinite(grads["mask"][0][q]).all() and grads["mask"][0][q].any()


@pytest.mark.parametrize("C", [c for c in cases.CLASS_COUNTS if c > 1])
def test_an_unmatched_query_aimed_at_class_zero_shows(C):
    """Classes 0 and C - 1 swapped in the logits, the weights and the labels is the same problem with the unmatched
    queries aimed at (the original) class 0; its class gradient, swapped back, is that wrong kernel's."""
    case = cases.classes(C)
    vals, grads = _restate(case)
    swap = np.arange(C)
    swap[[0, C - 1]] = C - 1, 0
    args = dict(case["args"], cls_logits=case["args"]["cls_logits"][:, :, swap])
    gt = dict(case["gt"], cls_labels=[swap[c] for c in case["gt"]["cls_labels"]])
    w_vals, w_grads = _restate(case, args=args, gt=gt, empty_weight=case["empty_weight"][swap])
    assert _beyond_close(w_vals, vals) and _beyond_close(w_grads["cls"][:, :, swap], grads["cls"])
    # ... and the default weights instead of the case's show too
    d_vals, d_grads = loss_ref.losses(gt=case["gt"], upstream=UP64, **case["args"])
    assert _beyond_close(d_vals, vals) and _beyond_close(d_grads["cls"], grads["cls"])


def test_a_second_round_that_never_runs_shows():
    """The class logits beyond the first 64 (log-sum-exp) count in the loss; a sample beyond the fourth, a row or a
    query beyond the 64th count in the sums."""
    for C in (65, 257):
        case = cases.classes(C)
        vals, _ = _restate(case)
        z = case["args"]["cls_logits"][0].astype(np.float64)
        target = np.full(3, C - 1)
        target[case["gt"]["row_indices"][0]] = case["gt"]["cls_labels"][0]
        w = case["empty_weight"].astype(np.float64)[target]
        wrong = vals.copy()  # the log-sum-exp over the first round's 64 logits only
        wrong[2] += (w * (np.logaddexp.reduce(z[:, :64], 1) - np.logaddexp.reduce(z, 1))).sum() / w.sum()
        assert _beyond_close(wrong, vals)
    case = cases.batches("B5_last_kept")
    assert _restate(case)[0].all()  # sample 4 is everything there is
    case = cases.rows()
    vals, _ = _restate(case)
    gt = {k: [v[0][:128]] for k, v in case["gt"].items()}
    assert _beyond_close(_restate(case, gt=gt)[0], vals)


# ---------------------------------------------------------------------------------------------- match_cost's cases
def _want_cost(d, weights=match_ref.WEIGHTS):
    return [None if s is None else match_ref.cost(d["cls_logits"][b], s["mask_logits"], d["conf_logits"][b],
                                                  d["box_preds"][b], s["mask"], s["cls"], s["box"], weights=weights)
            for b, s in enumerate(d["samples"])]


def test_match_cases_are_what_they_say():
    for C in (1, 200):
        d = cases.match_classes(C)
        s = d["samples"][0]
        assert d["cls_logits"].shape == (1, 17, C) and s["mask_logits"].shape == (17, 5) and s["mask"].shape == (17, 5)
        assert C == 1 or s["cls"].max() >= 64
        assert np.isfinite(_want_cost(d)[0]).all() and (_want_cost(d)[0] != BIG).all()
    d = cases.match_batches("B40_every_other_none")
    assert len(d["samples"]) == 40 and all((s is None) == bool(b % 2) for b, s in enumerate(d["samples"]))
    assert all(s["mask"].shape[0] == 1 for s in d["samples"] if s is not None)
    d = cases.match_batches("Bmax")
    assert len(d["samples"]) == _lib.SPP_GT_MAX_SAMPLES == d["cls_logits"].shape[0] and d["cls_logits"].shape[1] == 17
    assert all(s["mask"].shape == (1, 1) and s["mask_logits"].shape == (17, 1) for s in d["samples"])
    d = cases.match_batches("Q65_I65_S3")
    assert d["samples"][0]["mask_logits"].shape == (65, 3) and d["samples"][0]["mask"].shape == (65, 3)
    for name in cases.MATCH_BATCHES:
        assert all(w is None or (np.isfinite(w).all() and (w != BIG).all()) for w in _want_cost(cases.match_batches(name)))


def test_match_infinite_logits_take_exactly_the_rows_stated():
    d = cases.match_class_logits()
    z, s = d["cls_logits"][0], d["samples"][0]
    assert s["cls"].tolist() == [0, 1, 2, 0] and 3 not in s["cls"]
    assert np.isneginf(z[0]).tolist() == [False, False, False, True] and np.isneginf(z[1]).tolist() == [True, False, False, False]
    assert np.isposinf(z[2]).sum() == 1 and np.isneginf(z[3]).all() and np.isfinite(z[4:]).all()
    want = _want_cost(d)[0]
    assert np.array_equal(np.flatnonzero((want == BIG).all(1)), d["big_rows"][0]) and (want == BIG).sum() == 2 * 4
    assert np.isfinite(want).all()
    only_class = match_ref.cost64(z, s["mask_logits"], d["conf_logits"][0], d["box_preds"][0], s["mask"], s["cls"],
                                  s["box"], weights=(1, 0, 0, 0, 0))
    assert (only_class[1, [0, 3]] == 0.0).all() and (only_class[1, [1, 2]] < 0.0).all()  # -inf on the target: a term of 0
    assert (only_class[0] < 0.0).all()
    d = cases.match_mask_logits()
    x = d["samples"][0]["mask_logits"]
    assert np.isposinf(x).sum() == 1 and np.isposinf(x[2]).any() and np.isneginf(x).sum() == 1 and np.isneginf(x[5]).any()
    want = _want_cost(d)[0]
    assert np.array_equal(np.flatnonzero((want == BIG).all(1)), d["big_rows"][0]) and (want == BIG).sum() == 2 * 4
    # the mask of the infinite logits' columns has both a 0 and a 1, or the one the kernel would meet is asserted here
    m = d["samples"][0]["mask"]
    print("mask under +inf:", m[:, 3].tolist(), "under -inf:", m[:, 6].tolist())


def test_match_boxes_are_the_kink_pairs_and_ties_are_ties():
    d, case = cases.match_boxes(), cases.kinks()
    for k, name in enumerate(cases.MATCH_BOX_PAIRS):
        p, g = _box_pair(case, name)
        assert np.array_equal(d["box_preds"][0, k], p) and np.array_equal(d["samples"][0]["box"][k], g)
    assert set(cases.MATCH_BOX_PAIRS) == {"tie_" + f for f in cases.FACES} | {"touching", "identical", "disjoint"}
    assert np.isfinite(_want_cost(d)[0]).all()
    only_giou = match_ref.cost64(d["cls_logits"][0], d["samples"][0]["mask_logits"], d["conf_logits"][0],
                                 d["box_preds"][0], d["samples"][0]["mask"], d["samples"][0]["cls"],
                                 d["samples"][0]["box"], weights=(0, 0, 0, 0, 1))
    k = cases.MATCH_BOX_PAIRS.index("identical")
    assert only_giou[k, k] == pytest.approx(-1.0, abs=1e-6)
    assert only_giou[cases.MATCH_BOX_PAIRS.index("disjoint"), cases.MATCH_BOX_PAIRS.index("disjoint")] > 0.0
    d = cases.match_ties()
    want = _want_cost(d)[0]
    assert want.shape == (4, 3) and want[0].tobytes() == want[1].tobytes() and want[:, 0].tobytes() == want[:, 1].tobytes()
    assert len(set(want[[0, 2, 3]][:, [0, 2]].ravel().tolist())) == 6
    for dup in (1, 2):  # the solver on the restatement's cost: a valid assignment of the optimal total
        rows, cols = consumer_ops.linear_sum_assignment(want, dup)
        assert match_ref.check_assignment(want, rows, cols, dup)
        assert match_ref.total(want, rows, cols) == pytest.approx(match_ref.brute_force(want, dup), rel=1e-12, abs=1e-12)


def test_point_pairs_are_what_they_say():
    args = cases.point_pairs()
    p, g = point_loss_ref.boxes(args["corners_offset"], args["corners_offset_labels"], args["coords_float"])
    x2 = np.tile(args["coords_float"].astype(np.float64), (1, 2))
    assert np.array_equal(p - x2, args["corners_offset"].astype(np.float64))  # the additions are exact
    assert np.array_equal(g - x2, args["corners_offset_labels"].astype(np.float64))
    assert p[0, 0] == g[0, 3] and (np.minimum(p[0, 4:], g[0, 4:]) - np.maximum(p[0, 1:3], g[0, 1:3]) > 0.01).all()
    assert np.array_equal(p[1], g[1]) and p[2, 0] > g[2, 3] + 5
    assert (np.abs(p[3:] - g[3:]) >= 0.1).all()
    _, grads = point_loss_ref.losses(upstream=np.array([0, 0, 1.0, 0]), **args)
    assert grads["corners"][0, 0] != 0.0 and grads["corners"][1].all() and (np.abs(grads["corners"][1]) < 1e-6).all()
    _, grads = point_loss_ref.losses(upstream=np.array([0, 1.0, 0, 0]), **args)
    assert not grads["corners"][1].any()


# ---------------------------------------------------------------------------------------------- the library's bound on B
def test_one_sample_more_than_the_library_admits_is_refused_before_a_device_is_touched():
    B, Q, C, S = _lib.SPP_GT_MAX_SAMPLES + 1, 2, 3, 2
    f = lambda *s: torch.zeros(*s, dtype=torch.float32)  # noqa: E731
    entry = {"mask": f(1, S), "cls": torch.zeros(1, dtype=torch.int64), "box": f(1, 6)}
    with pytest.raises(ValueError, match="batch size %d beyond %d" % (B, B - 1)):
        consumer_ops.match_cost(f(B, Q, C), [f(Q, S)] * B, f(B, Q), f(B, Q, 6), [entry] * B)
    with pytest.raises(ValueError, match="batch size %d beyond %d" % (B, B - 1)):
        consumer_ops.hungarian_match(f(B, Q, C), [f(Q, S)] * B, f(B, Q), f(B, Q, 6), [entry] * B)
    gt = {"row_indices": [np.array([0])] * B, "inst_labels": [f(1, S)] * B,
          "cls_labels": [torch.zeros(1, dtype=torch.int64)] * B, "box_labels": [f(1, 6)] * B}
    with pytest.raises(ValueError, match="batch size %d beyond %d" % (B, B - 1)):
        consumer_ops.matched_losses(f(B, Q, C), [f(Q, S)] * B, f(B, Q), f(B, Q, 6), f(B * S), list(range(0, B * S + 1, S)),
                                    f(B * S, 2), f(B * S, 3), gt)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # at the bound itself the checks pass
        B -= 1
        consumer_ops.matched_losses(f(B, Q, C), [f(Q, S)] * B, f(B, Q), f(B, Q, 6), f(B * S), list(range(0, B * S + 1, S)),
                                    f(B * S, 2), f(B * S, 3), {k: v[:B] for k, v in gt.items()})
