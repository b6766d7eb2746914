"""consumer_ops.matched_losses on the MI355X: losses and all four gradients against the NumPy float64 restatement
tests/loss_ref.py at the kernels' column, wave and batch edges and on edge data; the other call forms, repeatability,
the device's refusal; the real reference's outputs (tests/golden/losses_*.npz); and the chain get_spp_gt ->
hungarian_match -> matched_losses -> backward.

Tolerances (tests/loss_ref.py): device against the restatement 1 float32 ulp of the value plus 1e-9 times the array's
largest magnitude; device against a fixture 4 x the fixture's own ref_dev of that loss or gradient array.
"""
import numpy as np
import pytest

import loss_ref as ref

pytestmark = pytest.mark.gpu

UP = np.array([0.7, 1.3, 0.9, 1.1, 0.6, 1.7, 2.3], dtype=np.float32)


def _dev(a, dtype=None):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    return t if dtype is None else t.to(dtype)


def _problem(seed, Q, C, F, shapes):
    """shapes: per sample (n_gt, S), "no_logits" or "no_rows".  Label boxes around the origin hold about half of the
    columns; the predictions stay off the boxes' ties."""
    rng = np.random.default_rng(seed)
    B = len(shapes)
    sizes = [s[1] if isinstance(s, tuple) else 7 for s in shapes]
    off = np.cumsum([0] + sizes)
    N = int(off[-1])
    lo = rng.uniform(-2, 0, (B, Q, 3))
    args = {"cls_logits": rng.normal(0, 2, (B, Q, C)).astype(np.float32), "mask_logits": [],
            "conf_logits": rng.normal(0, 1, (B, Q)).astype(np.float32),
            "box_preds": np.concatenate([lo, lo + rng.uniform(0.5, 3, (B, Q, 3))], 2).astype(np.float32),
            "prob_labels": rng.uniform(0.05, 1, N).astype(np.float32), "batch_offsets": off,
            "levelset_feats": rng.uniform(0, 1, (N, F)).astype(np.float32),
            "levelset_coords": rng.uniform(-1.5, 1.5, (N, 3)).astype(np.float32)}
    gt = {k: [] for k in ("row_indices", "inst_labels", "cls_labels", "box_labels")}
    for s, S in zip(shapes, sizes):
        n = s[0] if isinstance(s, tuple) else 2
        args["mask_logits"].append(None if s == "no_logits" else rng.normal(0, 3, (Q, S)).astype(np.float32))
        glo = rng.uniform(-1.6, -0.4, (n, 3))
        gt["row_indices"].append(None if s == "no_rows" else rng.permutation(Q)[:n].astype(np.int64))
        gt["inst_labels"].append((rng.random((n, S)) < 0.4).astype(np.float32))
        gt["cls_labels"].append(rng.integers(0, C, n).astype(np.int64))
        gt["box_labels"].append(np.concatenate([glo, glo + rng.uniform(1.2, 2.6, (n, 3))], 1).astype(np.float32))
    return args, gt


LEVELSET_ONLY = np.array([0, 0, 0, 0, 0, 0, 1], dtype=np.float32)


def fractional_case():
    """Targets from {0, 0.25, 0.5, 1}: the op takes any float32 target as the value it is."""
    args, gt = _problem(16, 5, 4, 3, [(3, 257), (1, 64)])
    rng = np.random.default_rng(17)
    gt["inst_labels"] = [rng.choice(np.array([0, 0.25, 0.5, 1], dtype=np.float32), a.shape) for a in gt["inst_labels"]]
    return args, gt


def clamped_case():
    """One matched row alone, the members of its label box at -14: A = members * sigmoid(-14) lies below the clamp
    of 1e-5 and within a factor of five of it, so the clamped mean's own derivative is of the level-set term's size.
    Returns the members too."""
    args, gt = _problem(303, 1, 3, 3, [(1, 65)])  # a seed whose box holds 6 of the 65 columns
    mem = ref.members(args["levelset_coords"], gt["box_labels"][0])[0]
    args["mask_logits"][0][0, mem] = -14.0
    return args, gt, mem


def _run(args, gt, up=UP, backward=True, requires=("cls", "mask", "conf", "box"), cls_dtype=None, logits=None, **kw):
    """One call (and its backward): the f32[7] and the gradients as NumPy, ``None`` where none was asked for."""
    import torch
    from gapro_amd import consumer_ops as ops

    t = {k: _dev(args[k]) for k in ("cls_logits", "conf_logits", "box_preds", "prob_labels", "levelset_feats",
                                    "levelset_coords")}
    x = logits if logits is not None else [None if a is None else _dev(a) for a in args["mask_logits"]]
    for k, name in (("cls", "cls_logits"), ("conf", "conf_logits"), ("box", "box_preds")):
        t[name].requires_grad_(k in requires)
    mask_req = requires if isinstance(requires, dict) else {"mask": "mask" in requires}
    for b, a in enumerate(x):
        if a is not None:
            a.requires_grad_(bool(mask_req.get("mask") is True or (isinstance(mask_req.get("mask"), (list, tuple))
                                                                    and b in mask_req["mask"])))
    dgt = {"row_indices": gt["row_indices"],
           "inst_labels": [None if a is None else _dev(a) for a in gt["inst_labels"]],
           "cls_labels": [None if a is None else _dev(a, cls_dtype or torch.int64) for a in gt["cls_labels"]],
           "box_labels": [None if a is None else _dev(a) for a in gt["box_labels"]]}
    out = ops.matched_losses(t["cls_logits"], x, t["conf_logits"], t["box_preds"], t["prob_labels"],
                             args["batch_offsets"], t["levelset_feats"], t["levelset_coords"], dgt, **kw)
    assert list(out) == list(ref.NAMES) + ["kl_loss"] and float(out["kl_loss"]) == 0.0 and not out["kl_loss"].requires_grad
    vec = torch.stack([out[k] for k in ref.NAMES])
    assert vec.is_cuda and vec.dtype == torch.float32
    grads = None
    if backward:
        (vec * _dev(np.asarray(up, dtype=np.float32))).sum().backward()
        g = lambda a: None if a is None or a.grad is None else a.grad.cpu().numpy()  # noqa: E731
        grads = {"cls": g(t["cls_logits"]), "conf": g(t["conf_logits"]), "box": g(t["box_preds"]),
                 "mask": [g(a) for a in x]}
    return vec.detach().cpu().numpy(), grads


def _compare(args, gt, up=UP, **kw):
    got, grads = _run(args, gt, up=up, **kw)
    want, wgrads = ref.losses(gt=gt, upstream=up, empty_weight=None if "empty_weight" not in kw else
                              kw["empty_weight"].cpu().numpy(), voxel_scale=kw.get("voxel_scale", 50), **args)
    assert ref.close(got, want)
    for k in ("cls", "conf", "box"):
        assert ref.close(grads[k], wgrads[k]), k
    for b, w in enumerate(wgrads["mask"]):
        if w is None:
            assert grads["mask"][b] is None
        else:
            assert grads["mask"][b].shape == w.shape and ref.close(grads["mask"][b], w), b
    return got, grads, want, wgrads


# S on both sides of a wave (64) and of the workgroup's stride (256), one column, and several rounds of the stride; Q, C,
# F and the n_gt rule (1 or Q) rotate over them, the second sample taking the other rule and another S
SIZES = [1, 63, 64, 65, 255, 256, 257, 1025]


@pytest.mark.parametrize("k", range(len(SIZES)))
def test_edge_shapes_equal_the_restatement(k):
    Q, C, F = (1, 5, 17)[k % 3], (2, 19)[k % 2], (1, 3, 8)[(k // 2) % 3]
    S, S2 = SIZES[k], SIZES[(k + 3) % len(SIZES)]
    args, gt = _problem(100 + k, Q, C, F, [(Q if k % 2 else 1, S), (1 if k % 2 else Q, S2)])
    _compare(args, gt)


@pytest.mark.parametrize("Q,C,F", [(17, 2, 8), (1, 19, 3), (5, 19, 1), (70, 3, 2)])
def test_every_size_of_q_c_and_f(Q, C, F):
    """The combinations the rotation above leaves out, and Q = 70: more queries than a wave of the finishing kernel."""
    args, gt = _problem(200 + Q, Q, C, F, [(Q, 65), (1, 130)])
    _compare(args, gt)


def test_batches_with_skipped_samples_and_different_sizes():
    args, gt = _problem(7, 6, 4, 3, [(3, 65), "no_logits", "no_rows", (6, 130)])
    got, grads, _, _ = _compare(args, gt)
    assert grads["mask"][1] is None and grads["mask"][2] is None
    assert not grads["cls"][1:3].any() and not grads["conf"][1:3].any() and not grads["box"][1:3].any()
    assert grads["cls"][0].any() and grads["cls"][3].any()
    first, _ = _run({**args, "cls_logits": args["cls_logits"][:1], "conf_logits": args["conf_logits"][:1],
                     "box_preds": args["box_preds"][:1], "mask_logits": args["mask_logits"][:1],
                     "batch_offsets": args["batch_offsets"][:2]}, {k: v[:1] for k, v in gt.items()}, backward=False)
    assert (got != first).any()  # the skipped samples count in the division by B


def test_all_skipped_batch_is_zeros():
    args, gt = _problem(8, 4, 3, 2, ["no_logits", "no_rows"])
    got, _ = _run(args, gt, backward=False)
    assert got.shape == (7,) and not got.any()


def test_edge_data_equals_the_restatement():
    """x = 0 (counts for the IoU), |x| = 100, a predicted box with min above max, a label box that holds no column."""
    args, gt = _problem(9, 6, 5, 3, [(4, 130), (2, 65)])
    rows = gt["row_indices"][0]
    x = args["mask_logits"][0]
    x[rows[0], ::3] = 0.0
    x[rows[1], ::2] = 100.0
    x[rows[1], 1::4] = -100.0
    x[rows[2], :] = 100.0
    args["box_preds"][0, rows[0], 3:] = args["box_preds"][0, rows[0], :3] - 0.5
    gt["box_labels"][0][3] += 40.0
    got, grads, want, _ = _compare(args, gt)
    assert np.isfinite(got).all() and all(np.isfinite(g).all() for g in grads["mask"])
    x0 = np.zeros_like(x)  # every logit 0: every column counts, iou = sum t / S
    args["mask_logits"][0] = x0
    got0, _ = _run(args, gt, backward=False)
    assert ref.close(got0, ref.losses(gt=gt, **args))


def test_no_box_holds_a_column():
    args, gt = _problem(10, 5, 3, 3, [(3, 65)])
    gt["box_labels"][0] += 40.0
    got, grads, _, _ = _compare(args, gt, up=np.array([0, 0, 0, 0, 0, 0, 1], dtype=np.float32))
    assert got[6] == 0.0 and not grads["mask"][0].any()


def test_member_logits_at_minus_thirty_take_the_clamped_mean():
    args, gt = _problem(11, 5, 3, 3, [(2, 65)])
    rows = gt["row_indices"][0]
    off = args["batch_offsets"]
    mem = ref.members(args["levelset_coords"][off[0]:off[1]], gt["box_labels"][0])
    assert mem[0].sum() >= 3
    args["mask_logits"][0][rows[0], mem[0]] = -30.0
    assert mem[0].sum() / (1.0 + np.exp(30.0)) < 1e-5
    _, grads, _, wgrads = _compare(args, gt, up=np.array([0, 0, 0, 0, 0, 0, 1], dtype=np.float32))
    assert grads["mask"][0][rows[0], mem[0]].all()  # tiny, and not flushed
    _compare(args, gt)
    # at -14 the clamp's own term is of the gradient's size, and the gradient array is this one row
    args, gt, mem = clamped_case()
    assert 3 <= mem.sum() <= 12 and 2e-6 <= mem.sum() / (1.0 + np.exp(14.0)) < 1e-5
    _, grads, _, _ = _compare(args, gt, up=LEVELSET_ONLY)
    assert grads["mask"][0][0, mem].all()


def test_fractional_targets_are_taken_as_they_are():
    args, gt = fractional_case()
    assert all(((a > 0) & (a < 1)).any() for a in gt["inst_labels"])
    _compare(args, gt)


def test_zero_upstream_weights_and_partial_requires_grad():
    args, gt = _problem(12, 5, 4, 3, [(3, 65), (2, 63)])
    _compare(args, gt, up=np.array([0, 1, 0, 2, 0, 0, 3], dtype=np.float32))
    got, grads = _run(args, gt, requires={"cls": True, "mask": [1]})
    _, want = ref.losses(gt=gt, upstream=UP, **args)
    assert grads["conf"] is None and grads["box"] is None and grads["mask"][0] is None
    assert ref.close(grads["cls"], want["cls"]) and ref.close(grads["mask"][1], want["mask"][1])
    got, grads = _run(args, gt, requires=("box",))
    assert grads["cls"] is None and grads["conf"] is None and grads["mask"] == [None, None]
    assert ref.close(grads["box"], want["box"])


def test_nan_where_the_reference_has_it():
    args, gt = _problem(13, 5, 4, 3, [(3, 65)])
    args["prob_labels"][:] = 0.0  # a zero weight sum
    got, _ = _run(args, gt, backward=False)
    assert np.isnan(got[1]) and np.isfinite(np.delete(got, 1)).all()
    assert ref.close(got, ref.losses(gt=gt, **args))
    args, gt = _problem(13, 5, 4, 3, [(3, 65)])
    args["box_preds"][0, gt["row_indices"][0][1], 4] = np.nan
    got, _ = _run(args, gt, backward=False)
    assert np.isnan(got[[4, 5]]).all() and np.isfinite(got[[0, 1, 2, 3, 6]]).all()
    assert ref.close(got, ref.losses(gt=gt, **args))


def test_strided_logits_int32_labels_weights_scale_and_another_stream():
    import torch

    args, gt = _problem(14, 6, 5, 3, [(3, 65), (4, 257)])
    wide = [_dev(np.concatenate([a, np.full((a.shape[0], 5), 7.0, np.float32)], 1)) for a in args["mask_logits"]]
    views = [w[:, :a.shape[1]].detach() for w, a in zip(wide, args["mask_logits"])]
    assert not views[0].is_contiguous()
    got, grads, _, _ = _compare(args, gt, logits=views, cls_dtype=torch.int32)
    assert grads["mask"][0].shape == args["mask_logits"][0].shape
    weight = _dev(np.random.default_rng(1).uniform(0.2, 2, 5).astype(np.float32))
    _compare(args, gt, empty_weight=weight, voxel_scale=20)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        there = _run(args, gt)
    stream.synchronize()
    here = _run(args, gt)
    assert np.array_equal(there[0], here[0])
    assert all(np.array_equal(there[1][k], here[1][k]) for k in ("cls", "conf", "box"))
    assert all(np.array_equal(a, b) for a, b in zip(there[1]["mask"], here[1]["mask"]))


def test_two_calls_give_equal_bytes():
    args, gt = _problem(15, 17, 19, 8, [(17, 1025), (5, 255)])
    a, b = _run(args, gt), _run(args, gt)
    assert a[0].tobytes() == b[0].tobytes()
    for k in ("cls", "conf", "box"):
        assert a[1][k].tobytes() == b[1][k].tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[1]["mask"], b[1]["mask"]))


@pytest.mark.parametrize("bad", [-1, "C"])
def test_a_class_label_outside_the_classes_is_refused_by_the_device(bad):
    from gapro_amd._lib import GaproError

    C = 4
    args, gt = _problem(16, 5, C, 3, [(3, 65), (2, 63)])
    gt["cls_labels"][1][1] = C if bad == "C" else -1
    with pytest.raises(GaproError, match="sample 1: a class label outside"):
        _run(args, gt, backward=False)
    got, grads = _run(args, gt, check=False)
    assert np.isnan(got).all()
    assert not grads["cls"].any() and not grads["conf"].any() and not grads["box"].any()
    assert all(g.shape == a.shape and not g.any() for g, a in zip(grads["mask"], args["mask_logits"]))


@pytest.mark.parametrize("name", ref.FIXTURES)
def test_fixture_equals_the_reference(name):
    """Within 4 x ref_dev (max |float32 run - float64 run| of the reference itself) of the reference's float32 values."""
    z, args, gt = ref.fixture(name)
    got, grads = _run(args, gt, up=z["upstream"].astype(np.float32))
    dev = np.abs(got.astype(np.float64) - z["ref_losses32"])
    print("%s: losses: device - reference %s, ref_dev %s" % (name, dev, z["ref_dev_losses"]))
    worst = {}
    for k in ("cls", "conf", "box"):
        worst[k] = np.abs(grads[k].astype(np.float64) - z["ref_g%s32" % k]).max()
    worst["mask"] = 0.0
    for b, rows in enumerate(gt["row_indices"]):
        if rows is None:
            assert grads["mask"][b] is None
            continue
        rest = np.setdiff1d(np.arange(int(z["n_queries"])), rows)
        assert not grads["mask"][b][rest].any()
        worst["mask"] = max(worst["mask"], np.abs(grads["mask"][b][rows].astype(np.float64) - z["ref_gmask32_%d" % b]).max())
    for k, v in worst.items():
        print("%s: grad %s: device - reference %.3g, ref_dev %.3g" % (name, k, v, float(z["ref_dev_%s" % k])))
    assert (dev <= 4 * z["ref_dev_losses"]).all()
    for k, v in worst.items():
        assert v <= 4 * float(z["ref_dev_%s" % k]), k


def test_the_chain_from_get_spp_gt_to_backward():
    import spp_gt_ref
    from gapro_amd import consumer_ops as ops

    z, _ = spp_gt_ref.fixture("two")
    B = int(z["batch_size"])
    assert B == 2
    dc = ops.get_spp_gt(_dev(z["labels"]), _dev(z["spps"]), _dev(z["cls"]), _dev(z["box"]), _dev(z["offsets"]), B)
    assert all(e is not None for e in dc)
    Q, C, F = 12, int(z["cls"].max()) + 2, 3
    sizes = [int(e["mask"].shape[1]) for e in dc]
    rng = np.random.default_rng(21)
    args, _ = _problem(22, Q, C, F, [(1, s) for s in sizes])
    lo = rng.uniform(-8, 8, (B, Q, 3))
    args["box_preds"] = np.concatenate([lo, lo + rng.uniform(0.5, 4, (B, Q, 3))], 2).astype(np.float32)
    args["levelset_coords"] = rng.uniform(-8, 8, args["levelset_coords"].shape).astype(np.float32)
    dev_args = [_dev(args["cls_logits"]), [_dev(a) for a in args["mask_logits"]], _dev(args["conf_logits"]),
                _dev(args["box_preds"])]
    gt, _ = ops.hungarian_match(*dev_args, dc, dup_gt=3)
    for t in [dev_args[0], dev_args[2], dev_args[3]] + dev_args[1]:
        t.requires_grad_()
    out = ops.matched_losses(*dev_args, _dev(args["prob_labels"]), args["batch_offsets"], _dev(args["levelset_feats"]),
                             _dev(args["levelset_coords"]), gt)
    sum(float(u) * out[k] for u, k in zip(UP, ref.NAMES)).backward()
    gt_np = {k: [v if isinstance(v, np.ndarray) else v.cpu().numpy() for v in gt[k]] for k in gt}
    want, wg = ref.losses(gt=gt_np, upstream=UP, **args)
    assert ref.close(np.array([float(out[k].detach()) for k in ref.NAMES], dtype=np.float32), want)
    assert ref.close(dev_args[0].grad.cpu().numpy(), wg["cls"]) and ref.close(dev_args[2].grad.cpu().numpy(), wg["conf"])
    assert ref.close(dev_args[3].grad.cpu().numpy(), wg["box"])
    for b in range(B):
        assert ref.close(dev_args[1][b].grad.cpu().numpy(), wg["mask"][b])
