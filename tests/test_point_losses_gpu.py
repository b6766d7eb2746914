"""consumer_ops.point_wise_losses and criterion_losses on the MI355X: the four losses and all three gradient arrays
against the NumPy float64 restatement tests/point_loss_ref.py at the kernels' wave, round, run and fold edges, for every
class count that changes the LDS layout, both label types, with and without class weights and on edge data; the other
call forms, repeatability, the device's refusal; the real reference's outputs (tests/golden/point_losses_*.npz,
criterion_two.npz); and criterion_losses against the same composition written out.

Tolerances: device against the restatement loss_ref.close, 1 float32 ulp of the value plus 1e-9 times the array's largest
magnitude; device against a fixture 4 x the fixture's own ref_dev of that loss or gradient array.
"""
import itertools
import os

import numpy as np
import pytest

import point_loss_ref as ref

pytestmark = pytest.mark.gpu

UP = np.array([0.7, 1.3, 0.9, 1.1], dtype=np.float32)
IGNORE = -100
INPUTS = ("scores", "corners", "conf")


def _dev(a, dtype=None):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    return t if dtype is None else t.to(dtype)


def _problem(seed, N, C, p_pos=0.6, p_ignore=0.1):
    """Label corners around the point, predicted corners off them by at least 0.01 on every face."""
    rng = np.random.default_rng(seed)
    lab = np.concatenate([-rng.uniform(0.2, 2.5, (N, 3)), rng.uniform(0.2, 2.5, (N, 3))], 1)
    pred = lab + rng.choice([-1.0, 1.0], (N, 6)) * rng.uniform(0.01, 0.6, (N, 6))
    sem = rng.integers(0, C, N)
    sem[rng.random(N) < p_ignore] = IGNORE
    inst = rng.integers(0, 9, N)
    inst[rng.random(N) >= p_pos] = IGNORE
    return {"semantic_scores": rng.normal(0, 2, (N, C)).astype(np.float32), "corners_offset": pred.astype(np.float32),
            "box_conf": rng.uniform(0, 1, N).astype(np.float32), "semantic_labels": sem.astype(np.int64),
            "instance_labels": inst.astype(np.int64), "corners_offset_labels": lab.astype(np.float32),
            "coords_float": rng.uniform(-6, 6, (N, 3)).astype(np.float32)}


def _run(args, up=UP, backward=True, requires=INPUTS, sem_dtype=None, inst_dtype=None, tensors=None, **kw):
    """One call (and its backward): the f32[4] and the gradients as NumPy, ``None`` where none was asked for."""
    import torch
    from gapro_amd import consumer_ops as ops

    t = {k: _dev(args[k]) for k in ref.ARGS}
    t["semantic_labels"] = t["semantic_labels"].to(sem_dtype or torch.int64)
    t["instance_labels"] = t["instance_labels"].to(inst_dtype or torch.int64)
    t.update(tensors or {})
    leaves = {"scores": t["semantic_scores"], "corners": t["corners_offset"], "conf": t["box_conf"]}
    for k, leaf in leaves.items():
        leaf.requires_grad_(k in requires)
    if isinstance(kw.get("semantic_weight"), np.ndarray):
        kw["semantic_weight"] = _dev(kw["semantic_weight"])
    out = ops.point_wise_losses(*[t[k] for k in ref.ARGS], **kw)
    assert list(out) == list(ref.NAMES)
    vec = torch.stack([out[k] for k in ref.NAMES])
    assert vec.is_cuda and vec.dtype == torch.float32
    grads = None
    if backward and requires:
        (vec * _dev(np.asarray(up, dtype=np.float32))).sum().backward()
        grads = {k: None if leaf.grad is None else leaf.grad.cpu().numpy() for k, leaf in leaves.items()}
        for k, leaf in leaves.items():
            assert grads[k] is None or grads[k].shape == tuple(leaf.shape), k
    return vec.detach().cpu().numpy(), grads


def _compare(args, up=UP, **kw):
    got, grads = _run(args, up=up, **kw)
    want, wgrads = ref.losses(upstream=up, **args, **{k: v for k, v in kw.items()
                                                      if k in ("semantic_weight", "ignore_label", "voxel_scale")})
    assert ref.close(got, want)
    for k in INPUTS:
        assert ref.close(grads[k].reshape(wgrads[k].shape), wgrads[k]), k
    return got, grads, want, wgrads


def _constants():
    from gapro_amd import _lib

    return _lib.POINT_LOSS_RUN, _lib.POINT_LOSS_FOLD


# N on both sides of a wave (64) and of a round of the workgroup (256); C rotates over every class count of the issue
SIZES = [1, 63, 64, 65, 255, 256, 257]
CLASSES = [2, 13, 20, 63, 64]


@pytest.mark.parametrize("k", range(len(SIZES)))
def test_edge_sizes_equal_the_restatement(k):
    import torch

    N, C = SIZES[k], CLASSES[k % len(CLASSES)]
    args = _problem(100 + k, N, C)
    types = [(torch.int64, torch.int64), (torch.int32, torch.int64), (torch.int64, torch.int32),
             (torch.int32, torch.int32)][k % 4]
    weight = np.random.default_rng(k).uniform(0.3, 2, C).astype(np.float32) if k % 2 else None
    _compare(args, sem_dtype=types[0], inst_dtype=types[1], semantic_weight=weight)


@pytest.mark.parametrize("C", CLASSES)
def test_every_class_count_with_and_without_weights(C):
    """Two workgroups and a ragged last wave at every LDS row pitch (C | 1: 3, 13, 21, 63, 65)."""
    run, _ = _constants()
    args = _problem(200 + C, run + 70, C)
    _compare(args)
    _compare(args, semantic_weight=np.random.default_rng(C).uniform(0.3, 2, C).astype(np.float32), voxel_scale=20)


def test_one_point_more_than_a_workgroups_run():
    run, _ = _constants()
    args = _problem(31, run + 1, 20)
    got, grads, _, _ = _compare(args)
    args["instance_labels"][:run] = IGNORE  # the last workgroup's single point carries every box term
    args["instance_labels"][run] = 3
    got, grads, _, _ = _compare(args)
    assert grads["corners"][run].any() and not grads["corners"][:run].any()


def test_one_record_more_than_finish_folds_in_a_pass():
    run, fold = _constants()
    N = run * fold + 1
    args = _problem(32, N, 2)
    args["instance_labels"][N - 1], args["semantic_labels"][N - 1] = 4, 1
    got, grads, want, _ = _compare(args)
    less = {k: v[:N - 1] for k, v in args.items()}
    assert (ref.losses(**less) != want).any()  # the last record counts


@pytest.mark.parametrize("case", ["n0", "n1", "nN", "all_ignored"])
def test_counts_at_their_ends(case):
    args = _problem(40, 300, 13)
    if case == "n0":
        args["instance_labels"][:] = IGNORE
    elif case == "n1":
        args["instance_labels"][:] = IGNORE
        args["instance_labels"][257] = 0
    elif case == "nN":
        args["instance_labels"][:] = 2
    else:
        args["semantic_labels"][:] = IGNORE
    got, grads, _, _ = _compare(args)
    if case == "n0":
        assert not got[1:].any() and not grads["corners"].any() and not grads["conf"].any() and np.isfinite(got[0])
        args["corners_offset"][5, 2], args["box_conf"][9] = np.inf, np.nan  # the one deviation: still exact zeros
        got, grads = _run(args)
        assert not got[1:].any() and not grads["corners"].any() and not grads["conf"].any()
    if case == "n1":
        assert np.flatnonzero(grads["conf"]).tolist() == [257]
    if case == "all_ignored":  # NaN, and zeros from the backward, as torch (tests/test_point_losses_cpu.py)
        assert np.isnan(got[0]) and np.isfinite(got[1:]).all() and not grads["scores"].any()


def test_edge_data_equals_the_restatement():
    """Logits of +-100, a predicted box with hi < lo on one axis (an active clamp), exact ties in min / max pairs and
    zero L1 differences."""
    args = _problem(41, 200, 20, p_pos=1.0, p_ignore=0.0)
    z, c, l = args["semantic_scores"], args["corners_offset"], args["corners_offset_labels"]
    z[0, :] = -100.0
    z[0, args["semantic_labels"][0]] = 100.0
    z[1, :] = 100.0
    z[2, :] = -100.0
    z[3, ::2], z[3, 1::2] = 100.0, -100.0
    c[10, 3] = c[10, 0] - 0.5
    c[11, 5] = c[11, 2] - 0.25
    c[20] = l[20]                      # every pair tied, every L1 difference zero
    c[21, 0], c[21, 4] = l[21, 0], l[21, 4]
    args["coords_float"][20:22] = np.array([[0.5, -1.25, 2.0], [4.0, 0.0, -8.0]], dtype=np.float32)  # the adds are exact
    got, grads, _, wgrads = _compare(args)
    assert np.isfinite(got).all() and all(np.isfinite(grads[k]).all() for k in INPUTS)
    assert wgrads["corners"][21, 0] != 0.0 and grads["scores"][1].any()


def test_a_nan_corner_reaches_the_box_terms_and_nothing_else():
    """A NaN in one corners_offset row: by the rule the L1, the GIoU and, through the IoU, the confidence error of that
    point are NaN, so the three losses over P are; the semantic loss and every other point's gradients are not."""
    args = _problem(42, 130, 13, p_pos=1.0)
    args["corners_offset"][70, 4] = np.nan
    got, grads, _, _ = _compare(args)
    assert np.isfinite(got[0]) and np.isnan(got[1:]).all()
    assert np.isfinite(grads["scores"]).all()
    rest = np.delete(np.arange(130), 70)
    assert np.isfinite(grads["corners"][rest]).all() and np.isfinite(grads["conf"][rest]).all()
    assert np.isnan(grads["corners"][70]).any() and np.isnan(grads["conf"][70])


@pytest.mark.parametrize("requires", [s for r in range(4) for s in itertools.combinations(INPUTS, r)])
def test_requires_grad_on_each_subset(requires):
    args = _problem(43, 321, 20)
    got, grads = _run(args, requires=requires)
    want, wgrads = ref.losses(upstream=UP, **args)
    assert ref.close(got, want)
    for k in INPUTS:
        if k in requires:
            assert ref.close(grads[k], wgrads[k]), k
        else:
            assert grads is None or grads[k] is None


def test_box_conf_as_a_column_and_strided_scores():
    import torch

    args = _problem(44, 333, 13)
    want, wgrads = ref.losses(upstream=UP, **args)
    wide = _dev(np.concatenate([args["semantic_scores"], np.full((333, 3), 50.0, np.float32)], 1))
    view = wide[:, :13].detach()
    assert not view.is_contiguous() and view.stride(0) == 16
    got, grads = _run(args, tensors={"semantic_scores": view, "box_conf": _dev(args["box_conf"])[:, None].contiguous()})
    assert ref.close(got, want) and grads["conf"].shape == (333, 1) and grads["scores"].shape == (333, 13)
    for k in INPUTS:
        assert ref.close(grads[k].reshape(wgrads[k].shape), wgrads[k]), k
    every_other = _dev(np.repeat(args["semantic_scores"], 2, axis=1))[:, ::2].detach()  # columns of stride 2: copied
    assert every_other.stride(1) == 2
    got2, grads2 = _run(args, tensors={"semantic_scores": every_other})
    assert got2.tobytes() == got.tobytes() and grads2["scores"].tobytes() == grads["scores"].tobytes()
    assert torch.cuda.is_available()


def test_two_calls_give_equal_bytes():
    run, _ = _constants()
    args = _problem(45, 3 * run + 17, 20)
    a, b = _run(args), _run(args)
    assert a[0].tobytes() == b[0].tobytes()
    for k in INPUTS:
        assert a[1][k].tobytes() == b[1][k].tobytes()


@pytest.mark.parametrize("bad", [-1, "C"])
def test_a_semantic_label_outside_the_classes_is_refused_by_the_device(bad):
    from gapro_amd._lib import GaproError

    run, _ = _constants()
    C = 13
    args = _problem(46, run + 300, C)
    args["semantic_labels"][run + 150] = C if bad == "C" else -1
    args["semantic_labels"][run + 222] = C + 5
    with pytest.raises(GaproError, match="point %d: a semantic label" % (run + 150)):
        _run(args, backward=False)
    got, grads = _run(args, check=False)
    assert np.isnan(got).all()
    assert all(not grads[k].any() for k in INPUTS)
    args["instance_labels"][3] = 10 ** 12  # an instance label is only compared with ignore_label
    args["semantic_labels"][[run + 150, run + 222]] = 0
    _compare(args)


@pytest.mark.parametrize("name", ref.FIXTURES)
def test_fixture_equals_the_reference(name):
    """Within 4 x ref_dev (max |float32 run - float64 run| of the reference itself) of the reference's float32 values."""
    z, args = ref.fixture(name)
    weight = args.pop("semantic_weight")
    got, grads = _run(args, up=z["upstream"].astype(np.float32), semantic_weight=weight)
    dev = np.abs(got.astype(np.float64) - z["ref_losses32"])
    print("%s: losses: device - reference %s, ref_dev %s" % (name, dev, z["ref_dev_losses"]))
    assert (dev <= 4 * z["ref_dev_losses"]).all()
    for k in INPUTS:
        worst = np.abs(grads[k].astype(np.float64) - z["ref_g%s32" % k]).max()
        print("%s: grad %s: device - reference %.3g, ref_dev %.3g" % (name, k, worst, float(z["ref_dev_%s" % k])))
        assert worst <= 4 * float(z["ref_dev_%s" % k]), k


def _criterion_two():
    z = np.load(os.path.join(ref.GOLDEN, "criterion_two.npz"))
    B = int(z["batch_size"])
    batch = {"semantic_labels": _dev(z["pw_semantic_labels"]), "instance_labels": _dev(z["pw_instance_labels"]),
             "coords_float": _dev(z["pw_coords_float"]), "corners_offset_labels": _dev(z["pw_corners_offset_labels"])}
    model = {k: _dev(z["pw_" + k]) for k in ("semantic_scores", "corners_offset", "box_conf")}
    model.update({k: _dev(z[k]) for k in ("cls_logits", "conf_logits", "box_preds", "dc_prob_labels", "dc_rgb_feats",
                                          "dc_coords_float", "dc_mu_labels", "dc_var_labels", "mu_pred", "logvar_pred")})
    model["mask_logits"] = [_dev(z["mask_logits_%d" % b]) for b in range(B)]
    model["dc_inst_mask_arr"] = [{k: _dev(z["%s_%d" % (k, b)]) for k in ("mask", "cls", "box")} for b in range(B)]
    model["dc_batch_offsets"] = z["batch_offsets"].tolist()
    return z, batch, model


KEYS = list(ref.NAMES) + ["dice_loss", "bce_loss", "cls_loss", "iou_loss", "box_loss", "giou_loss", "levelset_loss",
                          "kl_loss"]


def test_criterion_equals_the_reference_and_the_composition_written_out():
    """All twelve values of Criterion.forward (trainall) within 4 x ref_dev; bit for bit what the four calls give."""
    import torch
    from gapro_amd import consumer_ops as ops

    z, batch, model = _criterion_two()
    C = int(z["cls_logits"].shape[2])
    out = ops.criterion_losses(batch, model, instance_classes=C - 1, semantic_only=False, trainall=True)
    assert list(out) == KEYS
    got = np.array([float(out[k]) for k in KEYS])
    dev = np.abs(got - z["ref_values32"].astype(np.float64))
    print("criterion_two: device - reference %s, ref_dev %s" % (dev, z["ref_dev"]))
    assert (dev <= 4 * z["ref_dev"]).all()

    pw = ops.point_wise_losses(model["semantic_scores"], model["corners_offset"], model["box_conf"],
                               batch["semantic_labels"], batch["instance_labels"], batch["corners_offset_labels"],
                               batch["coords_float"])
    gt, _ = ops.hungarian_match(model["cls_logits"], model["mask_logits"], model["conf_logits"], model["box_preds"],
                                model["dc_inst_mask_arr"], dup_gt=4)
    main = ops.matched_losses(model["cls_logits"], model["mask_logits"], model["conf_logits"], model["box_preds"],
                              model["dc_prob_labels"], model["dc_batch_offsets"], model["dc_rgb_feats"],
                              model["dc_coords_float"], gt)
    kl = ops.kl_to_gp_loss(model["mu_pred"], model["logvar_pred"], model["dc_mu_labels"], model["dc_var_labels"],
                           weight=0.1)
    want = [pw[k] * 0.25 for k in ref.NAMES] + [main[k] * w for k, w in list(ops.LOSS_WEIGHT.items())[:7]] + [kl]
    assert torch.stack([out[k] for k in KEYS]).cpu().numpy().tobytes() == torch.stack(want).cpu().numpy().tobytes()

    # the other branches: semantic_only returns the four point-wise values unscaled; neither flag: no point-wise keys;
    # the offsets as a device tensor
    only = ops.criterion_losses(batch, model)
    assert list(only) == list(ref.NAMES) and all(float(only[k]) == float(pw[k]) for k in ref.NAMES)
    model["dc_batch_offsets"] = _dev(z["batch_offsets"])
    rest = ops.criterion_losses(batch, model, instance_classes=C - 1, semantic_only=False)
    assert list(rest) == KEYS[4:] and all(float(rest[k]) == float(out[k]) for k in KEYS[4:])


def test_criterion_backward_reaches_every_prediction():
    from gapro_amd import consumer_ops as ops

    z, batch, model = _criterion_two()
    leaves = [model[k] for k in ("semantic_scores", "corners_offset", "box_conf", "cls_logits", "conf_logits",
                                 "box_preds", "mu_pred", "logvar_pred")] + model["mask_logits"]
    for t in leaves:
        t.requires_grad_()
    out = ops.criterion_losses(batch, model, instance_classes=int(z["cls_logits"].shape[2]) - 1, semantic_only=False,
                               trainall=True)
    sum(out.values()).backward()
    assert all(t.grad is not None and t.grad.shape == t.shape and bool(t.grad.any()) for t in leaves)
    up = np.full(4, 0.25)
    pw = {k: z["pw_" + k] for k in ref.ARGS}
    _, wg = ref.losses(upstream=up, **pw)
    assert ref.close(model["semantic_scores"].grad.cpu().numpy(), wg["scores"])
    assert ref.close(model["corners_offset"].grad.cpu().numpy(), wg["corners"])
    assert ref.close(model["box_conf"].grad.cpu().numpy(), wg["conf"])
