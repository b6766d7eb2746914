"""point_wise_losses and criterion_losses without a device: the restatement tests/point_loss_ref.py against the
reference's float64 run kept in the fixtures, its analytic gradients against central differences, the n = 0 and
all-ignored conventions (and what torch's own backward does there), every ValueError the two calls raise before they
touch a device, criterion_losses' branches on ``model_outputs=None``, and the constants the bindings share with the
header."""
import os
import re

import numpy as np
import pytest
import torch

import point_loss_ref as ref
from gapro_amd import _lib, consumer_ops
from gapro_amd.consumer_ops import criterion_losses, point_wise_losses  # noqa: F401  (the module is about these calls)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IGNORE = -100


@pytest.mark.parametrize("name", ref.FIXTURES)
def test_restatement_equals_the_reference_float64_run(name):
    z, args = ref.fixture(name)
    vals, grads = ref.losses(upstream=z["upstream"], **args)
    assert (np.abs(vals - z["ref_losses64"]) * 1000 <= z["ref_dev_losses"]).all()
    for k in ("scores", "corners", "conf"):
        assert np.abs(grads[k] - z["ref_g%s64" % k]).max() * 1000 <= float(z["ref_dev_%s" % k]), k


def test_fixtures_are_what_they_are_meant_to_be():
    shapes = {"mixed": (700, 20), "weighted": (300, 13), "nopos": (130, 20)}
    for name in ref.FIXTURES:
        z, args = ref.fixture(name)
        assert args["semantic_scores"].shape == shapes[name]
        assert os.path.getsize(os.path.join(ref.GOLDEN, "point_losses_%s.npz" % name)) <= 300 * 1024
        pos, ign = (args["instance_labels"] != IGNORE).mean(), (args["semantic_labels"] == IGNORE).mean()
        assert (pos == 0.0) if name == "nopos" else (0.5 < pos < 0.7)
        assert 0.01 < ign < 0.1
        assert (args["semantic_weight"] is not None) == (name == "weighted")
    z, _ = ref.fixture("nopos")
    assert not z["ref_losses32"][1:].any() and not z["ref_gcorners32"].any() and not z["ref_gconf32"].any()
    z = np.load(os.path.join(ref.GOLDEN, "criterion_two.npz"))
    assert z["ref_values32"].shape == z["ref_values64"].shape == z["ref_dev"].shape == (12,)
    assert z["pw_semantic_scores"].shape == (400, 20)


def small_problem(seed=3, N=5, C=4, weighted=True):
    """Float64 inputs off every kink: one point of no instance, one ignored semantic label, a predicted box with
    hi < lo on one axis (an active clamp)."""
    rng = np.random.default_rng(seed)
    lab = np.concatenate([-rng.uniform(0.5, 1.5, (N, 3)), rng.uniform(0.5, 1.5, (N, 3))], 1)
    pred = lab + rng.choice([-1.0, 1.0], (N, 6)) * rng.uniform(0.1, 0.4, (N, 6))
    pred[1, 3] = pred[1, 0] - 0.3
    sem, inst = rng.integers(0, C, N), rng.integers(0, 3, N)
    sem[2], inst[0] = IGNORE, IGNORE
    args = {"semantic_scores": rng.normal(0, 1.5, (N, C)), "corners_offset": pred, "box_conf": rng.uniform(0, 1, N),
            "semantic_labels": sem, "instance_labels": inst, "corners_offset_labels": lab,
            "coords_float": rng.uniform(-3, 3, (N, 3))}
    return args, (rng.uniform(0.3, 2, C).astype(np.float32) if weighted else None)


@pytest.mark.parametrize("weighted", [False, True])
def test_analytic_gradients_equal_central_differences(weighted):
    args, weight = small_problem(weighted=weighted)
    vals, grads = ref.losses(semantic_weight=weight, voxel_scale=20, upstream=ref.UPSTREAM, **args)
    assert np.isfinite(vals).all()
    h = 1e-6
    for key, name in (("semantic_scores", "scores"), ("corners_offset", "corners"), ("box_conf", "conf")):
        # the confidence loss has no gradient through the IoU, which a difference quotient by the corners would see
        up = ref.UPSTREAM * (np.array([1, 1, 1, 0]) if name == "corners" else 1)
        g = ref.losses(semantic_weight=weight, voxel_scale=20, upstream=up, **args)[1][name]
        assert np.array_equal(g, grads[name])
        arr = args[key]
        num = np.zeros(arr.shape)
        for idx in np.ndindex(arr.shape):
            keep = arr[idx]
            arr[idx] = keep + h
            hi = float(up @ ref.losses(semantic_weight=weight, voxel_scale=20, **args))
            arr[idx] = keep - h
            lo = float(up @ ref.losses(semantic_weight=weight, voxel_scale=20, **args))
            arr[idx] = keep
            num[idx] = (hi - lo) / (2 * h)
        assert np.abs(num - g).max() <= 1e-6 * np.abs(g).max() + 1e-8, key
        assert np.abs(g).max() > 0, key
    assert not grads["scores"][2].any() and not grads["corners"][0].any() and grads["conf"][0] == 0.0


def _torch_cal_point_wise(args, weight=None, voxel_scale=50):
    """The torch statement of cal_point_wise_loss (criterion.py:136-191), for the conventions below."""
    import torch.nn.functional as F

    t = {k: torch.as_tensor(v) for k, v in args.items()}
    z, c, conf = (t[k].clone().requires_grad_() for k in ("semantic_scores", "corners_offset", "box_conf"))
    sem = F.cross_entropy(z, t["semantic_labels"], ignore_index=IGNORE, weight=weight)
    pos = t["instance_labels"] != IGNORE
    if pos.sum() == 0:
        rest = [0 * c.sum(), 0 * conf.sum(), 0 * conf.sum()]
    else:
        n = pos.sum()
        l1 = F.l1_loss(c[pos], t["corners_offset_labels"][pos], reduction="sum") / n
        a = c[pos] + t["coords_float"][pos].repeat(1, 2)
        b = t["corners_offset_labels"][pos] + t["coords_float"][pos].repeat(1, 2)
        inter = torch.prod(torch.clamp(torch.min(a[:, 3:], b[:, 3:]) - torch.max(a[:, :3], b[:, :3]), min=0.0), -1)
        va = torch.prod(torch.clamp(a[:, 3:] - a[:, :3], min=0.0), -1)
        vb = torch.prod(torch.clamp(b[:, 3:] - b[:, :3], min=0.0), -1)
        union = va + vb - inter
        iou = inter / (union + 1e-6)
        bound = torch.prod(torch.clamp(torch.max(a[:, 3:], b[:, 3:]) - torch.min(a[:, :3], b[:, :3]), min=0.0), -1)
        giou = iou - (bound - union) / (bound + 1e-6)
        rest = [l1 * voxel_scale / 50.0, torch.sum(1 - giou) / n, F.mse_loss(conf[pos], iou.detach(), reduction="sum") / n]
    return [sem] + rest, (z, c, conf)


def test_the_restatement_equals_torch_in_float64_on_an_active_clamp():
    args, _ = small_problem(weighted=False)
    out, (z, c, conf) = _torch_cal_point_wise(args)
    sum(float(u) * v for u, v in zip(ref.UPSTREAM, out)).backward()
    vals, grads = ref.losses(upstream=ref.UPSTREAM, **args)
    assert np.allclose(vals, [float(v.detach()) for v in out], rtol=1e-13, atol=0)
    for g, t in ((grads["scores"], z), (grads["corners"], c), (grads["conf"], conf)):
        assert np.allclose(g, t.grad.numpy(), rtol=1e-12, atol=1e-15)


def test_every_semantic_label_ignored_nan_loss_and_torch_backward_gives_zeros():
    """What the kernel copies: F.cross_entropy is NaN and autograd's gradient of the scores is ZEROS, not NaN."""
    args, _ = small_problem(weighted=False)
    args["semantic_labels"][:] = IGNORE
    for dtype in (np.float32, np.float64):
        cast = {k: v.astype(dtype) if v.dtype.kind == "f" else v for k, v in args.items()}
        out, (z, _, _) = _torch_cal_point_wise(cast)
        assert torch.isnan(out[0])
        out[0].backward()
        assert not z.grad.any() and not torch.isnan(z.grad).any()
    vals, grads = ref.losses(upstream=ref.UPSTREAM, **args)
    assert np.isnan(vals[0]) and np.isfinite(vals[1:]).all() and not grads["scores"].any()
    assert grads["corners"].any() and grads["conf"].any()


def test_no_positive_point_exact_zeros_also_for_non_finite_inputs():
    """The one deviation: the reference's 0 * corners_offset.sum() is NaN for a non-finite input, the rule's 0 is not."""
    args, _ = small_problem(weighted=False)
    args["instance_labels"][:] = IGNORE
    vals, grads = ref.losses(upstream=ref.UPSTREAM, **args)
    assert np.isfinite(vals[0]) and not vals[1:].any() and not grads["corners"].any() and not grads["conf"].any()
    args["corners_offset"][1, 2] = np.inf
    out, _ = _torch_cal_point_wise(args)
    assert torch.isnan(out[1]) and float(out[2].detach()) == 0.0
    assert not ref.losses(**args)[1:].any()


def _tensors(N=9, C=5):
    rng = np.random.default_rng(2)
    f = lambda *s: torch.as_tensor(rng.normal(0, 1, s), dtype=torch.float32)  # noqa: E731
    return [f(N, C), f(N, 6), f(N), torch.as_tensor(rng.integers(0, C, N)), torch.as_tensor(rng.integers(0, 3, N)),
            f(N, 6), f(N, 3)]


def test_point_wise_losses_every_refusal_before_a_device_is_touched():
    """CPU tensors throughout: a call that got past its checks would raise RuntimeError (no CPU path), not ValueError."""
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        point_wise_losses(*_tensors())
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # the forms the checks accept
        a = _tensors()
        a[2], a[3], a[0] = a[2][:, None], a[3].int(), torch.zeros(9, 10)[:, ::2]
        point_wise_losses(*a, semantic_weight=[1.0, 2, 3, 4, 5], voxel_scale=20, ignore_label=-1)

    def case(match, edit=lambda a: None, **kw):
        a = _tensors()
        edit(a)
        with pytest.raises(ValueError, match=match):
            point_wise_losses(*a, **kw)

    case("semantic_scores must be", lambda a: a.__setitem__(0, a[0].double()))
    case("semantic_scores must be", lambda a: a.__setitem__(0, a[0][0]))
    case("semantic_scores must be", lambda a: a.__setitem__(0, a[0].numpy()))
    case("classes; 2 to 64", lambda a: a.__setitem__(0, a[0][:, :1]))
    case("classes; 2 to 64", lambda a: a.__setitem__(0, torch.zeros(9, 65)))
    case("corners_offset must be", lambda a: a.__setitem__(1, a[1][:, :5]))
    case("corners_offset must be", lambda a: a.__setitem__(1, a[1][:8]))
    case("corners_offset must be", lambda a: a.__setitem__(1, a[1].double()))
    case("box_conf must be", lambda a: a.__setitem__(2, a[2][:8]))
    case("box_conf must be", lambda a: a.__setitem__(2, a[2][None, :]))
    case("box_conf must be", lambda a: a.__setitem__(2, a[2].half()))
    case("semantic_labels must be", lambda a: a.__setitem__(3, a[3].float()))
    case("semantic_labels must be", lambda a: a.__setitem__(3, a[3][:8]))
    case("instance_labels must be", lambda a: a.__setitem__(4, a[4].to(torch.int16)))
    case("instance_labels must be", lambda a: a.__setitem__(4, a[4][:, None]))
    case("corners_offset_labels must be", lambda a: a.__setitem__(5, a[5][:, :3]))
    case("coords_float must be", lambda a: a.__setitem__(6, a[6][:, :2]))
    case("coords_float must be", lambda a: a.__setitem__(6, a[6].double()))
    case("semantic_weight must be a float32 tensor", semantic_weight=torch.ones(4))
    case("semantic_weight must be a float32 tensor", semantic_weight=torch.ones(5, dtype=torch.float64))
    case("semantic weights for 5 classes", semantic_weight=[1.0] * 6)
    case("semantic_weight must be None", semantic_weight=3.0)
    case("semantic_weight must be None", semantic_weight=["a"] * 5)
    case("ignore_label must be an int", ignore_label=-100.0)
    case("ignore_label must be an int", ignore_label=True)
    case("ignore_label must be an int", ignore_label=2 ** 63)
    case("voxel_scale must be a finite", voxel_scale=float("nan"))
    case("voxel_scale must be a finite", voxel_scale=float("inf"))
    case("voxel_scale must be a finite", voxel_scale="50")
    case("one device is expected", lambda a: a.__setitem__(5, a[5].to("meta")))
    case("one device is expected", lambda a: a.__setitem__(3, a[3].to("meta")))
    case("one device is expected", semantic_weight=torch.ones(5, device="meta"))


def test_no_points_nan_and_three_zeros_without_a_launch():
    a = [t[:0] for t in _tensors()]
    out = point_wise_losses(*a)
    assert list(out) == list(ref.NAMES) == list(consumer_ops.POINT_LOSS_NAMES)
    assert all(v.shape == () and v.dtype == torch.float32 for v in out.values())
    assert np.isnan(float(out["pw_sem_loss"])) and [float(out[k]) for k in ref.NAMES[1:]] == [0.0, 0.0, 0.0]


def _criterion_inputs():
    a = _tensors()
    batch = {"semantic_labels": a[3], "instance_labels": a[4], "coords_float": a[6], "corners_offset_labels": a[5]}
    model = {"semantic_scores": a[0], "corners_offset": a[1], "box_conf": a[2]}
    return batch, model


def test_criterion_losses_placeholder_branch_and_key_order():
    batch, _ = _criterion_inputs()
    for kw in ({}, {"semantic_only": False}, {"semantic_only": False, "trainall": True}):
        out = criterion_losses(batch, None, **kw)
        assert list(out) == ["Placeholder"]
        v = out["Placeholder"]
        assert v.requires_grad and v.is_leaf and v.dtype == torch.float32 and float(v.detach()) == 0.0
        assert v.device == batch["semantic_labels"].device and v.shape == ()
    assert list(consumer_ops.LOSS_WEIGHT) == list(consumer_ops.LOSS_NAMES) + ["kl_loss"]
    assert list(consumer_ops.LOSS_WEIGHT.values()) == [1, 1, 0.5, 0.5, 0.5, 0.5, 0.5, 0.1]
    w = consumer_ops._empty_weight_of(torch.device("cpu"), 3, 0.1, None)
    assert w.tolist() == pytest.approx([1, 1, 1, 0.1]) and w.dtype == torch.float32
    w = consumer_ops._empty_weight_of(torch.device("cpu"), 3, 0.2, (9.0, 2.0, 3.0, 4.0, 5.0))
    assert w.tolist() == pytest.approx([2, 3, 4, 0.2])  # shifted by label_shift = 1; eos_coef is overwritten at 3 only


def test_criterion_losses_every_refusal_before_a_device_is_touched():
    batch, model = _criterion_inputs()
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # semantic_only: the point-wise call is reached
        criterion_losses(batch, model)

    def case(match, b=batch, m=model, **kw):
        with pytest.raises(ValueError, match=match):
            criterion_losses(b, m, **kw)

    case("batch_inputs must be a dict", b=[1])
    case("model_outputs must be a dict or None", m=[1])
    case("batch_inputs lacks 'semantic_labels'", b={})
    case("batch_inputs lacks 'instance_labels'", b={"semantic_labels": batch["semantic_labels"]}, m=None)
    case("batch_inputs lacks 'coords_float'", b={k: batch[k] for k in ("semantic_labels", "instance_labels")})
    case("model_outputs lacks 'box_conf'", m={k: model[k] for k in ("semantic_scores", "corners_offset")})
    case("model_outputs lacks 'cls_logits'", semantic_only=False)
    case("model_outputs lacks 'cls_logits'", semantic_only=False, trainall=True)
    case("must be tensors", b={**batch, "semantic_labels": [1, 2]})
    case("instance_classes must be a positive int", instance_classes=0)
    case("instance_classes must be a positive int", instance_classes=18.0)
    case("dup_gt must be a positive int", dup_gt=0)
    case("eos_coef must be a finite", eos_coef=float("nan"))
    case("loss_weight must be a dict", loss_weight={"dice_loss": 1})
    case("loss_weight must be a dict", loss_weight={**consumer_ops.LOSS_WEIGHT, "bce_loss": float("inf")})
    case("loss_weight must be a dict", loss_weight=[1] * 8)
    case("semantic_weight must be None or a sequence", semantic_weight=3.0)
    case("semantic weights for 5 classes", semantic_weight=[1.0] * 4)
    case("voxel_scale must be a finite", voxel_scale=float("inf"))
    case("ignore_label must be an int", ignore_label=None)
    case("corners_offset must be", m={**model, "corners_offset": model["corners_offset"][:, :5]})


def test_constants_follow_the_header():
    text = open(os.path.join(ROOT, "include", "gapro_hip.h")).read()
    define = lambda n: int(re.search(r"#define %s (\d+)" % n, text).group(1))  # noqa: E731
    assert define("GAPRO_POINT_LOSS_N") == _lib.POINT_LOSS_N == len(ref.NAMES)
    assert define("GAPRO_POINT_LOSS_MIN_CLASSES") == _lib.POINT_LOSS_MIN_CLASSES
    assert define("GAPRO_POINT_LOSS_MAX_CLASSES") == _lib.POINT_LOSS_MAX_CLASSES
    assert define("GAPRO_POINT_LOSS_RUN") == _lib.POINT_LOSS_RUN and define("GAPRO_POINT_LOSS_FOLD") == _lib.POINT_LOSS_FOLD
    lib = _lib.load()
    for n in ("gapro_point_loss_workspace_bytes", "gapro_point_loss_forward", "gapro_point_loss_backward"):
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    size = lib.gapro_point_loss_workspace_bytes
    assert size(0, 20) == 0 and size(10, 1) == 0 and size(10, 65) == 0 and size(_lib.POINT_LOSS_MAX_POINTS + 1, 20) == 0
    assert size(1, 2) > 0 and size(1, 2) % 256 == 0
    assert size(_lib.POINT_LOSS_RUN + 1, 20) >= 64 + 2 * 64 > size(1, 20) - 256
    import gapro_amd

    for n in ("point_wise_losses", "criterion_losses"):
        assert n in gapro_amd.__all__ and getattr(gapro_amd, n) is getattr(consumer_ops, n)
