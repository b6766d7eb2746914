"""matched_losses without a device: the restatement tests/loss_ref.py against the reference's float64 run kept in the
fixtures, its analytic gradients against central differences, every ValueError the call raises before it touches a
device, and the struct the bindings share with the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import loss_ref
from gapro_amd import _lib, consumer_ops
from gapro_amd.consumer_ops import matched_losses  # noqa: F401  (the module is about this call: without it, nothing here runs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", loss_ref.FIXTURES)
def test_restatement_equals_the_reference_float64_run(name):
    z, args, gt = loss_ref.fixture(name)
    vals, grads = loss_ref.losses(gt=gt, upstream=z["upstream"], **args)
    assert (np.abs(vals - z["ref_losses64"]) * 1000 <= z["ref_dev_losses"]).all()
    for k in ("cls", "conf", "box"):
        assert np.abs(grads[k] - z["ref_g%s64" % k]).max() * 1000 <= float(z["ref_dev_%s" % k]), k
    for b, rows in enumerate(gt["row_indices"]):
        if rows is None:
            assert grads["mask"][b] is None
            continue
        rest = np.setdiff1d(np.arange(int(z["n_queries"])), rows)
        assert not grads["mask"][b][rest].any()
        assert np.abs(grads["mask"][b][rows] - z["ref_gmask64_%d" % b]).max() * 1000 <= float(z["ref_dev_mask"])


def test_fixtures_cover_a_skipped_sample_and_a_box_without_a_column():
    z, args, gt = loss_ref.fixture("wide")
    assert bool(z["is_none"][1]) and gt["row_indices"][1] is None
    z, args, gt = loss_ref.fixture("two")
    off = args["batch_offsets"]
    empty = [(~loss_ref.members(args["levelset_coords"][off[b]:off[b + 1]], gt["box_labels"][b]).any(1)).sum()
             for b in range(2)]
    assert max(empty) >= 1
    for name in loss_ref.FIXTURES:
        assert os.path.getsize(os.path.join(loss_ref.GOLDEN, "losses_%s.npz" % name)) <= 300 * 1024


def small_problem(seed=5, Q=3, S=7, n=2, C=4, F=2, clamp_row=False):
    """One sample, off every kink; with ``clamp_row`` the members of row 0 sit at -14 (A = 5e-6), so max(A, 1e-5) is active and
    its own d mu / d v carries weight."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 2, (Q, S))
    x[np.abs(x) < 0.1] += 0.3
    rows = rng.permutation(Q)[:n]
    box = np.concatenate([rng.uniform(-1, 0, (n, 3)), rng.uniform(1, 2, (n, 3))], 1).astype(np.float32)
    coords = rng.uniform(-0.9, 0.9, (S, 3)).astype(np.float32)
    coords[0] = 5.0  # a column outside every box
    if clamp_row:
        x[rows[0], 1:] = -14.0
    args = {"cls_logits": rng.normal(0, 1, (1, Q, C)), "mask_logits": [x], "conf_logits": rng.normal(0, 1, (1, Q)),
            "box_preds": (box[rng.integers(0, n, Q)] + rng.normal(0, 0.3, (Q, 6)))[None],
            "prob_labels": rng.uniform(0.1, 1, S), "batch_offsets": [0, S], "levelset_feats": rng.uniform(0, 1, (S, F)),
            "levelset_coords": coords}
    gt = {"row_indices": [rows], "inst_labels": [(rng.random((n, S)) < 0.5).astype(np.float64)],
          "cls_labels": [rng.integers(0, C, n)], "box_labels": [box]}
    return args, gt


@pytest.mark.parametrize("clamp_row", [False, True])
def test_analytic_gradients_equal_central_differences(clamp_row):
    """3 queries x 7 columns; the restatement keeps float64 inputs as they are, so a step of 1e-6 is resolved."""
    args, gt = small_problem(clamp_row=clamp_row)
    up = np.array([0.7, 1.3, 0.9, 1.1, 0.6, 1.7, 2.3])
    if clamp_row:
        up = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1e6])  # the level-set term alone: the clamped row's is of the order 1e-6
    _, grads = loss_ref.losses(gt=gt, upstream=up, **args)
    if clamp_row:
        x, rows = args["mask_logits"][0], gt["row_indices"][0]
        assert (1.0 / (1.0 + np.exp(-x[rows[0], 1:]))).sum() < 1e-5
    h = 1e-6
    for key, arr, g in (("cls_logits", args["cls_logits"], grads["cls"]), ("conf_logits", args["conf_logits"], grads["conf"]),
                        ("box_preds", args["box_preds"], grads["box"]), ("mask", args["mask_logits"][0], grads["mask"][0])):
        num = np.zeros(arr.shape)
        for idx in np.ndindex(arr.shape):
            keep = arr[idx]
            arr[idx] = keep + h
            hi = float(up @ loss_ref.losses(gt=gt, **args))
            arr[idx] = keep - h
            lo = float(up @ loss_ref.losses(gt=gt, **args))
            arr[idx] = keep
            num[idx] = (hi - lo) / (2 * h)
        scale = max(np.abs(g).max(), 1e-12)
        assert np.abs(num - g.reshape(arr.shape)).max() <= 1e-6 * scale + 1e-8, key
        assert np.abs(g).max() > 0 or (clamp_row and key != "mask"), key


def _fails_close(got, want):
    with pytest.raises(AssertionError, match="max error"):
        loss_ref.close(np.asarray(got).astype(np.float32), want)


@pytest.mark.parametrize("binarise", [lambda t: t == 1, lambda t: t != 0], ids=["eq1", "ne0"])
def test_the_fractional_case_separates_a_walk_that_binarises(binarise):
    """tests/test_losses_gpu.py's case at its own tolerance: with the targets made 0 / 1 either way, the losses that read
    them and every sample's mask gradients leave `close`."""
    from test_losses_gpu import UP, fractional_case

    args, gt = fractional_case()
    want, wgrads = loss_ref.losses(gt=gt, upstream=UP, **args)
    wrong = {**gt, "inst_labels": [binarise(t).astype(np.float32) for t in gt["inst_labels"]]}
    got, grads = loss_ref.losses(gt=wrong, upstream=UP, **args)
    for k in ("dice_loss", "bce_loss", "iou_loss"):
        i = loss_ref.NAMES.index(k)
        print("%s: %.3g of the value" % (k, abs(got[i] - want[i]) / abs(want[i])))
        _fails_close(got[i:i + 1], want[i:i + 1])
    for g, w in zip(grads["mask"], wgrads["mask"]):
        print("mask gradient: %.3g of the largest magnitude" % (np.abs(g - w).max() / np.abs(w).max()))
        _fails_close(g, w)


def test_the_clamped_case_separates_a_gradient_without_the_clamps_own_term():
    from test_losses_gpu import LEVELSET_ONLY, clamped_case

    args, gt, mem = clamped_case()
    assert 3 <= mem.sum() <= 12
    _, wgrads = loss_ref.losses(gt=gt, upstream=LEVELSET_ONLY, **args)
    want = wgrads["mask"][0]
    assert loss_ref.close(want.astype(np.float32), want)
    k_ls = 1.0 / (1.0 + 1e-4) / mem.sum()
    wrong = loss_ref.without_clamp_term(want[0], args["mask_logits"][0][0], mem, args["levelset_feats"], k_ls)
    print("without the term: %.3g of the largest magnitude" % (np.abs(wrong - want[0]).max() / np.abs(want).max()))
    _fails_close(wrong[None, :], want)


def _torch_problem(Q=5, S=9, n=2, C=4, F=3, B=2):
    rng = np.random.default_rng(11)
    t = lambda a, d=torch.float32: torch.as_tensor(np.asarray(a)).to(d)  # noqa: E731
    N = B * S
    args = [t(rng.normal(0, 1, (B, Q, C))), [t(rng.normal(0, 1, (Q, S))) for _ in range(B)], t(rng.normal(0, 1, (B, Q))),
            t(rng.normal(0, 1, (B, Q, 6))), t(rng.uniform(0.1, 1, N)), [S * b for b in range(B + 1)],
            t(rng.uniform(0, 1, (N, F))), t(rng.uniform(-1, 1, (N, 3)))]
    gt = {"row_indices": [np.array([1, 3]) for _ in range(B)],
          "inst_labels": [t(rng.random((n, S)) < 0.5) for _ in range(B)],
          "cls_labels": [t(rng.integers(0, C, n), torch.int64) for _ in range(B)],
          "box_labels": [t(rng.uniform(-1, 1, (n, 6))) for _ in range(B)]}
    return args, gt


def _raises(match, args, gt, **kw):
    with pytest.raises(ValueError, match=match):
        consumer_ops.matched_losses(*args, gt, **kw)


def test_every_refusal_before_a_device_is_touched():
    """CPU tensors throughout: a call that got past its checks would raise RuntimeError (no CPU path), not ValueError."""
    def fresh():
        return _torch_problem()

    args, gt = fresh()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        consumer_ops.matched_losses(*args, gt)

    def case(match, edit, **kw):
        args, gt = fresh()
        edit(args, gt)
        _raises(match, args, gt, **kw)

    case("cls_logits must be", lambda a, g: a.__setitem__(0, a[0].double()))
    case("cls_logits must be", lambda a, g: a.__setitem__(0, a[0][0]))
    case("conf_logits must be", lambda a, g: a.__setitem__(2, a[2][:, :4]))
    case("box_preds must be", lambda a, g: a.__setitem__(3, a[3][..., :5]))
    case("mask_logits must be a list", lambda a, g: a.__setitem__(1, a[1][:1]))
    case("gt_dict must hold", lambda a, g: g.pop("box_labels"))
    case("gt_dict must hold", lambda a, g: g.__setitem__("cls_labels", g["cls_labels"][:1]))
    case("prob_labels must be", lambda a, g: a.__setitem__(4, a[4].double()))
    case("levelset_feats must be", lambda a, g: a.__setitem__(6, a[6][:-1]))
    case("level-set features; 1 to 8", lambda a, g: a.__setitem__(6, torch.zeros(18, 9)))
    case("level-set features; 1 to 8", lambda a, g: a.__setitem__(6, torch.zeros(18, 0)))
    case("levelset_coords must be", lambda a, g: a.__setitem__(7, a[7][:, :2]))
    case("empty_weight must be", lambda a, g: None, empty_weight=torch.ones(5))
    case("empty_weight must be", lambda a, g: None, empty_weight=torch.ones(4, dtype=torch.float64))
    case("voxel_scale must be a finite", lambda a, g: None, voxel_scale=float("nan"))
    case("voxel_scale must be a finite", lambda a, g: None, voxel_scale=float("inf"))
    case("voxel_scale must be a finite", lambda a, g: None, voxel_scale="50")
    case("batch offsets for batch_size", lambda a, g: a.__setitem__(5, [0, 9]))
    case("must not decrease", lambda a, g: a.__setitem__(5, [9, 0, 9]))
    case("must not decrease", lambda a, g: a.__setitem__(5, [0, 9, 19]))
    case("must not decrease", lambda a, g: a.__setitem__(5, [-1, 8, 17]))
    case("host sequence of integers", lambda a, g: a.__setitem__(5, [0, 9.5, 18]))
    case("row_indices is empty", lambda a, g: g["row_indices"].__setitem__(0, np.array([], dtype=np.int64)))
    case("row_indices must be a 1-D integer", lambda a, g: g["row_indices"].__setitem__(0, np.array([1.0, 3.0])))
    case("row_indices must be a 1-D integer", lambda a, g: g["row_indices"].__setitem__(0, [1, 3]))
    case(r"a row index outside \[0, 5\)", lambda a, g: g["row_indices"].__setitem__(1, np.array([1, 5])))
    case(r"a row index outside \[0, 5\)", lambda a, g: g["row_indices"].__setitem__(1, np.array([-1, 2])))
    case("listed twice", lambda a, g: g["row_indices"].__setitem__(0, np.array([3, 3])))
    case("mask_logits is", lambda a, g: a[1].__setitem__(0, a[1][0][:, :8]))       # S_b against the offsets
    case("mask_logits is", lambda a, g: a[1].__setitem__(0, a[1][0][:4]))
    case("mask_logits must be a float32", lambda a, g: a[1].__setitem__(1, a[1][1].double()))
    case("inst_labels must be", lambda a, g: g["inst_labels"].__setitem__(0, g["inst_labels"][0][:, :8]))
    case("inst_labels must be", lambda a, g: g["inst_labels"].__setitem__(0, g["inst_labels"][0][:1]))
    case("cls_labels must be", lambda a, g: g["cls_labels"].__setitem__(0, g["cls_labels"][0].float()))
    case("an earlier sample's", lambda a, g: g["cls_labels"].__setitem__(1, g["cls_labels"][1].int()))
    case("box_labels must be", lambda a, g: g["box_labels"].__setitem__(1, g["box_labels"][1][:, :5]))
    case("one device is expected", lambda a, g: a.__setitem__(2, a[2].to("meta")))
    case("row_indices must be on the host", lambda a, g: g["row_indices"].__setitem__(0, torch.tensor([1, 3], device="meta")))
    case("batch_offsets must be on the host", lambda a, g: a.__setitem__(5, torch.tensor([0, 9, 18], device="meta")))


def test_call_forms_the_checks_accept_and_the_all_skipped_batch():
    args, gt = _torch_problem()
    gt["row_indices"] = [torch.tensor([1, 3], dtype=torch.int32), None]      # a CPU tensor; a skipped sample
    args[5] = np.array([0, 9, 18])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        consumer_ops.matched_losses(*args, gt)
    args[1] = [None, args[1][1]]                                             # every sample skipped: zeros, nothing runs
    out = consumer_ops.matched_losses(*args, gt)
    assert list(out) == list(consumer_ops.LOSS_NAMES) + ["kl_loss"]
    assert all(v.shape == () and v.dtype == torch.float32 and float(v) == 0.0 and not v.requires_grad
               for v in out.values())


def test_struct_and_constants_follow_the_header():
    assert C.sizeof(_lib.MatchLossTask) == 5 * 8 + 2 * 4 + 2 * 8
    text = open(os.path.join(ROOT, "include", "gapro_hip.h")).read()
    assert int(re.search(r"#define GAPRO_MATCH_LOSS_N (\d+)", text).group(1)) == _lib.MATCH_LOSS_N == len(loss_ref.NAMES)
    assert int(re.search(r"#define GAPRO_MATCH_LOSS_MAX_FEATS (\d+)", text).group(1)) == _lib.MATCH_LOSS_MAX_FEATS
    body = re.search(r"typedef struct \{([^}]*)\} gapro_match_loss_task;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"\b([a-z_0-9]+)\s*(?:,|$)", decl.strip())]
    assert names == [f[0] for f in _lib.MatchLossTask._fields_]
    assert tuple(consumer_ops.LOSS_NAMES) == loss_ref.NAMES
    lib = _lib.load()
    assert lib.gapro_match_loss_workspace_bytes(0, 4, 1) == 0 and lib.gapro_match_loss_workspace_bytes(2, 4, 9) == 0
    assert lib.gapro_match_loss_workspace_bytes(2, 4, 3) % 256 == 0 and lib.gapro_match_loss_workspace_bytes(2, 4, 3) > 0
