"""SPFormer's criterion without a device: the restatement tests/spf_loss_ref.py against the reference's float64 run kept
in the fixtures, the as-released BCE against its switch, the integer score filter, the host solver on the fixtures'
cost matrices, every ValueError the Python layer raises before it touches a device, and the bindings."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import spf_loss_ref as ref
from gapro_amd import _lib, consumer_ops
from gapro_amd.consumer_ops import spformer_criterion, spformer_layer_losses, spformer_match  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def restated(args, z, **kw):
    return ref.layer_losses(args["labels"], args["scores"], args["masks"], args["gts"], args["indices"],
                            args["sp_coords"], args["sp_rgb_feats"], args["sp_prob_labels"], args["batch_offsets"],
                            upstream=z["upstream"], **kw)


@pytest.mark.parametrize("name", ref.FIXTURES)
def test_restatement_equals_the_reference_float64_run(name):
    """At least 1000 times more closely than the float32 run does; the ratio found is printed (pytest -s)."""
    z, args = ref.fixture(name)
    table, grads = restated(args, z)
    err, dev = np.abs(table - z["ref_table64"]), z["ref_dev_table"]
    print("%s: float32 run / restatement, by their distance to the float64 run: %.3g"
          % (name, (dev[dev > 0] / np.maximum(err[dev > 0], 1e-300)).min()))
    assert (err * 1000 <= dev).all()
    L1, B, Q = int(z["n_heads"]), int(z["batch_size"]), int(z["n_queries"])
    for h in range(L1):
        for k in ("labels", "scores"):
            want = z["ref_g%s64_%d" % (k, h)]
            assert np.abs(grads[k][h].reshape(want.shape) - want).max() * 1000 <= z["ref_dev_%s" % k][h], (k, h)
        for b in range(B):
            rows = args["indices"][h][b][0]
            if args["gts"][b] is None:
                assert grads["masks"][h][b] is None and len(rows) == 0
                continue
            assert not grads["masks"][h][b][np.setdiff1d(np.arange(Q), rows)].any()
            assert np.abs(grads["masks"][h][b][rows] - z["ref_gmasks64_%d_%d" % (h, b)]).max() * 1000 \
                <= z["ref_dev_masks"][h]


def test_fixtures_cover_what_they_are_there_for():
    heads, skipped, none_kept, counts = set(), 0, 0, []
    for name in ref.FIXTURES:
        z, args = ref.fixture(name)
        assert os.path.getsize(os.path.join(ref.GOLDEN, "spf_losses_%s.npz" % name)) <= 1024 * 1024
        heads.add(int(z["n_heads"]))
        off = args["batch_offsets"]
        for b, g in enumerate(args["gts"]):
            skipped += g is None
            if g is None:
                continue
            rows, cols = args["indices"][-1][b]
            x, t = args["masks"][-1][b][rows], g[1][cols].astype(np.float64)
            inter = ((x >= 0) * t).sum(1)
            none_kept += not ref.iou_kept(inter, (x >= 0).sum(1) + t.sum(1) - inter).any()
            counts += ref.members(args["sp_coords"][off[b]:off[b + 1]], g[2]).sum(1).tolist()
    assert {1, 3} <= heads and skipped >= 1 and none_kept >= 1 and min(counts) < 100 <= max(counts)


@pytest.mark.parametrize("name", ref.FIXTURES)
def test_released_bce_is_the_plain_mean_and_the_switches_change_what_they_name(name):
    z, args = ref.fixture(name)
    table, _ = restated(args, z)
    weighted, _ = restated(args, z, weighted_bce=True)
    divided, _ = restated(args, z, dice_div_main=True)
    col = ref.NAMES.index("mask_bce_loss")
    assert (np.abs(table[:, col] - z["ref_table64"][:, col]) * 1000 <= z["ref_dev_table"][:, col]).all()
    assert (np.abs(weighted[:, col] - z["ref_table64"][:, col]) > 1000 * z["ref_dev_table"][:, col]).all()
    other = [k for k in range(5) if k != col]
    assert np.array_equal(weighted[:, other], table[:, other])
    B, dice = int(z["batch_size"]), ref.NAMES.index("mask_dice_loss")
    assert np.allclose(divided[-1, dice] * B, table[-1, dice], rtol=1e-14) and B > 1
    assert np.array_equal(divided[:-1], table[:-1]) and np.array_equal(np.delete(divided, dice, 1), np.delete(table, dice, 1))


def test_integer_score_filter_is_the_float32_expression_for_every_pair():
    """iou > 0.5 as the reference forms it in float32 (and in float64), against 2 inter > union, union <= 4096."""
    union = np.arange(0, 4097)[None, :]
    inter = np.arange(0, 4097)[:, None]
    ok = inter <= union
    want = ref.iou_kept(inter, union)
    f32 = inter.astype(np.float32) / (union.astype(np.float32) + np.float32(1e-6)) > np.float32(0.5)
    f64 = inter.astype(np.float64) / (union.astype(np.float64) + 1e-6) > 0.5
    assert np.array_equal(f32[ok], np.broadcast_to(want, ok.shape)[ok])
    assert np.array_equal(f64[ok], np.broadcast_to(want, ok.shape)[ok])


def test_the_clamped_case_separates_a_gradient_without_the_clamps_own_term():
    """tests/test_spf_losses_gpu.py's case at its own tolerance."""
    from loss_ref import close, without_clamp_term
    from test_spf_losses_gpu import LEVELSET_ONLY, clamped_case

    p, mem = clamped_case()
    assert 3 <= mem.sum() <= 12
    _, grads = ref.layer_losses(p["labels"], p["scores"], p["masks"], p["gts"], p["indices"], p["sp_coords"],
                                p["sp_rgb_feats"], p["sp_prob_labels"], upstream=LEVELSET_ONLY, min_points=3)
    want = grads["masks"][0][0]
    assert want[0, mem].all() and close(want.astype(np.float32), want)
    k_ls = 1.0 / (1.0 + 1e-4) / mem.sum()
    wrong = without_clamp_term(want[0], p["masks"][0][0][0], mem, p["sp_rgb_feats"], k_ls)
    print("without the term: an error of %.3g" % np.abs(wrong - want[0]).max())
    with pytest.raises(AssertionError, match="max error"):
        close(wrong[None, :].astype(np.float32), want)


@pytest.mark.parametrize("name", ref.FIXTURES)
def test_host_solver_reproduces_every_fixture_assignment(name):
    z, args = ref.fixture(name)
    for h, head in enumerate(args["indices"]):
        for b, (rows, cols) in enumerate(head):
            if args["gts"][b] is None:
                continue
            cost = ref.cost_matrix(args["labels"][h][b], args["masks"][h][b], args["gts"][b][0], args["gts"][b][1])
            r, c = consumer_ops.linear_sum_assignment(cost.astype(np.float32))
            assert sorted(zip(r.tolist(), c.tolist())) == sorted(zip(rows.tolist(), cols.tolist())), (h, b)


# ---- the Python layer's refusals ----------------------------------------------------------------------------------------
def problem(L1=2, B=2, Q=4, C=5, S=(6, 3), n=(2, 1), F=3):
    rng = np.random.default_rng(3)
    t = lambda *shape: torch.from_numpy(rng.normal(0, 1, shape).astype(np.float32))  # noqa: E731
    labels = [t(B, Q, C) for _ in range(L1)]
    scores = [t(B, Q, 1) for _ in range(L1)]
    masks = [[t(Q, S[b]) for b in range(B)] for _ in range(L1)]
    insts = [{"gt_labels": torch.arange(n[b]) % (C - 1), "gt_spmasks": (t(n[b], S[b]) > 0).float(),
              "gt_boxes": t(n[b], 6)} for b in range(B)]
    indices = [[(np.arange(n[b]), np.arange(n[b])) for b in range(B)] for _ in range(L1)]
    N = sum(S)
    return {"pred_labels": labels, "pred_scores": scores, "pred_masks": masks, "insts": insts, "indices": indices,
            "sp_coords": t(N, 3), "sp_rgb_feats": t(N, F), "sp_prob_labels": t(N).abs(), "batch_offsets": [0, S[0], N]}


def refused(call, text, **change):
    args = problem()
    kw = {}
    for k, v in change.items():
        (args if k in args else kw)[k] = v(args[k]) if callable(v) and k in args else v
    with pytest.raises(ValueError, match=text):
        call(args, kw)


def losses_call(args, kw):
    return spformer_layer_losses(**args, **kw)


def match_call(args, kw):
    return spformer_match(args["pred_labels"], args["pred_masks"], args["insts"], **kw)


def edit(path, value):
    """A copy of a nested list with the entry at ``path`` replaced."""
    def go(seq):
        def at(v, p):
            if not p:
                return value(v) if callable(value) else value
            v = dict(v) if isinstance(v, dict) else list(v)
            v[p[0]] = at(v[p[0]], p[1:])
            return v
        return at(seq, path)
    return go


def test_layer_losses_refuse_before_a_device_is_touched():
    r = lambda text, **change: refused(losses_call, text, **change)  # noqa: E731
    r("insts must be a non-empty list", insts=[])
    r("sample 1: an object or dict with gt_labels", insts=edit([1], 5))
    r("gt_spmasks must be", insts=edit([0, "gt_spmasks"], lambda m: m[:1]))
    r("gt_spmasks must be", insts=edit([0, "gt_spmasks"], lambda m: m.double()))
    r("gt_labels must be an int32 or int64", insts=edit([0, "gt_labels"], lambda v: v.float()))
    r("an earlier sample's", insts=edit([1, "gt_labels"], lambda v: v.int()))
    r("gt_boxes must be a float32", insts=edit([0, "gt_boxes"], lambda v: v[:, :5]))
    r("pred_labels must be a tensor or a non-empty list", pred_labels=[])
    r("pred_masks must follow pred_labels", pred_masks=lambda m: m[:1])
    r("pred_scores must follow pred_labels", pred_scores=lambda m: m[:1])
    r("pred_scores is missing", pred_scores=None)
    r("pred_labels must be a non-empty float32", pred_labels=edit([0], lambda z: z.double()))
    r("head 1: pred_labels must be a float32", pred_labels=edit([1], lambda z: z[:, :3]))
    r("a class beside", pred_labels=lambda zs: [z[:, :, :1] for z in zs])
    r("pred_masks must be a list of 2 tensors", pred_masks=edit([1], lambda m: m[:1]))
    r("pred_masks must be a float32", pred_masks=edit([1, 0], lambda x: x[:3]))
    r("one column per superpoint", pred_masks=edit([1, 0], lambda x: x[:, :5]))
    r("pred_scores must be a float32 tensor of shape", pred_scores=edit([0], lambda s: s[:, :, 0:0]))
    r("indices must hold, per head", indices=lambda v: v[:1])
    r("a \\(rows, cols\\) pair", indices=edit([0, 0], (np.arange(2), np.arange(1))))
    r("a \\(rows, cols\\) pair", indices=edit([0, 0], (np.arange(2.0), np.arange(2))))
    r("no matched pair for a sample with instances", indices=edit([0, 0], ([], [])))
    r("rows must be distinct and inside \\[0, 4\\)", indices=edit([0, 0], (np.array([1, 1]), np.arange(2))))
    r("rows must be distinct and inside \\[0, 4\\)", indices=edit([0, 0], (np.array([1, 4]), np.arange(2))))
    r("a column outside \\[0, 2\\)", indices=edit([0, 0], (np.arange(2), np.array([0, 2]))))
    r("sp_prob_labels must be a non-empty float32", sp_prob_labels=lambda v: v[:0])
    r("sp_rgb_feats must be a float32", sp_rgb_feats=lambda v: v[:-1])
    r("9 level-set features; 1 to 8", sp_rgb_feats=lambda v: torch.zeros(9, 9))
    r("0 level-set features; 1 to 8", sp_rgb_feats=lambda v: torch.zeros(9, 0))
    r("sp_coords must be a float32", sp_coords=lambda v: v[:, :2])
    r("batch_offsets must hold batch_size \\+ 1 integers", batch_offsets=[0, 5, 9])
    r("batch_offsets must hold batch_size \\+ 1 integers", batch_offsets=[0, 6])
    r("batch_offsets must be integers", batch_offsets=[0, 6.5, 9])
    r("the samples have 10 columns", batch_offsets=[1, 7, 10])
    r("non_object_weight must be a finite number", non_object_weight=float("nan"))
    r("min_points must be a positive int", min_points=0)
    r("num_class=18", num_class=18)
    r("weighted_bce must be a bool", weighted_bce=1)
    r("dice_div_main must be a bool", dice_div_main="no")
    r("check must be a bool", check=None)
    many = problem(L1=1, B=1, n=(1,), S=(2,))
    many["pred_labels"] = [many["pred_labels"][0][:1]] * 1025
    with pytest.raises(ValueError, match="heads \\* samples beyond 1024"):
        spformer_layer_losses(**{**many, "pred_scores": many["pred_scores"] * 1025, "pred_masks": many["pred_masks"] * 1025})
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # everything passed: the one refusal of host tensors
        spformer_layer_losses(**problem())


def test_a_skipped_sample_takes_no_pairs_and_an_object_is_read_like_a_dict():
    class Inst:
        def __init__(self, d):
            self.gt_labels, self.gt_spmasks, self.gt_boxes = d["gt_labels"], d["gt_spmasks"], d["gt_boxes"]

        def __len__(self):
            return len(self.gt_labels)

    args = problem(n=(2, 0))
    args["insts"] = [Inst(d) for d in args["insts"]]
    with pytest.raises(ValueError, match="matched pairs for a sample without an instance"):
        spformer_layer_losses(**{**args, "indices": edit([0, 1], (np.arange(1), np.arange(1)))(args["indices"])})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spformer_layer_losses(**args)
    single = {k: (v[0] if k in ("pred_labels", "pred_scores", "pred_masks", "indices") else v) for k, v in args.items()}
    single["batch_offsets"] = torch.tensor(args["batch_offsets"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spformer_layer_losses(**single)
    every = problem(n=(0, 0))
    assert [[tuple(len(v) for v in pair) for pair in head] for head in match_call(every, {})] == [[(0, 0)] * 2] * 2


def test_match_refuses_before_a_device_is_touched():
    r = lambda text, **change: refused(match_call, text, **change)  # noqa: E731
    r("insts must be a non-empty list", insts=())
    r("pred_masks must follow pred_labels", pred_masks=lambda m: m[:1])
    r("one column per superpoint", pred_masks=edit([0, 1], lambda x: x[:, :2]))
    for bad in ((1, 1), (1, 1, -1), (1, float("inf"), 1), "abc", None):
        r("cost_weight must be three finite, non-negative numbers", cost_weight=bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        match_call(problem(), {})


def test_criterion_refuses_before_a_device_is_touched():
    args = problem()
    N = int(args["sp_prob_labels"].shape[0])
    pred = {"labels": args["pred_labels"][1], "scores": args["pred_scores"][1], "masks": args["pred_masks"][1],
            "sp_coords": args["sp_coords"], "sp_rgb_feats": args["sp_rgb_feats"],
            "batch_offsets": args["batch_offsets"], "sp_prob_labels": args["sp_prob_labels"],
            "sp_mu_labels": torch.zeros(N), "sp_var_labels": torch.ones(N), "sp_mu_preds": torch.zeros(N),
            "sp_logvar_preds": torch.zeros(N),
            "aux_outputs": [{"labels": args["pred_labels"][0], "scores": args["pred_scores"][0],
                             "masks": args["pred_masks"][0]}]}
    with pytest.raises(ValueError, match="pred must be a dict"):
        spformer_criterion([], args["insts"])
    for k in consumer_ops._SPF_PRED_KEYS:
        with pytest.raises(ValueError, match="pred lacks %r" % k):
            spformer_criterion({key: v for key, v in pred.items() if key != k}, args["insts"])
    with pytest.raises(ValueError, match="aux_outputs must be a list of dicts"):
        spformer_criterion({**pred, "aux_outputs": [{"labels": 1}]}, args["insts"])
    for bad in ((1, 1, 1, 1), (1, 1, 1, 1, float("nan")), None, "wxyz."):
        with pytest.raises(ValueError, match="loss_weight must be five finite numbers"):
            spformer_criterion(pred, args["insts"], loss_weight=bad)
    with pytest.raises(ValueError, match="num_class must be a positive int"):
        spformer_criterion(pred, args["insts"], num_class=0)
    with pytest.raises(ValueError, match="as_floats must be a bool"):
        spformer_criterion(pred, args["insts"], as_floats=1)
    with pytest.raises(ValueError, match="num_class=18"):  # what the composed calls refuse, still before a device
        spformer_criterion(pred, args["insts"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spformer_criterion(pred, args["insts"], num_class=4)


# ---- the bindings -----------------------------------------------------------------------------------------------------
def test_symbols_structs_and_exports():
    lib = _lib.load()
    for n in ("gapro_spf_loss_workspace_bytes", "gapro_spf_loss_forward", "gapro_spf_loss_backward"):
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    text = open(os.path.join(ROOT, "include", "gapro_hip.h")).read()
    assert int(re.search(r"#define GAPRO_SPF_LOSS_N (\d+)", text).group(1)) == _lib.SPF_LOSS_N == len(ref.NAMES)
    assert int(re.search(r"#define GAPRO_SPF_WEIGHTED_BCE (\d+)", text).group(1)) == _lib.SPF_WEIGHTED_BCE
    assert int(re.search(r"#define GAPRO_SPF_DICE_DIV_MAIN (\d+)", text).group(1)) == _lib.SPF_DICE_DIV_MAIN
    assert C.sizeof(_lib.SpfLossTask) == 7 * 8 + 4 * 4 + 2 * 8 and C.sizeof(_lib.SpfLossDims) == 8 * 4 + 8
    assert consumer_ops.SPF_LOSS_NAMES == ref.NAMES
    import gapro_amd
    for n in ("spformer_match", "spformer_layer_losses", "spformer_criterion"):
        assert n in gapro_amd.__all__ and getattr(gapro_amd, n) is getattr(consumer_ops, n)


def test_workspace_bytes_and_the_library_bounds():
    lib = _lib.load()
    assert lib.gapro_spf_loss_workspace_bytes(7, 10, 400, 0) > 0  # a batch of skipped samples is legitimate
    small, large = lib.gapro_spf_loss_workspace_bytes(1, 1, 1, 1), lib.gapro_spf_loss_workspace_bytes(7, 10, 400, 700)
    assert 0 < small < large and small % 256 == 0 and large % 256 == 0
    for bad in ((0, 1, 1, 0), (1, 0, 1, 0), (1, 1, 0, 0), (1, 1, 1, 2), (1, 1, 1, -1), (2, 1024, 1, 0), (1, 1025, 1, 0)):
        assert lib.gapro_spf_loss_workspace_bytes(*bad) == 0, bad
