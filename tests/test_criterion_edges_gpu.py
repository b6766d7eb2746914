"""The criterion kernels on the MI355X at their kinks, class and batch edges: every case of
tests/criterion_edge_cases.py through consumer_ops.matched_losses (losses and all four gradient arrays), match_cost /
hungarian_match and point_wise_losses against the NumPy float64 restatements, and criterion_losses' backward against the
restatement of what it composes.  tests/test_criterion_edges_cpu.py holds the restatements to torch's float64 autograd on
the same cases and shows that each kink case tells the right convention from a wrong one.

Tolerances: the project's own, unchanged -- loss_ref.close (1 float32 ulp of the value plus 1e-9 times the array's largest
magnitude, equal NaN patterns) and match_ref.close (1 float32 ulp plus 1e-9); exactly 100000 where the restatement has it
and nowhere else.  The runs and comparisons are those of tests/test_losses_gpu.py, test_match_gpu.py and
test_point_losses_gpu.py.
"""
import functools

import numpy as np
import pytest

import criterion_edge_cases as cases
import loss_ref
import match_ref
import test_losses_gpu as losses_gpu
import test_match_gpu as match_gpu
import test_point_losses_gpu as point_gpu

pytestmark = pytest.mark.gpu

_dev = losses_gpu._dev
_ids = lambda table: [c[0] for c in table]  # noqa: E731


def _compare_case(case, up=cases.UP, **kw):
    """losses_gpu._compare on a case: its class weights and label type go with it."""
    import torch

    if case["empty_weight"] is not None:
        kw["empty_weight"] = _dev(case["empty_weight"])
    return losses_gpu._compare(case["args"], case["gt"], up=up, cls_dtype=getattr(torch, case["cls_dtype"]), **kw)


# ------------------------------------------------------------------------------------------------------ matched_losses
@pytest.mark.parametrize("name,build,key", cases.LOSS_CASES, ids=_ids(cases.LOSS_CASES))
def test_matched_losses_equal_the_restatement(name, build, key):
    assert np.array_equal(cases.UP, losses_gpu.UP)
    case = build(*key)
    got, grads, want, wgrads = _compare_case(case)
    args, gt = case["args"], case["gt"]
    for b, x in enumerate(args["mask_logits"]):  # a skipped sample: no logit gradient, zeros in the other three
        if x is None or gt["row_indices"][b] is None:
            assert grads["mask"][b] is None
            assert not grads["cls"][b].any() and not grads["conf"][b].any() and not grads["box"][b].any()
    if name.startswith("nan_backward"):
        assert np.isnan(got).any() and any(np.isnan(g).any() for g in (grads["box"], grads["mask"][0]))
    else:
        assert np.isfinite(got).all() and np.delete(got[:6], 2).all() and (got[2] != 0.0) == (name != "classes-C1")
        assert all(np.isfinite(g).all() for g in [grads["cls"], grads["conf"], grads["box"]]
                   + [g for g in grads["mask"] if g is not None])


@functools.lru_cache(maxsize=None)
def _kinks_run(term):
    """The kinks case on the device once per upstream: every loss ("all") or one term of the box gradient alone."""
    up = {"all": cases.UP, "l1": np.array([0, 0, 0, 0, 0.6, 0, 0], dtype=np.float32),
          "giou": np.array([0, 0, 0, 0, 0, 1.7, 0], dtype=np.float32)}[term]
    case = cases.kinks()
    got, grads = losses_gpu._run(case["args"], case["gt"], up=up)
    want, wgrads = loss_ref.losses(gt=case["gt"], upstream=up, **case["args"])
    return got, grads, want, wgrads


def _only_row(got, want, q):
    """``want`` with row q taken from ``got``: loss_ref.close on it judges that row alone, at the whole array's bound."""
    out = want.astype(np.float32)
    out[..., q, :] = got[..., q, :]
    return out


@pytest.mark.parametrize("term", ["all", "l1", "giou"])
@pytest.mark.parametrize("row", cases.KINK_ROWS)
def test_each_kink_row_equals_the_restatement(row, term):
    """The gradients of one matched row of the kinks case; with the L1 or the GIoU term alone the kink's share of the
    box gradient is not a small part of a sum."""
    case = cases.kinks()
    q = case["query_of"][row]
    got, grads, want, wgrads = _kinks_run(term)
    assert loss_ref.close(_only_row(grads["box"], wgrads["box"], q), wgrads["box"]), row
    assert loss_ref.close(_only_row(grads["mask"][0], wgrads["mask"][0], q), wgrads["mask"][0]), row
    assert loss_ref.close(_only_row(grads["conf"][..., None], wgrads["conf"][..., None], q), wgrads["conf"][..., None]), row
    assert np.isfinite(grads["box"][0, q]).all() and np.isfinite(grads["mask"][0][q]).all()
    if row.startswith("tie_") and term == "l1":
        k = cases.FACES.index(row[4:])
        assert grads["box"][0, q, k] == 0.0 and np.delete(grads["box"][0, q], k).all()  # sign(0) = 0
    if row == "identical" and term == "l1":
        assert not grads["box"][0, q].any()                                             # exact zeros
    if row == "identical" and term == "giou":  # the share of the two 1e-6: tiny, not zero (the CPU test has the form)
        assert grads["box"][0, q].all() and (np.abs(grads["box"][0, q]) < 1e-6).all()
    if row == "touching" and term == "giou":
        assert grads["box"][0, q, 0] != 0.0                                             # the clamp passes at exactly 0
    if row in ("x_minus_1000", "x_plus_1000") and term == "all":
        assert grads["mask"][0][q].any()


def test_the_level_set_term_alone_on_the_faces_and_the_empty_sigmoid_sum():
    """Upstream weight on the level-set loss only: the membership and the clamped mean carry the whole gradient."""
    up = np.array([0, 0, 0, 0, 0, 0, 2.3], dtype=np.float32)
    for case in (cases.faces(), cases.kinks()):
        got, grads, want, wgrads = _compare_case(case, up=up)
        assert got[6] != 0.0 and grads["mask"][0].any()
    case = cases.faces()
    g = _compare_case(case, up=up)[1]["mask"][0][case["gt"]["row_indices"][0][0]]
    assert g[case["on_face"]].all() and not g[case["off_face"]].any() and not g[[12, 13, 16, 17]].any()


# ------------------------------------------------------------------------------------------ match_cost / hungarian_match
@pytest.mark.parametrize("name,build,key", cases.MATCH_CASES, ids=_ids(cases.MATCH_CASES))
def test_match_cost_equals_the_restatement(name, build, key):
    import torch
    from gapro_amd import consumer_ops as ops

    d = build(*key)
    want = match_gpu._want(d)
    got = ops.match_cost(*match_gpu._args(d, torch.int32 if name.endswith("C200") else None))
    assert match_gpu._check(got, want)
    for b, (g, w) in enumerate(zip(got, want)):  # exactly 100000 where the restatement has it, and nowhere else
        if w is None:
            continue
        big = g.cpu().numpy() == 100000.0
        assert np.array_equal(big, w == 100000.0)
        rows = d["big_rows"][b] if "big_rows" in d else []
        assert np.array_equal(np.flatnonzero(big.all(1)), rows) and big.sum() == len(rows) * w.shape[1]
    if name == "boxes":  # the box term alone, so that a kink pair's GIoU is the whole cell
        only = (0.0, 0.0, 0.0, 0.0, 1.0)
        assert match_gpu._check(ops.match_cost(*match_gpu._args(d), weights=only), match_gpu._want(d, only))
    if name == "class_logits":  # the class term alone: exactly 0 under a -inf target logit
        only = (1.0, 0.0, 0.0, 0.0, 0.0)
        got = ops.match_cost(*match_gpu._args(d), weights=only)
        assert match_gpu._check(got, match_gpu._want(d, only))
        assert not got[0].cpu().numpy()[1, [0, 3]].any()


def test_hungarian_match_on_exact_ties():
    """Two identical queries and two identical instances: equal rows and columns of the cost, equal-cost optima.  The
    solver's choice among them is its own; it is the one linear_sum_assignment makes on the device's cost, it is a valid
    assignment, and on the restatement's cost its total is the brute-force optimum to within the two costs' distance
    (2 n (1 ulp + 1e-9): each of the two assignments is judged on a cost at most 1 ulp + 1e-9 per cell from its own)."""
    from gapro_amd import consumer_ops as ops

    d = cases.match_ties()
    s = d["samples"][0]
    args = match_gpu._args(d)
    c = ops.match_cost(*args)[0].cpu().numpy()
    want = match_gpu._want(d)[0]
    assert match_ref.close(c, want)
    assert c[0].tobytes() == c[1].tobytes() and c[:, 0].tobytes() == c[:, 1].tobytes()
    gt, aux = ops.hungarian_match(*args, dup_gt=2)
    for out, dup in ((gt, 1), (aux, 2)):
        rows, cols = ops.linear_sum_assignment(c, dup)
        assert np.array_equal(out["row_indices"][0], rows)
        assert match_ref.check_assignment(c, rows, cols, dup)
        assert np.array_equal(out["inst_labels"][0].cpu().numpy(), s["mask"][cols])
        assert np.array_equal(out["cls_labels"][0].cpu().numpy(), s["cls"][cols])
        assert np.array_equal(out["box_labels"][0].cpu().numpy(), s["box"][cols])
        slack = 2 * len(rows) * (float(match_ref.ulp32(np.abs(want).max())) + 1e-9)
        best = match_ref.brute_force(want, dup)
        assert best - 1e-12 <= match_ref.total(want, rows, cols) <= best + slack
        assert match_ref.total(c, rows, cols) == pytest.approx(match_ref.brute_force(c, dup), rel=1e-12, abs=1e-12)


# ---------------------------------------------------------------------------------------------------- point_wise_losses
@pytest.mark.parametrize("pair", cases.POINT_PAIRS)
def test_point_wise_pairs_equal_the_restatement(pair):
    """The pair with the five generic points, under every loss and under the L1 and the GIoU term alone."""
    k = cases.POINT_PAIRS.index(pair)
    pick = [k, 3, 4, 5, 6, 7]
    args = {key: v[pick] for key, v in cases.point_pairs().items()}
    for up in (point_gpu.UP, np.array([0, 1.3, 0, 0], dtype=np.float32), np.array([0, 0, 0.9, 0], dtype=np.float32)):
        got, grads, want, wgrads = point_gpu._compare(args, up=up)
        assert np.isfinite(got).all() and all(np.isfinite(grads[key]).all() for key in point_gpu.INPUTS)
    if pair == "identical":  # the last run: the GIoU term alone
        assert grads["corners"][0].all() and (np.abs(grads["corners"][0]) < 1e-6).all()
    if pair == "touching":
        assert grads["corners"][0, 0] != 0.0


# ----------------------------------------------------------------------------------------------------- criterion_losses
def test_criterion_backward_equals_the_restatement_and_the_direct_kl_call():
    """sum(out.values()).backward(): the gradients of the matched losses' four inputs are the restatement's under the
    seven LOSS_WEIGHT values as upstream, the matcher's own gt (dup_gt = 4) and Criterion.empty_weight (ones, 0.1 last);
    those of mu_pred and logvar_pred are, byte for byte, a direct kl_to_gp_loss call's."""
    from gapro_amd import consumer_ops as ops

    z, batch, model = point_gpu._criterion_two()
    B, _, C = z["cls_logits"].shape
    main = [model[k] for k in ("cls_logits", "conf_logits", "box_preds")] + model["mask_logits"]
    for t in main + [model[k] for k in ("semantic_scores", "corners_offset", "box_conf", "mu_pred", "logvar_pred")]:
        t.requires_grad_()
    out = ops.criterion_losses(batch, model, instance_classes=C - 1, semantic_only=False, trainall=True)
    sum(out.values()).backward()

    gt, _ = ops.hungarian_match(model["cls_logits"].detach(), [x.detach() for x in model["mask_logits"]],
                                model["conf_logits"].detach(), model["box_preds"].detach(), model["dc_inst_mask_arr"],
                                dup_gt=4)
    gt_np = {k: [v if v is None or isinstance(v, np.ndarray) else v.cpu().numpy() for v in gt[k]] for k in gt}
    up = np.array([ops.LOSS_WEIGHT[k] for k in loss_ref.NAMES], dtype=np.float32)
    assert up.tolist() == loss_ref.UPSTREAM.tolist()
    weight = loss_ref.default_weight(C)
    assert ops._empty_weight_of(model["cls_logits"].device, C - 1, 0.1, None).cpu().numpy().tobytes() == weight.tobytes()
    args = {"cls_logits": z["cls_logits"], "mask_logits": [z["mask_logits_%d" % b] for b in range(B)],
            "conf_logits": z["conf_logits"], "box_preds": z["box_preds"], "prob_labels": z["dc_prob_labels"],
            "batch_offsets": z["batch_offsets"], "levelset_feats": z["dc_rgb_feats"],
            "levelset_coords": z["dc_coords_float"]}
    want, wg = loss_ref.losses(gt=gt_np, upstream=up, empty_weight=weight, **args)
    got = np.array([float(out[k].detach()) / float(u) for k, u in zip(loss_ref.NAMES, up)])
    assert np.allclose(got, want, rtol=1e-6, atol=0)  # the values: test_criterion_equals_the_reference_... has them
    assert loss_ref.close(model["cls_logits"].grad.cpu().numpy(), wg["cls"])
    assert loss_ref.close(model["conf_logits"].grad.cpu().numpy(), wg["conf"])
    assert loss_ref.close(model["box_preds"].grad.cpu().numpy(), wg["box"])
    for b in range(B):
        assert loss_ref.close(model["mask_logits"][b].grad.cpu().numpy(), wg["mask"][b]), b
    # a wrong LOSS_WEIGHT entry or the default-free weights would show: the restatement under them differs
    for k in range(7):
        other = up.copy()
        other[k] *= 2
        _, og = loss_ref.losses(gt=gt_np, upstream=other, empty_weight=weight, **args)
        with pytest.raises(AssertionError):
            for key in ("cls", "conf", "box"):
                loss_ref.close(model[key + ("_preds" if key == "box" else "_logits")].grad.cpu().numpy(), og[key])
            loss_ref.close(model["mask_logits"][0].grad.cpu().numpy(), og["mask"][0])

    mu, logvar = (_dev(z[k]).requires_grad_() for k in ("mu_pred", "logvar_pred"))
    ops.kl_to_gp_loss(mu, logvar, model["dc_mu_labels"], model["dc_var_labels"],
                      weight=ops.LOSS_WEIGHT["kl_loss"]).backward()
    assert mu.grad.any() and logvar.grad.any()
    assert model["mu_pred"].grad.cpu().numpy().tobytes() == mu.grad.cpu().numpy().tobytes()
    assert model["logvar_pred"].grad.cpu().numpy().tobytes() == logvar.grad.cpu().numpy().tobytes()
