"""The dynamic-convolution mask head without a GPU: the NumPy restatement (tests/dyco_ref.py) against the reference's
fixtures and against torch's float64 autograd, every wrong convention shown to fail, and the wrapper's refusals."""
import glob
import os

import numpy as np
import pytest
import torch

import dyco_cases as cases
import dyco_ref

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dyco_*.npz")))
NAMES = ("logits", "grad_controllers", "grad_mask_features", "grad_box_preds", "grad_queries_box_preds")


def _one(case):
    """The arguments of dyco_ref.forward / backward for a case of one sample."""
    return [case[k][0] if case[k].ndim == 3 else case[k] for k in cases.KEYS]


def _restatement(case, variant=None):
    args = _one(case)
    return dict(zip(NAMES, (dyco_ref.forward(*args, variant=variant),) +
                    dyco_ref.backward(*args, case["grads"][0], variant=variant)))


def _torch_statement(case):
    """The definition of include/gapro_hip.h written with torch einsums in float64, and autograd's gradients."""
    t = {k: torch.from_numpy(np.asarray(a, dtype=np.float64)) for k, a in zip(cases.KEYS, _one(case))}
    for k in cases.GRAD_KEYS:
        t[k].requires_grad_()
    th, f, qb, pb = t["controllers"], t["mask_features"], t["queries_box_preds"], t["box_preds"]
    Q, C = th.shape[0], f.shape[1]
    H = C // 2
    W1, W2, W3, b1, b2, _ = torch.split(th, [(C + 6) * C, C * H, H, C, H, 1], dim=1)
    rel = t["queries_locs"][:, None, :] - t["locs_float"][None, :, :]
    d = (qb[:, 3:] - qb[:, :3])[:, None, :] - (pb[:, 3:] - pb[:, :3])[None, :, :]
    x = torch.cat([rel, d.abs(), f[None].expand(Q, -1, -1)], dim=2)
    h1 = torch.relu(torch.einsum("qna,qaj->qnj", x, W1.reshape(Q, C + 6, C)) + b1[:, None, :])
    h2 = torch.relu(torch.einsum("qnj,qjk->qnk", h1, W2.reshape(Q, C, H)) + b2[:, None, :])
    y = torch.einsum("qnk,qk->qn", h2, W3)
    y.backward(torch.from_numpy(case["grads"][0].astype(np.float64)))
    out = {"logits": y.detach().numpy()}
    out.update({"grad_" + k: t[k].grad.numpy() for k in cases.GRAD_KEYS})
    return out


def _rel_err(a, b):
    return float(np.abs(a - b).max()) / max(float(np.abs(b).max()), 1e-300)


def test_fixtures_exist():
    assert len(GOLDEN) == 3


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_the_restatement_equals_the_reference_in_float64(path):
    z = np.load(path)
    assert os.path.getsize(path) < 100 * 1024
    case = {k: z[k] for k in cases.KEYS}
    case["grads"] = [z["upstream"]]
    got = _restatement(case)
    for k in NAMES:
        want = z[k + "_f64"].reshape(got[k].shape)
        assert want.dtype == np.float64 and _rel_err(got[k], want) <= 1e-12, k
        assert float(z["ref_dev_" + k]) > 0.0


@pytest.mark.parametrize("C", [32, 16])
def test_the_restatement_equals_torchs_float64_autograd(C):
    case = cases.make_case(31 + C, C, 4, [29])
    got, want = _restatement(case), _torch_statement(case)
    for k in NAMES:
        assert _rel_err(got[k], want[k]) <= 1e-12, k
    assert not got["grad_controllers"][:, -1].any()


def _kink_case(which):
    """A case with pre-activations of exactly 0 in the first layer (W1 and b1 zero; the second layer's bias keeps
    dh1 alive) or with every box-dimension difference exactly 0."""
    C, Q, N = 16, 2, 5
    case = cases.make_case(41, C, Q, [N])
    if which == "relu":
        case["controllers"][:, :, :(C + 6) * C] = 0.0
        ob1 = (C + 6) * C + C * (C // 2) + C // 2
        case["controllers"][:, :, ob1:ob1 + C] = 0.0
        case["controllers"][:, :, ob1 + C:ob1 + C + C // 2] = 1.0  # b2 > 0: the second layer is active
    else:
        dims = np.array([0.5, 0.25, 0.75], dtype=np.float32)
        for boxes in (case["box_preds"], case["queries_box_preds"][0]):
            boxes[:, :3] = np.round(boxes[:, :3] * 4) / 4
            boxes[:, 3:] = boxes[:, :3] + dims
    return case


@pytest.mark.parametrize("variant", dyco_ref.VARIANTS)
def test_each_wrong_convention_fails(variant):
    if variant in ("relu_one_at_zero", "sign_one_at_zero"):
        case = _kink_case("relu" if variant.startswith("relu") else "sign")
        keys = ("grad_controllers",) if variant.startswith("relu") else ("grad_box_preds", "grad_queries_box_preds")
    else:
        case, keys = cases.make_case(42, 16, 3, [11]), ("logits",)
    want, right, wrong = _torch_statement(case), _restatement(case), _restatement(case, variant)
    for k in NAMES:
        assert _rel_err(right[k], want[k]) <= 1e-12, k
    if variant == "min_minus_max":
        # Both box dimensions negated cancel under the abs: the same function, shown here rather than assumed.  The
        # convention can only go wrong on one side, which "query_min_minus_max" below catches.
        assert all(np.array_equal(wrong[k], right[k]) for k in NAMES)
        return
    for k in keys:
        scale = max(float(np.abs(want[k]).max()), 1.0)
        assert float(np.abs(wrong[k] - want[k]).max()) > 1e-3 * scale, (variant, k)


def test_a_box_dimension_taken_as_min_minus_max_on_one_side_fails():
    case = cases.make_case(43, 16, 3, [11])
    flipped = dict(case)
    flipped["queries_box_preds"] = np.concatenate([case["queries_box_preds"][..., 3:],
                                                   case["queries_box_preds"][..., :3]], axis=-1)
    right, wrong = _restatement(case), _restatement(flipped)
    assert _rel_err(wrong["logits"], right["logits"]) > 1e-3


def test_the_kink_cases_hold_exact_zeros():
    relu, sign = _kink_case("relu"), _kink_case("sign")
    _, _, _, p1, _ = dyco_ref.forward(*_one(relu), full=True)
    assert not p1.any()
    _, _, d, _, _ = dyco_ref.forward(*_one(sign), full=True)
    assert not d.any()
    got = _restatement(sign)
    assert not got["grad_box_preds"].any() and not got["grad_queries_box_preds"].any()


def test_param_count():
    from gapro_amd import dyco_param_count
    assert dyco_param_count(32) == 1793 == dyco_ref.param_count(32)
    assert dyco_param_count(16) == 513 == dyco_ref.param_count(16)
    for bad in (0, 8, 24, 48, 64, -32, 32.0, "32", None, True):
        with pytest.raises(ValueError):
            dyco_param_count(bad)


def _cpu_args(C=16, Q=3, sizes=(4, 0, 6)):
    case = cases.make_case(44, C, Q, list(sizes))
    return [torch.from_numpy(case[k]) for k in cases.KEYS] + [case["off"]]


def test_every_refusal_before_a_device_is_touched():
    from gapro_amd import consumer_ops as ops

    with pytest.raises(RuntimeError, match="no CPU fallback"):  # host tensors that pass every check
        ops.dynamic_mask_head(*_cpu_args())

    def refused(match, edit, **kw):
        args = _cpu_args()
        edit(args)
        with pytest.raises(ValueError, match=match):
            ops.dynamic_mask_head(*args, **kw)

    def put(i, value):
        return lambda a: a.__setitem__(i, value(a[i]) if callable(value) else value)

    refused("controllers", put(0, lambda t: t[0]))
    refused("controllers", put(0, lambda t: t.double()))
    refused("controllers", put(0, lambda t: t.numpy()))
    refused("parameters", put(0, lambda t: t[:, :, :-1]))
    refused("parameters", put(0, lambda t: torch.zeros(3, 3, 1793)))
    refused("a sample and a query", put(0, lambda t: t[:, :0]))
    refused("at most 64", lambda a: (a.__setitem__(0, torch.zeros(65, 3, 513)), a.__setitem__(4, torch.zeros(65, 3, 3)),
                                     a.__setitem__(5, torch.zeros(65, 3, 6)), a.__setitem__(6, [0] * 66)))
    refused("mask_features", put(1, lambda t: t.long()))
    refused("mask_features", put(1, lambda t: t[:, :, None, None]))
    refused("channels", put(1, lambda t: t[:, :8]))
    refused("locs_float", put(2, lambda t: t[:-1]))
    refused("locs_float", put(2, lambda t: t[:, :2]))
    refused("box_preds", put(3, lambda t: t[:, :5]))
    refused("box_preds", put(3, lambda t: t.int()))
    refused("queries_locs", put(4, lambda t: t[:, :-1]))
    refused("queries_box_preds", put(5, lambda t: t[:-1]))
    refused("batch_size", put(6, [0, 4, 10]))
    refused("must not decrease", put(6, [0, 6, 4, 10]))
    refused("must not decrease", put(6, [0, 4, 4, 11]))
    refused("must not decrease", put(6, [-1, 4, 4, 10]))
    refused("host sequence of integers", put(6, [0, 4.5, 4, 10]))
    refused("host sequence of integers", put(6, None))
    refused("check", lambda a: None, check=1)
    # the offsets as a NumPy array or a CPU tensor, half inputs and the trailing axis pass the checks
    for edit in (put(6, lambda o: np.array(o)), put(6, lambda o: torch.tensor(o)), put(1, lambda t: t[:, :, None]),
                 put(0, lambda t: t.half()), put(3, lambda t: t.bfloat16())):
        args = _cpu_args()
        edit(args)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.dynamic_mask_head(*args)


def test_mask_heads_forward_refusals():
    from gapro_amd import consumer_ops as ops
    C, Q, N = 16, 3, 7
    case = cases.make_case(45, C, Q, [N])
    W1, W2, W3, b1, b2, b3 = (torch.from_numpy(a.astype(np.float32)) for a in dyco_ref.split_params(case["controllers"][0], C))
    t = {k: torch.from_numpy(case[k]) for k in cases.KEYS}
    good = [t["mask_features"][:, :, None], [W1, W2, W3[:, :, None]], [b1, b2, b3[:, None]], Q, t["locs_float"],
            t["box_preds"], t["queries_locs"][0], t["queries_box_preds"][0]]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mask_heads_forward(*good)
    for i, bad in ((1, [W1, W2]), (2, None), (3, Q + 1), (3, 0), (6, t["queries_locs"]), (1, [W1[:, :-1], W2, W3])):
        args = list(good)
        args[i] = bad
        with pytest.raises(ValueError):
            ops.mask_heads_forward(*args)
