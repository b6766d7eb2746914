"""ISBNet's dynamic-convolution mask head on the device (gapro_amd/csrc/dyco_head.hip) against the NumPy restatement.

The kernels' tiles: a wave takes 16 points and a workgroup of four waves 64; the forward and the by-query backward run
a workgroup per (sample, query), the by-point backward a workgroup per 64 points of a sample.  The shapes of
tests/dyco_cases.py cross each of those edges.  The bound is the project's standing one: one float32 ulp of the value
plus 1e-9 times the array's largest magnitude, for the logits and for every gradient."""
import glob
import os

import numpy as np
import pytest
import torch

import dyco_cases as cases
import dyco_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dyco_*.npz")))


def _ops():
    from gapro_amd import consumer_ops
    return consumer_ops


def _tensors(case, grad=cases.GRAD_KEYS):
    out = {}
    for k in cases.KEYS:
        out[k] = torch.from_numpy(case[k]).to(DEV)
        if k in grad:
            out[k].requires_grad_()
    return out


def _run(case, grad=cases.GRAD_KEYS):
    """(logits, gradients) of the device for a case, as NumPy."""
    t = _tensors(case, grad)
    logits = _ops().dynamic_mask_head(*[t[k] for k in cases.KEYS], case["off"])
    live = [(y, torch.from_numpy(g).to(DEV)) for y, g in zip(logits, case["grads"]) if y is not None]
    if live and grad:
        torch.autograd.backward([y for y, _ in live], [g for _, g in live])
    grads = {k: t[k].grad.cpu().numpy() for k in grad if t[k].grad is not None}
    return [None if y is None else y.detach().cpu().numpy() for y in logits], grads


def _check(case, what):
    want_y, want_g = cases.reference(case)
    got_y, got_g = _run(case)
    Q = case["controllers"].shape[1]
    for b, (g, w) in enumerate(zip(got_y, want_y)):
        assert (g is None) == (w is None), (what, b)
        if w is not None:
            assert g.shape == (Q, case["off"][b + 1] - case["off"][b])
            cases.assert_close(g, w, "%s: logits of sample %d" % (what, b))
    for k in cases.GRAD_KEYS:
        cases.assert_close(got_g[k], want_g[k], "%s: gradient of %s" % (what, k))
    assert not got_g["controllers"][:, :, -1].any(), "b3's gradient column must be exact zeros"
    return got_y, got_g


@pytest.mark.parametrize("C", [32, 16])
@pytest.mark.parametrize("name", sorted(cases.SHAPES))
def test_logits_and_gradients_at_the_kernel_edges(name, C):
    Q, sizes, lead, tail = cases.SHAPES[name]
    case = cases.make_case(100 + C + len(name), C, Q, sizes, lead, tail)
    _, got_g = _check(case, "%s C=%d" % (name, C))
    lo, hi = case["off"][0], case["off"][-1]
    for k in ("mask_features", "box_preds"):  # the points that no sample owns: written, as zeros
        assert not got_g[k][:lo].any() and not got_g[k][hi:].any()
    for b, n in enumerate(sizes):
        if n == 0:
            assert not got_g["controllers"][b].any() and not got_g["queries_box_preds"][b].any()


@pytest.mark.parametrize("C", [32, 16])
def test_inputs_of_magnitude_1e4(C):
    _check(cases.make_case(7, C, 3, [21, 40], scale=1e4), "1e4 C=%d" % C)


@pytest.mark.parametrize("C", [32, 16])
def test_an_all_zero_controller_gives_exact_zeros(C):
    case = cases.make_case(8, C, 3, [19, 70])
    case["controllers"][:] = 0.0
    got_y, got_g = _run(case)
    assert all(not y.any() for y in got_y)
    assert all(not got_g[k].any() for k in cases.GRAD_KEYS)


@pytest.mark.parametrize("C", [32, 16])
def test_equal_box_dimensions_give_exact_zero_box_gradients(C):
    case = cases.make_case(9, C, 1, [1])
    dims = np.array([0.5, 0.25, 0.75], dtype=np.float32)  # exact in float32, and so are the sums below
    case["box_preds"][0] = np.concatenate([[1.0, 2.0, 1.5], np.array([1.0, 2.0, 1.5], dtype=np.float32) + dims])
    case["queries_box_preds"][0, 0] = np.concatenate([[0.5, 1.0, 2.0], np.array([0.5, 1.0, 2.0], dtype=np.float32) + dims])
    assert np.array_equal(case["box_preds"][0, 3:] - case["box_preds"][0, :3],
                          case["queries_box_preds"][0, 0, 3:] - case["queries_box_preds"][0, 0, :3])
    assert case["controllers"][0, 0, 3 * C:6 * C].all(), "W1's box rows are not zero"
    _, got_g = _check(case, "equal box dimensions C=%d" % C)
    assert not got_g["box_preds"].any() and not got_g["queries_box_preds"].any()
    assert got_g["controllers"][0, 0, :3 * C].any()


def test_subsets_of_the_gradients_equal_the_full_backward_and_two_calls_agree():
    case = cases.make_case(10, 32, 5, [37, 0, 70], lead=1)
    y0, full = _run(case)
    y1, again = _run(case)
    assert all((a is None and b is None) or a.tobytes() == b.tobytes() for a, b in zip(y0, y1))
    assert all(full[k].tobytes() == again[k].tobytes() for k in cases.GRAD_KEYS)
    for subset in (("controllers",), ("queries_box_preds",), ("mask_features",), ("box_preds",),
                   ("controllers", "box_preds"), ("mask_features", "queries_box_preds")):
        _, part = _run(case, subset)
        assert sorted(part) == sorted(subset)
        for k in subset:
            assert part[k].tobytes() == full[k].tobytes(), (subset, k)


@pytest.mark.parametrize("C", [32, 16])
def test_a_batch_equals_each_sample_alone(C):
    case = cases.make_case(11, C, 4, [50, 0, 17, 81], lead=2, tail=3)
    y, g = _run(case)
    off = case["off"]
    for b in range(4):
        lo, hi = off[b], off[b + 1]
        one = {k: case[k][b:b + 1] if k in ("controllers", "queries_locs", "queries_box_preds") else case[k][lo:hi]
               for k in cases.KEYS}
        one["off"], one["grads"] = [0, hi - lo], [case["grads"][b]]
        if hi == lo:
            assert y[b] is None
            continue
        y1, g1 = _run(one)
        assert y1[0].tobytes() == y[b].tobytes()
        assert g1["controllers"].tobytes() == g["controllers"][b:b + 1].tobytes()
        assert g1["queries_box_preds"].tobytes() == g["queries_box_preds"][b:b + 1].tobytes()
        assert g1["mask_features"].tobytes() == g["mask_features"][lo:hi].tobytes()
        assert g1["box_preds"].tobytes() == g["box_preds"][lo:hi].tobytes()


def test_mask_heads_forward_half_inputs_and_the_trailing_axis():
    ops = _ops()
    C, Q, N = 32, 6, 45
    case = cases.make_case(12, C, Q, [N])
    t = _tensors(case, ())
    W1, W2, W3, b1, b2, b3 = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV).requires_grad_()
                              for a in dyco_ref.split_params(case["controllers"][0], C))
    y = ops.mask_heads_forward(t["mask_features"][:, :, None], [W1, W2, W3[:, :, None]], [b1, b2, b3[:, None]], Q,
                               t["locs_float"], t["box_preds"], t["queries_locs"][0], t["queries_box_preds"][0])
    want_y, want_g = cases.reference(case)
    cases.assert_close(y.detach().cpu().numpy(), want_y[0], "mask_heads_forward")
    y.backward(torch.from_numpy(case["grads"][0]).to(DEV))
    cases.assert_close(W1.grad.cpu().numpy().reshape(Q, -1), want_g["controllers"][0][:, :(C + 6) * C],
                       "mask_heads_forward: gradient of the first weights")
    assert not b3.grad.any()
    # half inputs are cast to float32 and the output is float32
    half = {k: v.half() for k, v in t.items()}
    out = ops.dynamic_mask_head(*[half[k] for k in cases.KEYS], case["off"])[0]
    cast = dict(case, **{k: half[k].float().cpu().numpy() for k in cases.KEYS})
    assert out.dtype == torch.float32
    cases.assert_close(out.cpu().numpy(), cases.reference(cast)[0][0], "half inputs")


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_against_the_reference_fixtures(path):
    """Within 4 x the fixture's own ref_dev: the deviation of the reference's float32 run from its float64 run."""
    z = np.load(path)
    case = {k: z[k] for k in cases.KEYS}
    N = int(z["mask_features"].shape[0])
    case["off"], case["grads"] = [0, N], [z["upstream"]]
    got_y, got_g = _run(case)
    pairs = [("logits", got_y[0])] + [("grad_" + k, got_g[k]) for k in cases.GRAD_KEYS]
    for name, got in pairs:
        want = z[name + "_f64"].reshape(got.shape)
        err = float(np.abs(got.astype(np.float64) - want).max())
        print("%s: error %.3e, ref_dev %.3e" % (name, err, float(z["ref_dev_" + name])))
        assert err <= 4 * float(z["ref_dev_" + name]), name


def test_fixtures_exist():
    assert len(GOLDEN) == 3


def test_the_logits_feed_the_matcher_and_the_losses_and_backward_reaches_the_controllers():
    ops = _ops()
    C, Q, sizes, n_classes = 16, 5, [20, 0, 33], 4
    case = cases.make_case(13, C, Q, sizes)
    rng = np.random.default_rng(14)
    t = _tensors(case, ("controllers",))
    logits = ops.dynamic_mask_head(*[t[k] for k in cases.KEYS], case["off"])
    dev = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dt)
    dc = [None if n == 0 else {"mask": dev(rng.integers(0, 2, (3, n))), "cls": dev(rng.integers(0, n_classes, 3), torch.int64),
                               "box": dev(np.concatenate([rng.uniform(0, 1, (3, 3)), rng.uniform(2, 3, (3, 3))], 1))}
          for n in sizes]
    B, N = len(sizes), sum(sizes)
    cls_logits, conf_logits = dev(rng.normal(0, 1, (B, Q, n_classes + 1))), dev(rng.normal(0, 1, (B, Q)))
    gt, _ = ops.hungarian_match(cls_logits, logits, conf_logits, t["queries_box_preds"], dc)
    out = ops.matched_losses(cls_logits, logits, conf_logits, t["queries_box_preds"], dev(rng.uniform(0, 1, N)),
                             case["off"], dev(rng.normal(0, 1, (N, 3))), t["locs_float"], gt)
    (out["dice_loss"] + out["bce_loss"]).backward()
    g = t["controllers"].grad
    assert g is not None and torch.isfinite(g).all() and g[0].any() and g[2].any() and not g[1].any()


def test_peak_memory_is_the_outputs_and_the_gradients():
    """Derived, not measured: the call allocates the packed logits and the four gradients and nothing else (the
    workspace is 0 bytes), so the peak over a forward and a backward rises by their bytes, with 1 MB of slack for the
    allocator's rounding.  The reference's x alone would be 64 x 38 x 4096 x 4 = 40 MB."""
    C, Q, N = 32, 64, 4096
    case = cases.make_case(15, C, Q, [N])
    t = _tensors(case)
    up = torch.from_numpy(case["grads"][0]).to(DEV)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    y = _ops().dynamic_mask_head(*[t[k] for k in cases.KEYS], case["off"])[0]
    y.backward(up)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    allowed = 4 * (Q * N + sum(t[k].numel() for k in cases.GRAD_KEYS)) + (1 << 20)
    print("peak rise %d bytes, allowed %d" % (rise, allowed))
    assert rise <= allowed
