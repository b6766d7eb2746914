"""The sparse convolutions on the device (gapro_amd/csrc/spconv.hip) against the NumPy restatement (tests/spconv_ref.py).

The plans are integers and must equal the restatement's exactly.  The three forwards and all their gradients are float64
sums of the float32 operands rounded once, so the bound is |dev - ref| <= ulp32(ref) + T 2^-52 A with T the number of
terms of the element and A the same sum over |x| |w|, both computed by the restatement: derived, not measured.
Refusals are host-side checks or the plans' status word: nothing here provokes a fault."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import spconv_cases as cases
import spconv_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FNS = {"subm": "subm_conv3d", "down": "sparse_conv3d", "inverse": "sparse_inverse_conv3d"}


def _ops():
    from gapro_amd import consumer_ops
    return consumer_ops


def _plans(coords, shape, B, dtype=torch.int64, check=True):
    c = torch.from_numpy(np.ascontiguousarray(coords)).to(DEV).to(dtype)
    return _ops().subm_plan(c, shape, B, check=check), _ops().downsample_plan(c, shape, B, check=check)


def _layer(layer, plan, x, w, b, g):
    """(y, d feats, d weight, d bias) of one layer on the device, as NumPy (None for an absent bias)."""
    t = [None if a is None else torch.from_numpy(a).to(DEV).requires_grad_() for a in (x, w, b)]
    y = getattr(_ops(), FNS[layer])(t[0], t[1], plan, t[2])
    y.backward(torch.from_numpy(g).to(DEV))
    return (y.detach().cpu().numpy(),) + tuple(None if a is None else a.grad.cpu().numpy() for a in t)


@lru_cache(maxsize=None)
def _device(name):
    """The plans and the three layers of a case, computed once."""
    c = cases.BY_NAME[name]
    sub, down = _plans(c.coords, c.shape, c.batch_size)
    out = {layer: _layer(layer, sub if layer == "subm" else down, *cases.tensors(name, layer))
           for layer in cases.LAYERS}
    return sub, down, out


@lru_cache(maxsize=None)
def _reference(name, layer):
    c = cases.BY_NAME[name]
    x, w, b, g = cases.tensors(name, layer)
    tab, rows_in = ref.layer_tables(layer, c.coords, c.shape)
    dw, db = ref.backward_weight(tab, x, g, w.shape)
    return ref.forward(tab, x, w, b), ref.backward_input(tab, rows_in, g, w), dw, db


def _within(got, want, what):
    value, T, A = want
    assert got.shape == value.shape and got.dtype == np.float32, what
    err, tol = np.abs(got.astype(np.float64) - value), ref.tolerance(value, T, A)
    worst = np.argmax(err - tol) if err.size else 0
    print("%s: largest error %.3e at a bound of %.3e" % (what, err.flat[worst] if err.size else 0.0,
                                                         tol.flat[worst] if err.size else 0.0))
    assert (err <= tol).all(), (what, err.flat[worst], tol.flat[worst])


@pytest.mark.parametrize("name", cases.NAMES)
def test_plans_equal_the_restatement(name):
    c = cases.BY_NAME[name]
    sub, down, _ = _device(name)
    assert (sub.neighbours.cpu().numpy() == ref.subm_table(c.coords, c.shape)).all()
    coarse, children, parent, slot = ref.down_tables(c.coords, c.shape)
    assert down.n_out == len(coarse) and down.n_in == len(c.coords) and down.spatial_shape == ref.out_shape(c.shape)
    assert down.coords.dtype == torch.int32 and (down.coords.cpu().numpy() == coarse).all()
    assert (down.children.cpu().numpy() == children).all()
    assert (down.parent.cpu().numpy() == parent).all() and (down.child_slot.cpu().numpy() == slot).all()


@pytest.mark.parametrize("layer", cases.LAYERS)
@pytest.mark.parametrize("name", cases.NAMES)
def test_forward_and_gradients_within_the_float64_bound(name, layer):
    y, dx, dw, db = _device(name)[2][layer][:4]
    want_y, want_dx, want_dw, want_db = _reference(name, layer)
    _within(y, want_y, "%s %s forward" % (name, layer))
    _within(dx, want_dx, "%s %s d feats" % (name, layer))
    _within(dw, want_dw, "%s %s d weight" % (name, layer))
    if cases.BY_NAME[name].bias:
        _within(db, want_db, "%s %s d bias" % (name, layer))


@pytest.mark.parametrize("name", ["rows_65", "three_chunks", "c_40_224", "bias", "odd_all"])
def test_two_calls_give_equal_bytes(name):
    c = cases.BY_NAME[name]
    first = _device(name)
    sub, down = _plans(c.coords, c.shape, c.batch_size)
    for a, b in ((sub.neighbours, first[0].neighbours), (down.children, first[1].children),
                 (down.parent, first[1].parent), (down.coords, first[1].coords)):
        assert torch.equal(a, b)
    for layer in cases.LAYERS:
        again = _layer(layer, sub if layer == "subm" else down, *cases.tensors(name, layer))
        for a, b in zip(again, first[2][layer]):
            assert (a is None and b is None) or a.tobytes() == b.tobytes(), (name, layer)


@pytest.mark.parametrize("name", ["twin_samples", "empty_middle", "odd_all", "bias", "large_values"])
def test_a_batch_equals_each_sample_alone_bit_for_bit(name):
    c = cases.BY_NAME[name]
    _, down, out = _device(name)
    coarse_batch = down.coords.cpu().numpy()[:, 0]
    for s in range(c.batch_size):
        fine = c.coords[:, 0] == s
        if not fine.any():
            continue
        alone = c.coords[fine].copy()
        alone[:, 0] = 0
        sub1, down1 = _plans(alone, c.shape, 1)
        coarse = coarse_batch == s
        assert down1.n_out == coarse.sum()
        for layer in cases.LAYERS:
            x, w, b, g = cases.tensors(name, layer)
            rows_in, rows_out = {"subm": (fine, fine), "down": (fine, coarse), "inverse": (coarse, fine)}[layer]
            y1, dx1 = _layer(layer, sub1 if layer == "subm" else down1, x[rows_in], w, b, g[rows_out])[:2]
            assert y1.tobytes() == out[layer][0][rows_out].tobytes(), (name, layer, s, "forward")
            assert dx1.tobytes() == out[layer][1][rows_in].tobytes(), (name, layer, s, "d feats")


def test_one_plan_shared_by_two_layers_equals_two_plans():
    name = "c_32_48"
    c = cases.BY_NAME[name]
    sub, down, _ = _device(name)
    sub2, down2 = _plans(c.coords, c.shape, c.batch_size)
    x, w, _, g = cases.tensors(name, "subm")
    w2 = np.ascontiguousarray(np.flip(w, 0))         # another layer of the same level
    x2 = _layer("subm", sub, x, w, None, g)[0][:, :c.c_in].copy()      # its input: the first layer's output
    shared = _layer("subm", sub, x, w, None, g) + _layer("subm", sub, x2, w2, None, g)
    apart = _layer("subm", sub, x, w, None, g) + _layer("subm", sub2, x2, w2, None, g)
    xd, wd, _, gd = cases.tensors(name, "down")
    xi, wi, _, gi = cases.tensors(name, "inverse")
    shared += _layer("down", down, xd, wd, None, gd) + _layer("inverse", down, xi, wi, None, gi)
    apart += _layer("down", down, xd, wd, None, gd) + _layer("inverse", down2, xi, wi, None, gi)
    for a, b in zip(shared, apart):
        assert (a is None and b is None) or a.tobytes() == b.tobytes()


def test_int32_coordinates_and_half_inputs():
    name = "rows_65"
    c = cases.BY_NAME[name]
    sub, down, out = _device(name)
    sub32, down32 = _plans(c.coords, c.shape, c.batch_size, dtype=torch.int32)
    assert torch.equal(sub32.neighbours, sub.neighbours) and torch.equal(down32.children, down.children)
    assert torch.equal(down32.coords, down.coords) and torch.equal(down32.parent, down.parent)
    x, w, _, _ = cases.tensors(name, "subm")
    xh = torch.from_numpy(x).to(DEV).half()
    y = _ops().subm_conv3d(xh, torch.from_numpy(w).to(DEV), sub)
    want = _ops().subm_conv3d(xh.float(), torch.from_numpy(w).to(DEV), sub)   # computed from the float32 values
    assert y.dtype == torch.float16 and torch.equal(y, want.half())


def test_an_empty_level_runs_no_kernel_and_gives_bias_alone():
    c = cases.BY_NAME["extent_1"]
    _, down, out = _device("extent_1")
    assert down.n_out == 0 and down.spatial_shape == (0, 2, 2) and (down.parent.cpu().numpy() == -1).all()
    assert out["down"][0].shape == (0, c.c_out) and not out["down"][1].any() and not out["down"][2].any()
    bias = torch.arange(c.c_out, dtype=torch.float32, device=DEV)
    x = torch.zeros((0, c.c_in), device=DEV, requires_grad=True)
    w = torch.ones((c.c_out, 2, 2, 2, c.c_in), device=DEV, requires_grad=True)
    y = _ops().sparse_inverse_conv3d(x, w, down, bias)
    assert torch.equal(y, bias.expand(len(c.coords), c.c_out))
    y.sum().backward()
    assert x.grad.shape == (0, c.c_in) and not w.grad.any()
    none = torch.zeros((0, 4), dtype=torch.int64, device=DEV)
    sub0, down0 = _ops().subm_plan(none, (4, 4, 4), 1), _ops().downsample_plan(none, (4, 4, 4), 1)
    assert sub0.neighbours.shape == (27, 0) and down0.n_out == 0 and down0.coords.shape == (0, 4)
    assert _ops().subm_conv3d(x, torch.ones((3, 3, 3, 3, c.c_in), device=DEV), sub0).shape == (0, 3)


def test_bad_rows_are_refused_by_the_status_word():
    from gapro_amd._lib import GaproError
    ops = _ops()
    good = torch.tensor([[0, 1, 1, 1], [0, 1, 2, 1], [1, 3, 3, 3]], dtype=torch.int64, device=DEV)
    for plan in (ops.subm_plan, ops.downsample_plan):
        plan(good, (4, 4, 4), 2)
        for bad, text in (([0, 1, 1, 1], "same coordinates"), ([0, 4, 0, 0], "outside spatial_shape"),
                          ([0, 0, -1, 0], "outside spatial_shape"), ([2, 0, 0, 0], "batch index"),
                          ([-1, 0, 0, 0], "batch index")):
            rows = torch.cat([good, torch.tensor([bad], dtype=torch.int64, device=DEV)])
            with pytest.raises(GaproError, match=text):
                plan(rows, (4, 4, 4), 2)
    # unchecked, a flagged row simply has no pairs
    rows = torch.cat([good, torch.tensor([[0, 4, 0, 0], [5, 1, 1, 1]], dtype=torch.int64, device=DEV)])
    sub, down = ops.subm_plan(rows, (4, 4, 4), 2, check=False), ops.downsample_plan(rows, (4, 4, 4), 2, check=False)
    assert (sub.neighbours[:, 3:] == -1).all() and (down.parent[3:] == -1).all() and down.n_out == 3
    assert (sub.neighbours[:, :3].cpu().numpy() == ref.subm_table(good.cpu().numpy(), (4, 4, 4))).all()


def test_bad_arguments_are_refused_before_a_launch():
    ops = _ops()
    coords = torch.tensor([[0, 1, 1, 1], [0, 1, 2, 1]], dtype=torch.int64, device=DEV)
    sub, down = ops.subm_plan(coords, (4, 4, 4), 1), ops.downsample_plan(coords, (4, 4, 4), 1)
    x = torch.zeros((2, 6), device=DEV)
    w3, w2 = torch.zeros((8, 3, 3, 3, 6), device=DEV), torch.zeros((8, 2, 2, 2, 6), device=DEV)
    with pytest.raises(ValueError, match="feats has 3 rows, the plan was built for 2"):
        ops.subm_conv3d(torch.zeros((3, 6), device=DEV), w3, sub)
    with pytest.raises(ValueError, match="feats has 3 rows, the plan was built for 2"):
        ops.sparse_inverse_conv3d(torch.zeros((3, 6), device=DEV), w2, down)   # the inverse takes the COARSE rows
    with pytest.raises(ValueError, match="plan must be the SparseConvPlan of downsample_plan"):
        ops.sparse_conv3d(x, w2, sub)
    with pytest.raises(ValueError, match="plan must be the SparseConvPlan of subm_plan"):
        ops.subm_conv3d(x, w3, down)
    with pytest.raises(ValueError, match="weight must be"):
        ops.subm_conv3d(x, w2, sub)
    with pytest.raises(ValueError, match="weight must be"):
        ops.subm_conv3d(x, torch.zeros((8, 3, 3, 3, 5), device=DEV), sub)
    with pytest.raises(ValueError, match="bias must be"):
        ops.subm_conv3d(x, w3, sub, torch.zeros(7, device=DEV))
    with pytest.raises(ValueError, match="1 .. 512 channels"):
        ops.subm_conv3d(x, torch.zeros((513, 3, 3, 3, 6), device=DEV), sub)
    with pytest.raises(ValueError, match="one device is expected"):
        ops.subm_conv3d(x.cpu(), w3.cpu(), sub)
    with pytest.raises(ValueError, match="coords must be"):
        ops.subm_plan(coords[:, :3], (4, 4, 4), 1)
    with pytest.raises(ValueError, match="coords must be"):
        ops.downsample_plan(coords.float(), (4, 4, 4), 1)
    with pytest.raises(ValueError, match="spatial_shape must be"):
        ops.subm_plan(coords, (4, 4), 1)
    with pytest.raises(ValueError, match="spatial_shape must be"):
        ops.subm_plan(coords, (4, 0, 4), 1)
    with pytest.raises(ValueError, match="batch_size must be"):
        ops.downsample_plan(coords, (4, 4, 4), 0)
    with pytest.raises(ValueError, match="63-bit coordinate key"):
        ops.subm_plan(coords, (2 ** 21, 2 ** 21, 2 ** 21), 2)
    with pytest.raises(ValueError, match="check must be"):
        ops.subm_plan(coords, (4, 4, 4), 1, check=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.subm_plan(coords.cpu(), (4, 4, 4), 1)
