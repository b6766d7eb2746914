"""The NumPy restatement of the sparse convolutions (tests/spconv_ref.py) against torch's float64 dense conv3d /
conv_transpose3d and their autograd, its rulebooks against a brute-force search, and the wrong conventions it must not
have.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import spconv_cases as cases
import spconv_ref as ref

REL = 1e-12


def _close(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, what
    scale = max(np.abs(b).max(), 1e-300) if b.size else 1.0
    assert b.size == 0 or np.abs(a - b).max() <= REL * scale, (what, np.abs(a - b).max(), scale)


def _scatter(x, coords, B, shape):
    """[rows, C] on ``coords`` -> a dense [B, C, Dz, Dy, Dx] grid (zeros elsewhere), differentiable."""
    grid = torch.zeros((B,) + tuple(shape) + (x.shape[1],), dtype=torch.float64)
    c = torch.as_tensor(np.asarray(coords, dtype=np.int64))
    if len(c):
        grid = grid.index_put((c[:, 0], c[:, 1], c[:, 2], c[:, 3]), x)
    return grid.permute(0, 4, 1, 2, 3)


def _gather(grid, coords):
    c = torch.as_tensor(np.asarray(coords, dtype=np.int64))
    return grid[c[:, 0], :, c[:, 1], c[:, 2], c[:, 3]]


def dense_layer(layer, case, x, w, b):
    """The layer by torch's dense float64 ops, on leaves that require grad; None where torch has no such grid."""
    coarse, _, parent, _ = ref.down_tables(case.coords, case.shape)
    Do = ref.out_shape(case.shape)
    bias = None if b is None else b
    if layer == "subm":
        y = F.conv3d(_scatter(x, case.coords, case.batch_size, case.shape), w.permute(0, 4, 1, 2, 3), bias, padding=1)
        return _gather(y, case.coords)
    if min(Do) == 0:
        return None
    if layer == "down":
        y = F.conv3d(_scatter(x, case.coords, case.batch_size, case.shape), w.permute(0, 4, 1, 2, 3), bias, stride=2)
        return _gather(y, coarse)
    y = F.conv_transpose3d(_scatter(x, coarse, case.batch_size, Do), w.permute(4, 0, 1, 2, 3), bias, stride=2)
    inside = parent >= 0  # the dropped slice lies beyond the transposed convolution's grid: bias alone
    rows = [(_gather(y, case.coords[i:i + 1])[0] if inside[i] else
             (bias if bias is not None else torch.zeros(w.shape[0], dtype=torch.float64)))
            for i in range(len(case.coords))]
    return torch.stack(rows) + 0.0 * (x.sum() + w.sum())  # a graph even when every row was dropped


def reference_layer(layer, case, x, w, b, g, wrong=None):
    tab, rows_in = ref.layer_tables(layer, case.coords, case.shape, wrong)
    y = ref.forward(tab, x, w, b, wrong)[0]
    dx = ref.backward_input(tab, rows_in, g, w)[0]
    (dw, _, _), (db, _, _) = ref.backward_weight(tab, x, g, w.shape)
    return y, dx, dw, db


@pytest.mark.parametrize("layer", cases.LAYERS)
@pytest.mark.parametrize("name", cases.NAMES)
def test_restatement_equals_torch_dense_float64(name, layer):
    case = cases.BY_NAME[name]
    x, w, b, g = cases.tensors(name, layer)
    y, dx, dw, db = reference_layer(layer, case, x, w, b, g)
    leaves = [torch.tensor(t, dtype=torch.float64, requires_grad=True) if t is not None else None for t in (x, w, b)]
    dense = dense_layer(layer, case, *leaves)
    if dense is None:  # an extent of 1: no coarse voxel at all
        assert len(ref.down_tables(case.coords, case.shape)[0]) == 0
        assert y.shape[0] == (0 if layer == "down" else len(case.coords))
        if layer == "inverse":
            _close(y, np.broadcast_to(0.0 if b is None else b.astype(np.float64), y.shape), "bias alone")
        return
    _close(y, dense.detach().numpy(), "forward")
    dense.backward(torch.tensor(g, dtype=torch.float64))
    _close(dx, leaves[0].grad.numpy() if leaves[0].grad is not None else np.zeros_like(dx), "d feats")
    _close(dw, leaves[1].grad.numpy(), "d weight")
    if b is not None:
        _close(db, leaves[2].grad.numpy(), "d bias")


@pytest.mark.parametrize("name", cases.NAMES)
def test_rulebooks_equal_a_brute_force_search(name):
    case = cases.BY_NAME[name]
    c, shape = case.coords, case.shape
    nbr = ref.subm_table(c, shape)
    for k, d in enumerate(ref.OFFSETS):
        want = c[:, None, :] + np.array((0,) + d)[None, None, :]       # [V, 1, 4]
        hit = (want == c[None, :, :]).all(-1)                           # [V, V]: O(V^2)
        assert (hit.sum(1) <= 1).all()
        assert (nbr[k] == np.where(hit.any(1), hit.argmax(1), -1)).all(), k
    coarse, children, parent, slot = ref.down_tables(c, shape)
    Do = ref.out_shape(shape)
    q = np.concatenate([c[:, :1], c[:, 1:] >> 1], axis=1)
    kept = (q[:, 1:] < np.array(Do)).all(1)
    same = (q[:, None, :] == q[None, :, :]).all(-1) & kept[:, None] & kept[None, :]
    first = np.where(kept, same.argmax(1), -1)                          # the first row of each coarse voxel
    firsts = sorted(set(first[kept].tolist()))                          # ascending input row = the numbering
    assert (coarse == q[firsts]).all() and len(coarse) == len(firsts)
    assert (parent == np.where(kept, np.searchsorted(firsts, np.maximum(first, 0)), -1)).all()
    assert (slot == (c[:, 1] & 1) * 4 + (c[:, 2] & 1) * 2 + (c[:, 3] & 1)).all()
    for k in range(8):
        for v in range(len(coarse)):
            mine = np.nonzero((parent == v) & (slot == k))[0]
            assert len(mine) <= 1 and children[k, v] == (mine[0] if len(mine) else -1)


def _differs(a, b):
    return a.shape != b.shape or np.abs(a - b).max() > 1e-6 * max(np.abs(b).max(), 1.0)


@pytest.mark.parametrize("wrong, name, layer", [
    ("convolution", "full_block", "subm"),      # an asymmetric weight on a full 3^3 block
    ("xz", "rows_65", "subm"),                  # a 6 x 7 x 5 grid: z and x differ
    ("weight_layout", "c_32_48", "subm"),       # C_in != C_out
    ("weight_layout", "bias_odd", "down"),
    ("keep_odd", "odd_dz", "down"),             # voxels in z = 4 of Dz = 5
    ("no_batch", "twin_samples", "subm"),       # two samples with identical coordinates
    ("no_batch", "twin_samples", "down"),
])
def test_a_wrong_convention_is_caught(wrong, name, layer):
    case = cases.BY_NAME[name]
    x, w, b, g = cases.tensors(name, layer)
    right = dense_layer(layer, case, *[None if t is None else torch.tensor(t, dtype=torch.float64) for t in (x, w, b)])
    tab, _ = ref.layer_tables(layer, case.coords, case.shape, wrong)
    assert _differs(ref.forward(tab, x, w, b, wrong)[0], right.numpy()), wrong
    tab, _ = ref.layer_tables(layer, case.coords, case.shape)
    assert not _differs(ref.forward(tab, x, w, b)[0], right.numpy())


def test_a_dilating_submanifold_layer_is_caught():
    """Two stacked layers: the submanifold layer's output lives on the input's rows only.  A layer that also produced
    the inactive neighbours (a dense convolution) would feed them to the second layer."""
    case = cases.BY_NAME["rows_17"]
    x, w, _, _ = cases.tensors("rows_17", "subm")
    w2 = np.ascontiguousarray(w[:case.c_in, ..., :case.c_in]) if case.c_out >= case.c_in else None
    w1 = np.ascontiguousarray(w[:case.c_in])
    tab = ref.subm_table(case.coords, case.shape)
    ours = ref.forward(tab, ref.forward(tab, x, w1)[0], w1)[0]
    tx, tw = torch.tensor(x, dtype=torch.float64), torch.tensor(w1, dtype=torch.float64).permute(0, 4, 1, 2, 3)
    grid = _scatter(tx, case.coords, case.batch_size, case.shape)
    once = F.conv3d(grid, tw, padding=1)
    masked = _scatter(_gather(once, case.coords), case.coords, case.batch_size, case.shape)
    _close(ours, _gather(F.conv3d(masked, tw, padding=1), case.coords).numpy(), "submanifold twice")
    assert _differs(ours, _gather(F.conv3d(once, tw, padding=1), case.coords).numpy())
    assert w2 is not None


def test_coarse_rows_are_numbered_by_first_child_not_sorted():
    case = cases.BY_NAME["odd_all"]
    coarse = ref.down_tables(case.coords, case.shape)[0]
    by_sort = ref.down_tables(case.coords, case.shape, "sorted")[0]
    assert sorted(map(tuple, coarse)) == list(map(tuple, by_sort)) and (coarse != by_sort).any()
    # first-child order: the first appearances of the coarse coordinates while walking the input rows
    seen = []
    for r in case.coords:
        q = (int(r[0]),) + tuple(int(v) >> 1 for v in r[1:])
        if all(q[1 + a] < ref.out_shape(case.shape)[a] for a in range(3)) and q not in seen:
            seen.append(q)
    assert list(map(tuple, coarse)) == seen


def test_the_cases_cover_what_they_are_named_for():
    from gapro_amd import _lib
    lib = _lib.load()
    assert (cases.CIN_CHUNK, cases.MIN_CHUNK_ROWS) == (_lib.SPCONV_CIN_CHUNK, _lib.SPCONV_MIN_CHUNK_ROWS)
    c = cases.BY_NAME["three_chunks"]
    V = len(c.coords)
    rows = lib.gapro_spconv_chunk_rows(V, 27, c.c_in, c.c_out)
    assert rows == cases.MIN_CHUNK_ROWS and -(-V // rows) == 3 and -(-(V - 1) // rows) == 2
    assert lib.gapro_spconv_workspace_bytes(V, 27, c.c_in, c.c_out) >= 3 * 27 * 16 * 16 * 8
    # the workspace stays bounded at the consumers' step shape: 551 188 rows, 32 channels, and at 224 channels
    assert lib.gapro_spconv_workspace_bytes(551188, 27, 32, 32) <= (64 << 20) + 27 * 32 * 32 * 8 + (1 << 20)
    assert lib.gapro_spconv_workspace_bytes(4096, 27, 224, 224) <= (64 << 20) + 4096
    assert lib.gapro_spconv_workspace_bytes(0, 27, 32, 32) == 0 and lib.gapro_spconv_workspace_bytes(5, 27, 513, 4) == 0
    nbr = ref.subm_table(cases.BY_NAME["isolated"].coords, (7, 7, 7))
    assert (nbr[13] == [0, 1]).all() and (np.delete(nbr, 13, 0) == -1).all()
    assert (ref.subm_table(cases.BY_NAME["full_block"].coords, (6, 6, 6))[:, 13] >= 0).all()
    assert (ref.down_tables(cases.BY_NAME["odd_dz"].coords, (5, 4, 4))[2] == -1).sum() == 16
    assert len(ref.down_tables(cases.BY_NAME["extent_1"].coords, (1, 4, 5))[0]) == 0
    shuffled = cases.BY_NAME["rows_65"].coords
    assert (np.lexsort(shuffled.T[::-1]) != np.arange(len(shuffled))).any()
    # rows_1025: coarse rows are numbered in the first and in the second block of the down plan's scan, so the carry
    # into the second block is not zero and a coarse row's number is read from behind it
    late = cases.BY_NAME["rows_1025"]
    V = len(late.coords)
    assert V == cases.SCAN_BLOCK + 1 and late.batch_size == 1 and len(np.unique(late.coords, axis=0)) == V
    assert (np.lexsort(late.coords.T[::-1]) != np.arange(V)).any()
    children = ref.down_tables(late.coords, late.shape)[1]
    first_child = np.where(children >= 0, children, V).min(0)
    assert (first_child >= cases.SCAN_BLOCK).any() and (first_child < cases.SCAN_BLOCK).any()
