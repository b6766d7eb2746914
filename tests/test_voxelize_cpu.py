"""The voxelisation without a GPU: the NumPy restatement (tests/voxelize_ref.py) against hand-checked answers, every
wrong convention shown to fail on the case that catches it, and the host path (gapro_voxelize_host_*, through the public
``voxelization_idx`` on CPU tensors) bit for bit against the restatement on every indexing case.
"""
import numpy as np
import pytest

import voxelize_cases as cases
import voxelize_ref as ref


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the restatement against answers worked out by hand ---------------------------------------------------------------
def test_restatement_numbers_voxels_by_first_point():
    coords = cases.index_cases()["descending_keys"]["coords"]  # 9 5 9 1 5
    oc, im, om, flags = ref.voxelize_idx_ref(coords, 4)
    assert flags == 0
    assert im.tolist() == [0, 1, 0, 2, 1]
    assert oc.tolist() == [[0, 9, 9, 9], [0, 5, 5, 5], [0, 1, 1, 1]]
    assert om.tolist() == [[2, 0, 2], [2, 1, 4], [1, 3, 0]]
    assert ref.voxelize_idx_ref(coords, 1)[2].tolist() == [[1, 0], [1, 1], [1, 3]]  # mode 1: the first point
    assert ref.voxelize_idx_ref(coords, 2)[2].tolist() == [[1, 2], [1, 4], [1, 3]]  # mode 2: the last point
    assert ref.voxelize_idx_ref(coords, 0)[3] == ref.FLAG_DUPLICATE
    assert ref.voxelize_idx_ref(coords[[0, 1, 3]], 0)[2].tolist() == [[1, 0], [1, 1], [1, 2]]


def test_restatement_pools_in_float32_one_operation_at_a_time():
    third = np.float32(1.0) / np.float32(3.0)
    x = np.array([[1.0], [1.0], [1.0]], np.float32)
    table = np.array([[3, 0, 1, 2], [0, 2, 2, 2], [1, 2, 0, 0]], np.int32)
    out = ref.pool_forward_ref(x, table, 4)
    assert out[0, 0] == np.float32(np.float32(third + third) + third) and out[1, 0] == 0 and out[2, 0] == 1
    assert ref.pool_forward_ref(x, table, 3)[:, 0].tolist() == [3.0, 0.0, 1.0]
    neg = cases.pool_cases()["negative_zero"]
    got = ref.pool_forward_ref(neg["feats"], neg["map_rule"], 4)
    assert not np.signbit(got[:2]).any()  # 0 + (-0.0) = +0.0: a single -0.0 input gives +0.0
    d = ref.pool_backward_ref(np.array([[3.0], [5.0], [7.0]], np.float32), table, 4, 4)
    assert d[:, 0].tolist() == [float(np.float32(3.0) * third)] * 2 + [7.0, 0.0]  # point 2: listed by the later row


def test_restatement_refusals_and_flags():
    c = cases.index_cases()
    assert ref.voxelize_idx_ref(c["negative_batch"]["coords"], 4)[3] == ref.FLAG_BATCH
    assert ref.voxelize_idx_ref(c["max_active_at_cap"]["coords"], 4)[2].shape == (3, ref.MAX_ACTIVE + 1)
    with pytest.raises(ref.Refused):
        ref.voxelize_idx_ref(c["max_active_beyond_cap"]["coords"], 4)
    with pytest.raises(ref.Refused):
        ref.table_width(4, 2 ** 30, 1)
    assert ref.table_width(1, 2 ** 30 - 1, 7) == 2
    p = cases.pool_cases()
    assert ref.pool_flags(p["rows_C3"]["map_rule"], 200) == 0
    assert ref.pool_flags(p["garbage_padding"]["map_rule"], 200) == 0
    assert ref.pool_flags(p["bad_counts"]["map_rule"], 200) == ref.POOL_COUNT
    assert ref.pool_flags(p["bad_indices"]["map_rule"], 200) == ref.POOL_INDEX
    assert ref.pool_flags(p["listed_twice"]["map_rule"], 200) == ref.POOL_TWICE


# ---- every wrong convention fails on the case that catches it ----------------------------------------------------------
def test_cases_catch_the_wrong_conventions():
    c = cases.index_cases()
    for name in ("descending_keys", "distinct_65"):
        right = ref.voxelize_idx_ref(c[name]["coords"], 4)
        wrong = ref.voxelize_idx_ref(c[name]["coords"], 4, sorted_numbering=True)
        assert not _same(right[1], wrong[1]) and not _same(right[0], wrong[0])
    for name in ("interleaved", "rows_63_64_65", "rows_8_9"):
        right = ref.voxelize_idx_ref(c[name]["coords"], c[name]["mode"])
        wrong = ref.voxelize_idx_ref(c[name]["coords"], c[name]["mode"], unordered_rows=True)
        assert _same(right[1], wrong[1]) and not _same(right[2], wrong[2])
        assert all((np.diff(r[1:1 + r[0]]) > 0).all() for r in right[2])  # ascending rows
    for mode in (1, 2):
        coords = c["mode_%d_duplicates" % mode]["coords"]
        assert not _same(ref.voxelize_idx_ref(coords, mode)[2],
                         ref.voxelize_idx_ref(coords, mode, swap_first_last=True)[2])
    x, table = cases.three_way_row()
    got = {k: ref.pool_forward_ref(x, table, 4, convention=k).tobytes() for k in ("unfused", "fused", "divide")}
    assert len(set(got.values())) == 3


# ---- the host path ---------------------------------------------------------------------------------------------------
def _run_host(case):
    import torch

    from gapro_amd import consumer_ops as ops

    out = ops.voxelization_idx(torch.from_numpy(case["coords"].copy()), 4, case["mode"])
    assert all(not t.is_cuda for t in out)
    return tuple(t.numpy() for t in out)


def _check_index_case(run, case):
    """``run(case)`` against the restatement: the same bits, or the same refusal."""
    from gapro_amd._lib import GaproError

    try:
        oc, im, om, flags = ref.voxelize_idx_ref(case["coords"], case["mode"])
    except ref.Refused:
        with pytest.raises(ValueError):
            run(case)
        return
    if flags:
        with pytest.raises(GaproError) as err:
            run(case)
        assert err.value.code == ref.BAD_ARG
        return
    got_oc, got_im, got_om = run(case)
    assert _same(got_im, im) and _same(got_oc, oc) and _same(got_om, om)


@pytest.mark.parametrize("name", cases.INDEX_NAMES)
def test_host_path_equals_the_restatement(name):
    _check_index_case(_run_host, cases.index_cases()[name])


def test_host_path_on_colliding_keys_and_the_plan():
    from gapro_amd import consumer_ops as ops

    case = cases.collision_case(ops.voxelize_plan, ops.voxelize_hash)
    slots = ops.voxelize_plan(len(case["coords"]))
    assert slots >= 2 * len(case["coords"]) and slots & (slots - 1) == 0
    keys = np.unique(case["coords"], axis=0)
    assert len(keys) >= 40 and (ops.voxelize_hash(keys) & np.uint64(slots - 1)).max() < 8  # one cluster of the table
    _check_index_case(_run_host, case)


def test_header_arithmetic_refuses_without_allocating():
    from gapro_amd import consumer_ops as ops

    assert ops.voxel_table_shape(4, 3, 5) == 6 and ops.voxel_table_shape(1, 3, 5) == 2
    assert ops.voxel_table_shape(3, 2 ** 30 - 1, 1) == 2 and ops.voxel_table_shape(4, 1, 4096) == 4097
    for mode, n_voxels, max_active in ((4, 2 ** 30, 1), (4, 2 ** 20, 2 ** 11), (3, 1, 4097), (0, 5, 2),
                                       (1, 2 ** 30, 9)):
        with pytest.raises(ValueError):
            ops.voxel_table_shape(mode, n_voxels, max_active)  # a fabricated header: int32 overflow of M * (A + 1), ...


def test_voxelization_idx_refuses_bad_arguments():
    import torch

    from gapro_amd import consumer_ops as ops

    good = torch.zeros((5, 4), dtype=torch.int64)
    for coords, batchsize, mode in ((good.to(torch.int32), 1, 4), (torch.zeros((5, 5), dtype=torch.int64), 1, 4),
                                    (torch.zeros(5, dtype=torch.int64), 1, 4), (good, 0, 4), (good, 1.0, 4),
                                    (good, 1, 5), (good, 1, -1), (good, 1, True)):
        with pytest.raises(ValueError):
            ops.voxelization_idx(coords, batchsize, mode)
    oc, im, om = ops.voxelization_idx(good[:, 1:].t().contiguous().t(), 3)  # not contiguous: copied
    assert oc.tolist() == [[0, 0, 0]] and im.tolist() == [0] * 5 and om.tolist() == [[5, 0, 1, 2, 3, 4]]
    with pytest.raises(ValueError):
        ops.voxelization(torch.zeros((3, 2)), torch.zeros((1, 2), dtype=torch.int64))
    with pytest.raises(RuntimeError):
        ops.voxelization(torch.zeros((3, 2)), torch.zeros((1, 2), dtype=torch.int32))  # host tensors: no CPU pooling
