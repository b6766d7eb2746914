"""csrc/exact_sum.h on the MI355X.

1. The device's build of fixed_point_shift / to_fixed / fixed_mean against the host's (tests/test_exact_sum_cpu.py holds
   the host's against the oracle): the arrays of tests/exact_sum_cases.py, one launch of one workgroup.
2. The eight-lanes-per-point accumulation (accumulate_features / accumulate_features_wave8) at its edges through the two
   public calls that use it -- the scene partition's pooling (gapro_partition_pool_batch) and the pooled training sets
   (gapro_trainset_count / gapro_trainset_fill) -- each against oracle.pooled_feature_mean bit for bit.  One scene order
   holds the edges: a superpoint of exactly 8 points that fill one wave's point groups (the shuffle fold fires), of 7 and
   of 9 (it must not), two superpoints alternating point by point, a long run, and a 5-point tail (a partial last wave);
   the pattern is laid nine times with fresh ids (1197 points: a second 1024-point run of k_pool_lds, ten workgroups of
   k_ts_accum, every alignment of the pattern in a wave).  D in {1, 6, 8, 9, 32} puts the count lane D % 8 at 1, 6, 0, 1, 0
   and the feature loop at one, two and four rounds.

Already covered elsewhere, not repeated here: the pooling kernels' widths D in {1, 3, 7, 8, 9, 33} at run tails 1023 ..
2049 and every tier of the pooling plan at D = 6 and 32 with the table-full fallback (tests/partition_cases.py WIDTH_TAILS,
SWEEP "shuffled", FACE_CASES "crowded", run by test_partition_edges_gpu.py); sides of one point, of one superpoint,
shared superpoints and doubled lists of the training sets at D = 6 and 32 (test_fit_gp_gpu.py
test_pool_edge_cases_in_one_call).  The fallback case below adds the width those lack: D = 9, two feature rounds with
the count lane inside the first."""
import numpy as np
import pytest

import exact_sum_cases as X
import partition_cases as P
from oracle import gen_ps_oracle as O

pytestmark = pytest.mark.gpu

WIDTHS = (1, 6, 8, 9, 32)
PATTERN = ((0, 8), (1, 7), (2, 9)) + ((3, 1), (4, 1)) * 32 + ((5, 40), (6, 5))  # (superpoint, consecutive points)


def test_the_device_computes_what_the_host_computes():
    from gapro_amd._lib import Context

    host, dev = X.evaluate(None), X.evaluate(Context.get(0))
    for h, g in zip(host, dev):
        assert h.dtype == g.dtype and len(h) >= 88
        np.testing.assert_array_equal(g, h)


def _scene(d, runs, tiles, seed):
    """Points in the order of `runs`, laid `tiles` times with 7 fresh ids each; ids 10, 13, 16, ...; one instance box."""
    rng = np.random.default_rng(seed)
    idx = np.concatenate([np.full(c, s + 7 * t) for t in range(tiles) for s, c in runs])
    spp = (10 + 3 * idx).astype(np.int64)
    coords = rng.uniform(0.0, 1.0, size=(len(spp), 3)) * [4.0, 4.0, 2.0]
    feats = (3.0 * rng.standard_normal((len(spp), d))).astype(np.float32)
    return coords, feats, spp


def _expected(feats, spp):
    ids, inv = np.unique(spp, return_inverse=True)
    return ids, inv, O.pooled_feature_mean(feats, inv, len(ids))


def _pooled_by_the_partition(coords, feats, spp, want_lds=True):
    from gapro_amd import _lib

    kw = P.boxes_kw(coords, feats, spp, [[0.5, 0.5, 0.2, 2.5, 2.5, 1.5]])
    pipe, job = P._run_partition(kw)
    plan = _lib.load().gapro_partition_pool_plan(feats.shape[1], len(job.boxes))
    assert (plan > 0) == want_lds  # k_pool_lds with a table of 2^plan slots
    return plan, job.dev["point_count"].cpu().numpy(), job.dev["feats_spp"].cpu().numpy()


@pytest.mark.parametrize("d", WIDTHS)
def test_partition_pooling_at_the_wave_group_edges(d):
    coords, feats, spp = _scene(d, PATTERN, 9, 100 + d)
    assert len(spp) == 9 * 133 and len(spp) % 8 == 5 and len(spp) > P.K_POOL_RUN
    ids, inv, want = _expected(feats, spp)
    _, count, got = _pooled_by_the_partition(coords, feats, spp)
    np.testing.assert_array_equal(count, np.bincount(inv))
    np.testing.assert_array_equal(got, want)


def test_partition_pooling_when_the_lds_table_is_full():
    """About 700 superpoints of one or two points in the first 1024-point run, a table of 64 slots at most: most points
    take k_pool_lds's global branch; the last 70 points share one superpoint (the folded branch beside it)."""
    d = 9
    coords, feats, spp = _scene(d, tuple((s, 1 + s % 2) for s in range(7)), 160, 3)
    spp[-70:] = spp[-1]
    assert 1024 < len(spp) <= 2048
    ids, inv, want = _expected(feats, spp)
    plan, count, got = _pooled_by_the_partition(coords, feats, spp)
    assert len(np.unique(spp[:P.K_POOL_RUN])) > 10 * (1 << plan)
    np.testing.assert_array_equal(count, np.bincount(inv))
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("d", WIDTHS)
def test_training_set_pooling_at_the_wave_group_edges(d):
    """Side 1 lists every point in scene order (the pattern as it lies), side 2 the points of every other superpoint
    backwards: sides of whole superpoints, so their rows are the scene's pooled means themselves."""
    from gapro_amd import gp_train_sets

    coords, feats, spp = _scene(d, PATTERN, 9, 100 + d)
    ids, inv, want = _expected(feats, spp)
    every_other = np.nonzero(inv % 2 == 0)[0][::-1]
    (x, m1, m2, sel1, sel2), = gp_train_sets(coords, feats, spp, [(np.arange(len(spp)), every_other, np.arange(10))])
    assert (m1, m2) == (len(ids), (len(ids) + 1) // 2)
    np.testing.assert_array_equal(sel1, ids)
    np.testing.assert_array_equal(sel2, ids[::2])
    np.testing.assert_array_equal(x[:m1], want)
    np.testing.assert_array_equal(x[m1:], want[::2])
