"""Point-level fits without a GPU: the NumPy restatement of the training-set assembly (tests/fit_gp_ref.py) against
the oracle's pooled features, its ordering rules, the public names, and the errors raised before a device is touched."""
import ctypes as C

import numpy as np
import pytest

import fit_gp_ref as R
from oracle import gen_ps_oracle as O


@pytest.mark.parametrize("name", ["s0_walls", "s4_dups", "s5_lean"])
def test_whole_superpoint_sides_pool_to_the_partitions_rows(name):
    """A side made of whole superpoints pools to the partition's own feats_spp rows, bit for bit."""
    coords, feats, spp, inv, problems = R.golden_scene(name)
    ref = O.pooled_feature_mean(feats, inv, int(inv.max()) + 1)
    uniq = np.unique(spp)
    assert len(problems) == {"s0_walls": 9, "s4_dups": 4, "s5_lean": 19}[name]
    for prob in problems:
        x, m1, m2, s1, s2, status = R.train_set(coords, feats, spp, prob, spp_pool=True)
        ranks = np.concatenate([np.searchsorted(uniq, s1), np.searchsorted(uniq, s2)])
        assert status == 0 and x.dtype == np.float32 and x.shape == (m1 + m2, feats.shape[1])
        assert np.array_equal(x, ref[ranks])
        assert np.array_equal(s1, np.unique(spp[prob[0]])) and np.array_equal(s2, np.unique(spp[prob[1]]))


def test_pooling_counts_duplicates_and_ignores_order():
    rng = np.random.default_rng(0)
    feats = rng.normal(size=(50, 6)).astype(np.float32)
    spp = rng.integers(0, 5, size=50)
    inds = rng.permutation(50)[:30]
    rows, ids = R.pool_side(feats, spp, inds)
    rows2, ids2 = R.pool_side(feats, spp, inds[::-1])
    assert np.array_equal(rows, rows2) and np.array_equal(ids, ids2)
    twice, _ = R.pool_side(feats, spp, np.concatenate([inds, inds]))
    assert np.array_equal(rows, twice)  # every point twice: the same means, exactly
    once_more, _ = R.pool_side(feats, spp, np.concatenate([inds, inds[:1]]))
    assert not np.array_equal(rows, once_more)


def test_a_short_side_keeps_its_order():
    rng = np.random.default_rng(1)
    coords = rng.normal(size=(100, 3))
    feats = rng.normal(size=(100, 6)).astype(np.float32)
    b1, b2, it = rng.permutation(100)[:7], rng.permutation(100)[:8], np.arange(5)
    for k in (8, 9, 800):
        x, m1, m2, s1, s2, _ = R.train_set(coords, feats, np.zeros(100, np.int64), (b1, b2, it), k, spp_pool=False)
        assert (m1, m2) == (7, 8) and np.array_equal(s1, b1) and np.array_equal(s2, b2)
        assert np.array_equal(x, feats[np.concatenate([b1, b2])])
    x, m1, m2, s1, s2, _ = R.train_set(coords, feats, np.zeros(100, np.int64), (b1, b2, it), 7, spp_pool=False)
    assert (m1, m2) == (7, 7) and np.array_equal(s1, b1) and not np.array_equal(s2, b2[:7])


def test_ties_at_the_cut_go_to_the_earlier_position():
    """The k-th and (k + 1)-th distances are equal: the one listed first is kept, and equal distances inside the kept
    set stand in list order."""
    coords = np.zeros((8, 3))
    coords[:, 0] = [5.0, 1.0, 2.0, 2.0, 3.0, 2.0, 0.5, 2.0]  # the intersection point sits at the origin
    coords = np.concatenate([coords, np.zeros((1, 3))])
    side = np.array([0, 7, 5, 1, 3, 2, 4, 6])  # distances 25, 4, 4, 1, 4, 4, 9, .25
    c = R.centroid(coords, [8])
    assert np.array_equal(c, np.zeros(3))
    assert np.array_equal(R.nearest_side(coords, side, c, 4), [6, 1, 7, 5])  # .25, 1, then the first two 4s as listed
    assert np.array_equal(R.nearest_side(coords, side, c, 3), [6, 1, 7])
    assert np.array_equal(R.nearest_side(coords, side, c, 6), [6, 1, 7, 5, 3, 2])
    assert np.array_equal(R.nearest_side(coords, side[::-1], c, 4), [6, 1, 2, 3])


def test_the_centroid_does_not_depend_on_the_order():
    rng = np.random.default_rng(2)
    coords = rng.normal(scale=3.0, size=(5000, 3))
    it = rng.permutation(5000)[:3000]
    c = R.centroid(coords, it)
    assert np.array_equal(c, R.centroid(coords, it[::-1])) and np.array_equal(c, R.centroid(coords, np.sort(it)))
    assert np.max(np.abs(c - coords[it].mean(0))) < 1e-13


def test_a_non_finite_coordinate_elsewhere_does_not_move_the_centroid():
    rng = np.random.default_rng(4)
    coords = rng.normal(scale=3.0, size=(2000, 3))
    it = rng.permutation(1000)[:600]
    c = R.centroid(coords, it)
    for bad in (np.inf, -np.inf, np.nan):
        other = coords.copy()
        other[1500, 1] = bad  # a point of no problem
        assert np.array_equal(R.centroid(other, it), c)


def test_names_are_exported_and_the_descriptor_matches_the_header():
    import gapro_amd
    from gapro_amd import _lib

    for name in ("fit_gp", "fit_gp_batch", "gp_train_sets"):
        assert name in gapro_amd.__all__ and callable(getattr(gapro_amd, name))
    assert C.sizeof(_lib.TrainsetDesc) == 8 + 6 * 4 + 8
    lib = _lib.load()
    descs = (_lib.TrainsetDesc * 2)()
    for d, (n1, n2, t) in zip(descs, [(5, 7, 3), (2000, 1, 0)]):
        d.n1, d.n2, d.t = n1, n2, t
    assert lib.gapro_trainset_workspace_bytes(_lib.TRAINSET_NEAREST, C.cast(descs, C.c_void_p), 2, 0, 6) >= 2 * 3 * 8
    # pool: two rank tables per problem, and int64 sums + a count for at most min(n, S) rows per side
    need = 2 * 2 * 100 * 4 + (5 + 7 + 100 + 1) * (6 * 8 + 4)
    assert lib.gapro_trainset_workspace_bytes(_lib.TRAINSET_POOL, C.cast(descs, C.c_void_p), 2, 100, 6) >= need
    descs[1].n2 = 0  # an empty side
    assert lib.gapro_trainset_workspace_bytes(_lib.TRAINSET_POOL, C.cast(descs, C.c_void_p), 2, 100, 6) == 0


def _inputs(n=40):
    rng = np.random.default_rng(3)
    return rng.normal(size=(n, 3)), rng.normal(size=(n, 6)).astype(np.float32), rng.integers(0, 4, size=n)


@pytest.mark.parametrize("fn", ["gp_train_sets", "fit_gp_batch"])
def test_bad_arguments_raise_before_a_device_is_touched(fn, monkeypatch):
    import gapro_amd
    from gapro_amd import _lib
    from gapro_amd import gaussian_process_utils as G

    def no_device(*a, **k):
        raise AssertionError("a device was asked for")

    monkeypatch.setattr(G, "_pipeline", no_device)
    call = getattr(gapro_amd, fn)
    coords, feats, spp = _inputs()
    ok = (np.arange(5), np.arange(5, 12), np.arange(12, 20))
    for k in (0, -3, 1025):
        with pytest.raises(ValueError, match="npoint_nearest"):
            call(coords, feats, spp, [ok], npoint_nearest=k, spp_pool=False)
    with pytest.raises(ValueError, match="centroid"):  # T = 0 and a side longer than npoint_nearest
        call(coords, feats, spp, [(np.arange(5), np.arange(5, 12), [])], npoint_nearest=6, spp_pool=False)
    for mode in (True, False):
        with pytest.raises(ValueError, match="each side"):
            call(coords, feats, spp, [ok, (np.arange(5), [], np.arange(3))], spp_pool=mode)
        with pytest.raises(ValueError, match="outside"):
            call(coords, feats, spp, [(np.arange(5), np.array([40]), np.arange(3))], spp_pool=mode)
        with pytest.raises(ValueError):
            call(coords[:-1], feats, spp, [ok], spp_pool=mode)
        # the exact sums have room for 4 N terms: a list (indices may repeat) holds at most 2 N entries
        with pytest.raises(ValueError, match="longer than 2 times"):
            call(coords, feats, spp, [(np.tile(np.arange(5), 17), np.arange(5, 12), np.arange(3))], spp_pool=mode)
        # two grid rows per problem: a call holds at most TRAINSET_MAX_PROBLEMS of them, and says so
        assert _lib.TRAINSET_MAX_PROBLEMS == 32767
        with pytest.raises(ValueError, match="at most 32767"):
            call(coords, feats, spp, [ok] * (_lib.TRAINSET_MAX_PROBLEMS + 1), npoint_nearest=6, spp_pool=mode)
    # what is NOT an error: npoint_nearest is ignored when pooling; an empty intersection with short sides; a list of
    # exactly 2 N entries
    with pytest.raises(AssertionError, match="a device was asked for"):
        call(coords, feats, spp, [ok], npoint_nearest=0, spp_pool=True)
    with pytest.raises(AssertionError, match="a device was asked for"):
        call(coords, feats, spp, [(np.tile(np.arange(5), 16), np.arange(5, 12), np.arange(3))], spp_pool=True)
    with pytest.raises(AssertionError, match="a device was asked for"):
        call(coords, feats, spp, [(np.arange(5), np.arange(5, 12), [])], npoint_nearest=7, spp_pool=False)


def test_fit_gp_raises_the_same_errors(monkeypatch):
    import gapro_amd
    from gapro_amd import gaussian_process_utils as G

    monkeypatch.setattr(G, "_pipeline", lambda *a, **k: (_ for _ in ()).throw(AssertionError("device")))
    coords, feats, spp = _inputs()
    with pytest.raises(ValueError, match="npoint_nearest"):
        gapro_amd.fit_gp(coords, feats, spp, np.arange(5), np.arange(5, 12), np.arange(12, 20), 50, 2000, False)
    with pytest.raises(ValueError, match="each side"):
        gapro_amd.fit_gp(coords, feats, spp, [], np.arange(5, 12), np.arange(12, 20))
