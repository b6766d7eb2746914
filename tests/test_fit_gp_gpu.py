"""Point-level GP fits on the MI355X: the device-side training-set assembly against its NumPy restatement
(tests/fit_gp_ref.py) bit for bit, the chain assembly -> fit -> predict against the existing calls it is made of bit for
bit, and against the float64 oracle with tests/test_fit_gpu.py's tolerances."""
import numpy as np
import pytest

import fit_gp_ref as R
from trainset_cases import same_sets as _same_sets  # shared with tests/test_trainset_edges_gpu.py

pytestmark = pytest.mark.gpu

VAR_RTOL, MU_RTOL, MU_ATOL, P_ATOL = 1e-5, 1e-5, 1e-7, 2e-7  # tests/test_fit_gpu.py::_compare


# ---------------------------------------------------------------------------------------------- 1. pool, goldens
@pytest.mark.parametrize("name,n", [("s0_walls", 9), ("s4_dups", 4), ("s5_lean", 19)])
def test_pool_assembly_is_exact_on_the_golden_scenes(name, n):
    from gapro_amd import gp_train_sets

    coords, feats, spp, _, problems = R.golden_scene(name)
    assert len(problems) == n
    _same_sets(gp_train_sets(coords, feats, spp, problems), coords, feats, spp, problems, what=name)


# ---------------------------------------------------------------------------------------------- 2. pool, edge cases
def _scattered(d, span):
    """N = 20 000 points in runs of 1 .. 150 over 257 distinct ids that start at 7 and span `span` ids."""
    rng = np.random.default_rng(40 + d)
    n = 20000
    ids = np.sort(np.concatenate([[7, 7 + span - 1], 8 + rng.choice(span - 2, size=255, replace=False)])).astype(np.int64)
    runs = np.repeat(rng.integers(0, 257, size=n), rng.integers(1, 150, size=n))[:n]
    runs[:257] = np.arange(257)  # every id occurs
    spp = ids[runs]
    coords = rng.normal(scale=2.0, size=(n, 3))
    feats = (rng.normal(size=(n, d)) * (0.3 if d > 8 else 1.0)).astype(np.float32)
    return coords, feats, spp, rng


@pytest.mark.parametrize("d", [6, 32])
def test_pool_edge_cases_in_one_call(d):
    from gapro_amd import gp_train_sets

    coords, feats, spp, rng = _scattered(d, (1 << 20) - 1)
    assert len(np.unique(spp)) == 257 and spp.max() - spp.min() == (1 << 20) - 2
    n = len(spp)
    perm = rng.permutation(n)
    one_spp = np.nonzero(spp == spp[5000])[0]
    shared = np.nonzero(spp == spp[9000])[0]
    assert len(one_spp) >= 2 and len(shared) >= 4
    some = perm[:700]
    problems = [
        (perm[:1], perm[1:12001], perm[12001:12500]),                    # a side of one point, a side of 12 000
        (rng.permutation(one_spp), perm[300:900], perm[:50]),            # a side entirely inside one superpoint
        (np.r_[shared[::2], perm[100:180]], np.r_[perm[500:640], shared[1::2]], shared),  # sides sharing a superpoint
        (np.r_[some, some[::-1]], perm[2000:2300], perm[:10]),           # every index listed twice
        (some, perm[2000:2300], np.zeros(0, np.int64)),                  # the same once; an empty intersection
    ]
    got = gp_train_sets(coords, feats, spp, problems)
    _same_sets(got, coords, feats, spp, problems, what="D=%d" % d)
    assert got[0][1] == 1 and got[1][1] == 1 and got[0][2] > 200
    assert np.array_equal(got[3][0][:got[3][1]], got[4][0][:got[4][1]])  # twice the points, the same means
    assert len(np.intersect1d(got[2][3], got[2][4])) >= 1


def test_an_id_range_beyond_the_rank_table_is_refused():
    from gapro_amd import gp_train_sets
    from gapro_amd._lib import GaproError

    coords, feats, spp, _ = _scattered(6, (1 << 20) + 1)
    with pytest.raises(GaproError) as e:
        gp_train_sets(coords, feats, spp, [(np.arange(10), np.arange(10, 30), np.arange(5))])
    assert e.value.code == -6  # SPP_RANGE


# ---------------------------------------------------------------------------------------------- 3. nearest
def _nearest_case(k):
    """Sides of k - 1, k, k + 1, 5 000 and 12 000 points (disjoint index ranges, shuffled lists), two intersections, and
    on each long side 50 points (25 nearer, 25 farther, where there are as many) moved onto the coordinates of its k-th
    nearest point: equal distances on both sides of the cut."""
    rng = np.random.default_rng(100 + k)
    sizes = [max(k - 1, 1), k, k + 1, 5000, 12000, k + 1]
    n_it = 3000
    n = n_it + sum(sizes)
    coords = rng.normal(scale=1.5, size=(n, 3))
    feats = rng.normal(size=(n, 6)).astype(np.float32)
    spp = rng.integers(0, 300, size=n).astype(np.int64)
    it_a, it_b = rng.permutation(n_it)[:2000], rng.permutation(n_it)[:1500]
    sides, base = [], n_it
    for s in sizes:
        sides.append(base + rng.permutation(s))
        base += s
    sides[5] = np.r_[sides[5], sides[5][:3]]  # three indices listed twice: ties of their own
    pairs = [(0, 1, it_a), (2, 3, it_a), (4, 5, it_b)]
    straddle = 0
    for a, b, it in pairs:
        c = R.centroid(coords, it)
        for side in (sides[a], sides[b]):
            if len(side) <= k:
                continue
            order = side[np.lexsort((np.arange(len(side)), R.distances(coords, side, c)))]  # nearest first
            nearer, beyond = np.unique(order[:k - 1]), np.unique(order[k:])
            movers = [rng.choice(x, size=min(25, len(x)), replace=False) for x in (nearer, beyond) if len(x)]
            coords[np.concatenate(movers)] = coords[order[k - 1]]
            d = np.sort(R.distances(coords, side, c))
            straddle += int(d[k - 1] == d[k])
    problems = [(sides[a], sides[b], it) for a, b, it in pairs]
    return coords, feats, spp, problems, straddle


@pytest.mark.parametrize("k", [1, 40, 800, 1024])
def test_nearest_selection_is_exact_order_included(k):
    from gapro_amd import gp_train_sets

    coords, feats, spp, problems, straddle = _nearest_case(k)
    assert straddle == 4  # on every long side the crafted ties sit on the cut
    got = gp_train_sets(coords, feats, spp, problems, npoint_nearest=k, spp_pool=False)
    _same_sets(got, coords, feats, spp, problems, k, False, what="k=%d" % k)
    assert [(g[1], g[2]) for g in got] == [(max(k - 1, 1), k), (k, k), (k, k)]


# ---------------------------------------------------------------------------------------------- 4. chain = parts
def _parts(coords, feats, spp, problems, k, pool):
    """The chain's result from existing calls: fit_gp_spp_batch on the restated table, predict_gp_batch at the points."""
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch, predict_gp_batch

    tables, fits, base = [], [], 0
    for prob in problems:
        x, m1, m2, _, _, _ = R.train_set(coords, feats, spp, prob, k, pool)
        tables.append(x)
        fits.append((base + np.arange(m1), base + m1 + np.arange(m2), base + np.arange(min(3, m1 + m2))))
        base += m1 + m2
    _, models = fit_gp_spp_batch(np.concatenate(tables), fits, training_iter=50, return_models=True)
    return predict_gp_batch(models, feats, [np.asarray(p[2], dtype=np.int64) for p in problems])


def _assert_chain_equals_parts(got, parts):
    assert len(got) == len(parts)
    for i, (g, p) in enumerate(zip(got, parts)):
        probs, probs_new, labels, var_b, mu, var = g
        assert np.array_equal(probs, p[0]) and np.array_equal(probs_new, p[1]) and np.array_equal(labels, p[2]), i
        assert np.array_equal(mu, p[3]) and np.array_equal(var, p[4]), i
        assert var_b.dtype == np.float32 and np.array_equal(var_b, p[0] * (np.float32(1) - p[0])), i


def test_chain_equals_its_parts_pooled_and_alone_equals_batch():
    from gapro_amd import fit_gp_batch

    coords, feats, spp, _, problems = R.golden_scene("s5_lean")
    got = fit_gp_batch(coords, feats, spp, problems, return_latent=True)
    _assert_chain_equals_parts(got, _parts(coords, feats, spp, problems, 800, True))
    alone = fit_gp_batch(coords, feats, spp, [problems[3]], return_latent=True)[0]
    for a, b in zip(alone, got[3]):
        assert np.array_equal(a, b)


def test_chain_equals_its_parts_nearest():
    from gapro_amd import fit_gp_batch

    coords, feats, spp, _, problems = R.golden_scene("s0_walls")
    got = fit_gp_batch(coords, feats, spp, problems, npoint_nearest=40, spp_pool=False, return_latent=True)
    _assert_chain_equals_parts(got, _parts(coords, feats, spp, problems, 40, False))


def test_chain_equals_its_parts_on_the_cluster_route():
    """Sides of 900 and 5 000 points at k = 800: M = 1 600 (the multi-workgroup kernel), T = 3 000."""
    from gapro_amd import _lib, fit_gp_batch
    from gapro_amd.synth import make_gp_problem

    feats, b1, b2, it = make_gp_problem(5, 900, 5000, 3000, 6)
    rng = np.random.default_rng(6)
    coords = rng.normal(size=(len(feats), 3))
    spp = rng.integers(0, 50, size=len(feats)).astype(np.int64)
    problems = [(rng.permutation(b1), rng.permutation(b2), it)]
    assert _lib.load().gapro_fit_route(1600, 6) == 4
    got = fit_gp_batch(coords, feats, spp, problems, npoint_nearest=800, spp_pool=False, return_latent=True)
    assert len(got[0][0]) == 3000
    _assert_chain_equals_parts(got, _parts(coords, feats, spp, problems, 800, False))


# ---------------------------------------------------------------------------------------------- 5. float64 oracle
@pytest.mark.parametrize("name,pair,pool,k,m,t", [("s0_walls", 1, True, 800, 26, 96), ("s5_lean", 3, True, 800, 49, 447),
                                                  ("s4_dups", 0, False, 40, 80, 297)])
def test_against_the_float64_oracle(name, pair, pool, k, m, t):
    from gapro_amd import fit_gp_batch
    from oracle import svgp_oracle as so

    coords, feats, spp, _, problems = R.golden_scene(name)
    prob = problems[pair]
    x, m1, m2, _, _, _ = R.train_set(coords, feats, spp, prob, k, pool)
    assert (m1 + m2, len(prob[2])) == (m, t)
    y = np.r_[-np.ones(m1), np.ones(m2)]
    mu_r, var_r, p_r = so.svgp_fit_predict_autograd(x.astype(np.float64), y, feats[prob[2]].astype(np.float64), 50, "f64")
    probs, probs_new, labels, var_b, mu, var = fit_gp_batch(coords, feats, spp, [prob], npoint_nearest=k, spp_pool=pool,
                                                            return_latent=True)[0]
    print("%s pair %d: var rel %.3e  mu abs %.3e  p abs %.3e" % (
        name, pair, np.max(np.abs(var - var_r) / var_r), np.max(np.abs(mu - mu_r)), np.max(np.abs(probs - p_r))))
    np.testing.assert_allclose(var, var_r, rtol=VAR_RTOL)
    np.testing.assert_allclose(mu, mu_r, rtol=MU_RTOL, atol=MU_ATOL)
    np.testing.assert_allclose(probs, p_r, rtol=0, atol=P_ATOL)
    safe = np.abs(p_r - 0.5) > 1e-6
    np.testing.assert_array_equal(labels[safe], (p_r.astype(np.float32) >= np.float32(0.5))[safe])
    np.testing.assert_array_equal(probs_new, np.where(labels, probs, np.float32(1) - probs))
    np.testing.assert_array_equal(var_b, probs * (np.float32(1) - probs))


# ---------------------------------------------------------------------------------------------- 6. status, fit_gp
def test_a_nan_feature_fails_its_problem_alone():
    from gapro_amd import fit_gp_batch, gp_train_sets
    from gapro_amd._lib import GaproError

    coords, feats, spp, _, problems = R.golden_scene("s0_walls")
    problems = problems[:4]
    clean, st0 = fit_gp_batch(coords, feats, spp, problems, npoint_nearest=40, spp_pool=False, return_status=True)
    assert (st0 == 0).all()
    sets = gp_train_sets(coords, feats, spp, problems, npoint_nearest=40, spp_pool=False)
    others = np.concatenate([np.r_[s[3], s[4]] for i, s in enumerate(sets) if i != 2] +
                            [np.concatenate(p) for i, p in enumerate(problems) if i != 2])
    mine = np.setdiff1d(np.r_[sets[2][3], sets[2][4]], others)  # a row of problem 2 that no other problem reads
    assert len(mine)
    bad = feats.copy()
    bad[mine[0], 4] = np.nan
    got, st = fit_gp_batch(coords, bad, spp, problems, npoint_nearest=40, spp_pool=False, return_status=True)
    assert st[2] == R.NOT_FINITE and (np.delete(st, 2) == 0).all()
    for i in (0, 1, 3):
        for a, b in zip(got[i], clean[i]):
            assert np.array_equal(a, b), i
    for call in (gp_train_sets, fit_gp_batch):
        with pytest.raises(GaproError) as e:
            call(coords, bad, spp, problems, npoint_nearest=40, spp_pool=False)
        assert e.value.code == R.NOT_FINITE
    with pytest.raises(GaproError):  # pooling: the whole input is refused, as the generator refuses it
        fit_gp_batch(coords, bad, spp, problems)


@pytest.mark.parametrize("value", [np.inf, -np.inf, np.nan])
def test_a_non_finite_coordinate_fails_the_problems_that_meet_it_alone(value):
    """The centroid's fixed-point scale comes from the finite coordinates: an infinite coordinate somewhere in the input
    must not round the other problems' centroids (and with them their selections) to another grid."""
    from gapro_amd import fit_gp_batch, gp_train_sets

    coords, feats, spp, _, problems = R.golden_scene("s0_walls")
    problems = problems[:4]
    kw = dict(npoint_nearest=40, spp_pool=False)
    assert all(max(len(p[0]), len(p[1])) > 40 for p in problems)  # every problem needs its centroid
    clean, st0 = fit_gp_batch(coords, feats, spp, problems, return_status=True, **kw)
    assert (st0 == 0).all()
    free = np.setdiff1d(np.arange(len(coords)), np.concatenate([np.concatenate(p) for p in problems]))
    mine = np.setdiff1d(np.concatenate(problems[2]),
                        np.concatenate([np.concatenate(p) for i, p in enumerate(problems) if i != 2]))
    assert len(free) and len(mine)
    nobody = coords.copy()
    nobody[free[0], 1] = value  # a point of no problem: nothing changes
    _same_sets(gp_train_sets(nobody, feats, spp, problems, **kw), nobody, feats, spp, problems, 40, False)
    got, st = fit_gp_batch(nobody, feats, spp, problems, return_status=True, **kw)
    assert (st == 0).all()
    for g, c in zip(got, clean):
        for a, b in zip(g, c):
            assert np.array_equal(a, b)
    one = coords.copy()
    one[mine[0], 0] = value  # a point of problem 2 alone
    got, st = fit_gp_batch(one, feats, spp, problems, return_status=True, **kw)
    assert list(st) == [0, 0, R.NOT_FINITE, 0]
    for i in (0, 1, 3):
        for a, b in zip(got[i], clean[i]):
            assert np.array_equal(a, b), i


@pytest.mark.parametrize("pool", [True, False])
def test_fit_gp_returns_the_documented_tensors(pool):
    import torch

    from gapro_amd import fit_gp, fit_gp_batch

    coords, feats, spp, _, problems = R.golden_scene("s0_walls")
    b1, b2, it = problems[1]
    dev = torch.device("cuda:0")
    args = (torch.from_numpy(coords).to(dev), torch.from_numpy(feats).to(dev), torch.from_numpy(spp).to(dev),
            torch.from_numpy(b1).to(dev), torch.from_numpy(b2).to(dev), torch.from_numpy(it).to(dev))
    out = fit_gp(*args, 50, 40, pool)
    assert len(out) == 4 and all(o.device.type == "cuda" and o.shape == (len(it),) for o in out)
    assert [o.dtype for o in out] == [torch.float32, torch.float32, torch.bool, torch.float32]
    ref = fit_gp_batch(coords, feats, spp, [problems[1]], 50, 40, pool)[0]
    for o, r in zip(out, ref):
        assert np.array_equal(o.cpu().numpy(), r)
    cpu = fit_gp(coords.astype(np.float32).astype(np.float64), feats, spp, b1, b2, it, spp_pool=pool)
    assert all(isinstance(o, torch.Tensor) for o in cpu)
