"""The scene-partition kernels at their kernel-variant, bit-word, rounding and scan edges, bit for bit against the oracle.

The inputs come from partition_cases.py; test_partition_edges_cpu.py proves on the oracle alone that each is what it
claims (the pooling variant it takes, occupancy bits past word 0, runs that overflow / fit the LDS table, quotients that
a double division would decide differently), so that nothing here passes vacuously."""
import numpy as np
import pytest

import partition_cases as pc
from partition_cases import _check_against_oracle, _run_partition

pytestmark = pytest.mark.gpu


def _plan(d, boxes):
    from gapro_amd import _lib

    return _lib.load().gapro_partition_pool_plan(d, boxes)


# ------------------------------------------------------------------------------------------ kernel variants, bit words
@pytest.mark.parametrize("case", pc.SWEEP, ids=pc.SWEEP_IDS)
def test_every_pool_variant_and_word_count(case):
    kw = pc.sweep_scene(case)
    assert _plan(case.d, case.boxes) == case.plan
    pipe, job = _run_partition(kw, pc.SWEEP_THRESH)
    assert job.n_boxes == case.boxes
    _check_against_oracle(kw, job, pc.SWEEP_THRESH)


def test_most_boxes_the_lds_holds_and_one_more():
    from gapro_amd._lib import GaproError

    kw = pc.grid_scene(31, 3000, pc.LIMIT_BOXES - 1, 6, 0.25, "shuffled")
    assert _plan(6, pc.LIMIT_BOXES) == 0
    pipe, job = _run_partition(kw, pc.SWEEP_THRESH)
    assert job.n_boxes == pc.LIMIT_BOXES
    part = _check_against_oracle(kw, job, pc.SWEEP_THRESH)
    assert part.occ_spp[:, 1344:].any()  # the 22nd word
    kw = pc.grid_scene(31, 3000, pc.LIMIT_BOXES, 6, 0.25, "shuffled")
    with pytest.raises(GaproError) as e:
        _run_partition(kw, pc.SWEEP_THRESH)
    assert e.value.code == -1


@pytest.mark.parametrize("d,n,cell", pc.WIDTH_TAILS)
def test_feature_widths_and_run_tails(d, n, cell):
    kw = pc.width_tail_scene(d, n, cell)
    pipe, job = _run_partition(kw, pc.SWEEP_THRESH)
    assert job.n_points == n and job.feats.shape[1] == d
    _check_against_oracle(kw, job, pc.SWEEP_THRESH)


# ------------------------------------------------------------------------------------------ batches
def _pool_batch(pipe, jobs, tasks, d_tasks, d):
    import torch

    base = 0
    for job in jobs:
        job.feats_row_base = base
        base += job.n_spps
    feats_spp_all = torch.empty((base, d), dtype=torch.float32, device=pipe.device)
    pipe._pool_all(jobs, tasks, d_tasks, feats_spp_all)
    torch.cuda.synchronize()


def test_ragged_batch_across_variants():
    """One launch over scenes of 4, 71 and 201 boxes: the table is sized for the largest (nb_cap = 201, 32 slots) while
    every scene indexes its rows by its own box count and word count."""
    from gapro_amd.pipeline import Pipeline

    kws = [pc.grid_scene(51, 5000, 3, 6, 0.5, "coherent"), pc.grid_scene(52, 3000, 70, 6, 0.25, "shuffled"),
           pc.grid_scene(53, 6000, 200, 6, 0.5, "coherent")]
    assert [_plan(6, nb) for nb in (4, 71, 201)] == [6, 6, 5]
    pipe = Pipeline(device=0, training_iter=0)
    jobs = [pc.make_partition_job(kw, pc.SWEEP_THRESH) for kw in kws]
    tasks, d_tasks = pipe._prepare_all(jobs)
    _pool_batch(pipe, jobs, tasks, d_tasks, 6)
    assert [j.n_boxes for j in jobs] == [4, 71, 201]
    for kw, job in zip(kws, jobs):
        _check_against_oracle(kw, job, pc.SWEEP_THRESH)


def test_non_finite_scenes_are_reported_inside_a_batch():
    """strict = False: a scene with one NaN feature and one with one infinite coordinate get GAPRO_ERR_NOT_FINITE (-4) and
    leave the batch; the scenes around them are bit-exact."""
    from gapro_amd.pipeline import Pipeline

    kws = [pc.grid_scene(61 + i, 2500 + 300 * i, 4 + i, 6, 0.5, "coherent") for i in range(4)]
    kws[1]["mask_feats"][1234, 3] = np.nan
    kws[3]["coords_float"][77, 1] = np.inf
    pipe = Pipeline(device=0, training_iter=0)
    pipe.strict = False
    jobs = [pc.make_partition_job(kw, pc.SWEEP_THRESH) for kw in kws]
    tasks, d_tasks = pipe._prepare_all(jobs)
    assert [None if j.error is None else j.error.code for j in jobs] == [None, -4, None, -4]
    good = [j for j in jobs if j.error is None]
    _pool_batch(pipe, good, tasks, d_tasks, 6)
    for i in (0, 2):
        _check_against_oracle(kws[i], jobs[i], pc.SWEEP_THRESH)


# ------------------------------------------------------------------------------------------ the two float32 decisions
@pytest.mark.parametrize("thresh", pc.LADDER_THRESHOLDS, ids=lambda t: "%.4g" % t)
def test_fraction_ladder(thresh):
    """(float)count / (float)points >= thresh for every count / points with points <= 40, 999 and 998 of 1000, 1 and 2 of
    3: occ_bits, n_bbs and occ_count (and everything else) against the oracle's float32 division."""
    kw = pc.ladder_scene()
    pipe, job = _run_partition(kw, thresh)
    part = _check_against_oracle(kw, job, thresh)
    pairs = np.array(pc.ladder_pairs())
    n, k = pairs[:, 0], pairs[:, 1]
    got = pc.unpack_bits(job.dev["occ_bits"].cpu().numpy(), 2)[:, 0]
    np.testing.assert_array_equal(got, k.astype(np.float32) / n.astype(np.float32) >= np.float32(thresh))
    np.testing.assert_array_equal(job.dev["occ_count"].cpu().numpy()[:, 0], k)
    np.testing.assert_array_equal(job.dev["n_bbs"].cpu().numpy(), part.occ_spp.sum(1))


@pytest.mark.parametrize("b,mode", pc.FACE_CASES)
def test_points_on_and_next_to_the_six_faces(b, mode):
    """Closed interval against float64(float32 corner) -+ 0.005: on the face is inside, its inner float64 neighbour is
    inside, its outer neighbour is outside; for a box in word 0, at its last bit, and in word 1, and in each of the four
    copies of the interval test (partition_cases.FACE_CASES)."""
    kw, want, rank, rep = pc.face_scene(b, mode)
    n_inst = len(kw["instance_box"])
    assert _plan(6, n_inst + 1) == (0 if mode == "k_pool" else 6)
    pipe, job = _run_partition(kw, 0.5)
    _check_against_oracle(kw, job, 0.5)
    occ = pc.unpack_bits(job.dev["occ_bits"].cpu().numpy(), n_inst + 1)
    np.testing.assert_array_equal(occ[rank, b], want)
    assert not np.delete(occ[:, :n_inst], b, axis=1).any()
    np.testing.assert_array_equal(job.dev["occ_count"].cpu().numpy()[rank, b], want.astype(np.int32) * rep)


# ------------------------------------------------------------------------------------------ fixed-point pooling
def _pooling_scene(feats, layout, n_boxes=2):
    """Points on a line; superpoints by `layout`: "blocks" = 64 consecutive points each (whole waves of one superpoint: the
    shuffle-reduced branch), "strided16" = id i % 16 (per-point branch, the table holds them all), "strided512" = id
    i % 512 (more superpoints than slots: the global-atomics branch of k_pool_lds)."""
    n = len(feats)
    i = np.arange(n)
    spp = {"blocks": i // 64, "strided16": i % 16, "strided512": i % 512}[layout]
    coords = np.stack([i * (3.0 / max(n, 2)), np.full(n, 0.5), np.full(n, 0.5)], 1)
    box = np.tile(np.array([[0, 0, 0, 1, 1, 1]], np.float32), (n_boxes, 1))
    box[:, 0] += np.arange(n_boxes, dtype=np.float32) * 0.5
    box[:, 3] += np.arange(n_boxes, dtype=np.float32) * 0.5
    return pc.boxes_kw(coords, feats, spp, box)


def _tie_features(n=1024):
    """float32[n, 4] with |f|max = 1 (shift 50 at n = 1024).  Column 0: m 2^-51 for odd m of both signs, every one a tie
    of the rounding to 2^-50 (to even: (m +- 1) / 2, whichever is even).  Column 1: +x / -x in points i and i + 512
    (the same superpoint in every layout but "blocks", where i and i ^ 1 are paired): the sum is exactly 0.  Column 2:
    one 1.0.  Column 3: 3/4 and 1/4 of the grid step, which truncation and rounding take apart."""
    rng = np.random.default_rng(8)
    f = np.zeros((n, 4), np.float64)
    m = 2 * rng.integers(-2 ** 20, 2 ** 20, n) + 1
    f[:, 0] = np.ldexp(m.astype(np.float64), -51)
    x = (rng.standard_normal(n // 2) * 0.3).astype(np.float32).astype(np.float64)
    f[:n // 2, 1], f[n // 2:, 1] = x, -x
    f[5, 2] = 1.0
    f[:, 3] = np.ldexp(4.0 * rng.integers(-1000, 1000, n) + rng.choice([1.0, 3.0], n), -52)
    out = f.astype(np.float32)
    assert (out.astype(np.float64) == f).all() and np.abs(out).max() == 1.0
    return out


@pytest.mark.parametrize("layout,n_boxes", [("blocks", 2), ("strided16", 2), ("strided512", 2), ("strided16", 600)])
def test_pooling_rounds_ties_to_even_in_every_kernel_branch(layout, n_boxes):
    """With 600 boxes the pass runs on k_pool, otherwise on one of the three branches of k_pool_lds."""
    from oracle import gen_ps_oracle as O

    f = _tie_features()
    if layout == "blocks":  # pair +x / -x inside a block of 64
        f[:, 1] = np.where(np.arange(len(f)) % 2 == 0, 1, -1) * np.abs(np.repeat(f[0::2, 1], 2))
    kw = _pooling_scene(f, layout, n_boxes)
    assert _plan(4, n_boxes + 1) == (0 if n_boxes == 600 else 6)
    assert O.fixed_point_shift(1.0, 1024) == 50
    q = np.ldexp(f.astype(np.float64), 50)
    assert (np.abs(q[:, 0] - np.trunc(q[:, 0])) == 0.5).all()  # every one a tie
    pipe, job = _run_partition(kw, 0.8)
    part = _check_against_oracle(kw, job, 0.8)
    assert int(job.header.fixed_shift) == 50
    got = job.dev["feats_spp"].cpu().numpy()
    assert (got[:, 1] == 0).all()  # the pairs cancel exactly
    # what the test can tell apart: truncation, and rounding half away from zero, give other float32 means
    S, cnt = part.n_spps, part.point_count.astype(np.float64)
    for other in (np.trunc, lambda v: np.sign(v) * np.floor(np.abs(v) + 0.5)):
        sums = np.zeros((S, 4))
        np.add.at(sums, part.spp_inv, other(q))
        alt = (np.ldexp(sums, -50) / cnt[:, None]).astype(np.float32)
        assert (alt[:, 0] != got[:, 0]).any() or (alt[:, 3] != got[:, 3]).any()
    sums = np.zeros((S, 4))
    np.add.at(sums, part.spp_inv, np.trunc(q))
    assert ((np.ldexp(sums, -50) / cnt[:, None]).astype(np.float32)[:, 3] != got[:, 3]).any()


@pytest.mark.parametrize("n", [1, 2, 1024, 1025])
def test_fixed_shift_at_powers_of_two(n):
    """The shift drops by one from n = 2^k to 2^k + 1 points (61 - exponent - ceil(log2 n)): |f|max = 1 gives 60, 59, 50,
    49."""
    rng = np.random.default_rng(n)
    f = rng.uniform(-1, 1, (n, 6)).astype(np.float32)
    f[n // 2, 2] = -1.0
    kw = _pooling_scene(f, "strided16")
    pipe, job = _run_partition(kw, 0.8)
    _check_against_oracle(kw, job, 0.8)
    assert int(job.header.fixed_shift) == {1: 60, 2: 59, 1024: 50, 1025: 49}[n]


@pytest.mark.parametrize("kind", ["span", "zero", "huge", "denormal"])
def test_pooling_at_extreme_magnitudes(kind):
    """Columns from 2^-40 to 2^20 in one scene (the small ones lose bits to the common shift, exactly as the oracle's),
    all-zero features (shift 0), |f|max = 3e38 (a negative shift) and = 1e-45 (the smallest denormal, shift 209 - 11)."""
    from oracle import gen_ps_oracle as O

    n = 1500
    rng = np.random.default_rng(3)
    if kind == "span":
        f = rng.uniform(-1, 1, (n, 6)) * np.ldexp(1.0, [-40, -28, -16, 0, 10, 20])[None, :]
        f[7, 5] = np.ldexp(1.0, 20)
        shift = 61 - 21 - 11
    elif kind == "zero":
        f = np.zeros((n, 6))
        shift = 0
    elif kind == "huge":
        f = rng.uniform(-1, 1, (n, 6)) * 3e38
        f[11, 0] = 3e38
        shift = 61 - 128 - 11
    else:
        f = np.zeros((n, 6))
        f[:, 0] = np.where(np.arange(n) < 640, 1, rng.integers(-1, 2, n)) * 1e-45  # ten superpoints of mean 2^-149
        f[3, 1] = 1e-45
        shift = 61 + 148 - 11
    f = f.astype(np.float32)
    assert O.fixed_point_shift(float(np.abs(f).max()), n) == shift
    kw = _pooling_scene(f, "blocks")
    pipe, job = _run_partition(kw, 0.8)
    part = _check_against_oracle(kw, job, 0.8)
    assert int(job.header.fixed_shift) == shift
    assert np.isfinite(part.feats_spp).all() and (kind == "zero") == (not part.feats_spp.any())
    if kind == "denormal":
        assert (part.feats_spp[:10, 0] == np.float32(1e-45)).all() and np.float32(1e-45) > 0


# ------------------------------------------------------------------------------------------ the rank scan
def _id_scene(ids, n_boxes=2, seed=0):
    rng = np.random.default_rng(seed)
    n = len(ids)
    coords = rng.uniform(0, 3, (n, 3))
    box = np.array([[0, 0, 0, 1.5, 1.5, 1.5], [1, 1, 1, 2.5, 2.5, 2.5]], np.float32)[:n_boxes]
    return pc.boxes_kw(coords, rng.standard_normal((n, 6)), ids, box)


def _ids_of_range(rng, n, id_range, base=0):
    ids = rng.integers(0, id_range, n)
    ids[rng.integers(0, n)] = 0
    if id_range > 1:
        ids[(np.flatnonzero(ids == 0)[0] + 1) % n] = id_range - 1
    assert ids.max() - ids.min() + 1 == id_range
    return ids.astype(np.int64) + base


@pytest.mark.parametrize("id_range,cap", [(1, None), (2048, None), (2049, None), (524288, None), (524289, None),
                                          (1200001, 1 << 21)])
def test_rank_scan_at_chunk_and_carry_edges(id_range, cap):
    """Id ranges of exactly one scan chunk (2048) and one more, of exactly 256 chunks (one iteration of k_scan_offsets)
    and one more (the carry), and of 586 chunks."""
    rng = np.random.default_rng(id_range % 1000)
    kw = _id_scene(_ids_of_range(rng, 4000, id_range, base=-1234))
    pipe, job = _run_partition(kw, 0.8, spp_range_cap=cap)
    part = _check_against_oracle(kw, job, 0.8)
    assert job.n_spps == len(np.unique(kw["spp"])) and (id_range == 1) == (part.n_spps == 1)


@pytest.mark.parametrize("where", ["sparse_negative", "int64_min", "int64_max"])
def test_rank_scan_at_the_ends_of_int64(where):
    rng = np.random.default_rng(12)
    off = rng.integers(0, 50, 3000).astype(np.int64)
    if where == "sparse_negative":
        ids = off * 7919 - 300000
    elif where == "int64_min":
        ids = pc.INT64_MIN + off
    else:
        ids = pc.INT64_MAX - off
    kw = _id_scene(ids)
    pipe, job = _run_partition(kw, 0.8)
    _check_against_oracle(kw, job, 0.8)
    if where == "int64_min":
        assert job.header.spp_min <= pc.INT64_MIN + 50
    if where == "int64_max":
        assert job.header.spp_max >= pc.INT64_MAX - 50


def test_both_ends_of_int64_in_one_scene_is_a_range_error():
    from gapro_amd._lib import GaproError

    ids = np.where(np.arange(500) % 2 == 0, pc.INT64_MIN + 3, pc.INT64_MAX - 3).astype(np.int64)
    with pytest.raises(GaproError) as e:
        _run_partition(_id_scene(ids), 0.8)
    assert e.value.code == -6


def test_range_cap_boundary():
    """spp_range_cap = 4096: max - min = 4095 is the last range the table holds; 4096 is GAPRO_ERR_SPP_RANGE."""
    from gapro_amd._lib import GaproError

    rng = np.random.default_rng(2)
    kw = _id_scene(_ids_of_range(rng, 3000, 4096, base=10))
    assert int(kw["spp"].max() - kw["spp"].min()) == 4095
    pipe, job = _run_partition(kw, 0.8, spp_range_cap=4096)
    _check_against_oracle(kw, job, 0.8)
    kw = _id_scene(_ids_of_range(rng, 3000, 4097, base=10))
    with pytest.raises(GaproError) as e:
        _run_partition(kw, 0.8, spp_range_cap=4096)
    assert e.value.code == -6


def test_long_scene_passes_every_grid_stride_bound():
    """525 000 points (more than the 262 144 threads of k_stats' grid and the 524 288 of k_flags' / k_rank_lookup's), ids
    spread over 600 000 (the scan's carry), shuffled."""
    rng = np.random.default_rng(44)
    n = 525000
    ids = rng.integers(0, 600000, n).astype(np.int64)
    coords = rng.uniform(0, 3, (n, 3))
    box = np.array([[0, 0, 0, 1.5, 1.5, 1.5], [1, 1, 1, 2.5, 2.5, 2.5], [0.5, 0, 2, 3, 1, 3], [2, 2, 0, 3, 3, 1]], np.float32)
    kw = pc.boxes_kw(coords, (3 * rng.standard_normal((n, 6))), ids, box)
    # the extreme coordinates, ids and feature sit in the last points: only the grid-stride loops' later trips see them
    kw["coords_float"][-3:] = [[-1.0, 0.5, 0.5], [0.5, 4.0, 0.5], [0.5, 0.5, -2.0]]
    kw["spp"][-2:] = [-5, 600004]
    kw["mask_feats"][-1, 4] = 100.0
    pipe, job = _run_partition(kw, 0.5)
    assert job.n_boxes == 5
    _check_against_oracle(kw, job, 0.5)
