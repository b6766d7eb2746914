"""The inputs of test_partition_edges_gpu.py really are what that file claims (oracle only, no device), the pooling
plan query at every boundary, and the host scheduler and merge on occupancy rows of more than one 64-bit word."""
import ctypes as C
import os
import subprocess
import sys

from functools import lru_cache

import numpy as np
import pytest

import partition_cases as pc
from gapro_amd import _lib
from oracle import gen_ps_oracle as O
from test_host_golden import _occ_bits, _p

BAD_ARG = -1


# ------------------------------------------------------------------------------------------ the pooling plan
def _plan_rule(d, nb):
    """The 60 KiB rule restated: 48 bytes of corners per box beside a table of 64, 32 or 16 slots of
    {key, count, nb occupancy counts, d 64-bit sums}; corners alone may take the whole 64 KiB (global atomics)."""
    if d <= 0 or nb <= 0 or 48 * nb > 64 * 1024:
        return BAD_ARG
    for log2_slots in (6, 5, 4):
        if 48 * nb + (8 + 4 * nb + 8 * d) * (1 << log2_slots) <= 60 * 1024:
            return log2_slots
    return 0


@pytest.mark.parametrize("d,below,above", [
    (6, (190, 6), (191, 5)), (6, (338, 5), (339, 4)), (6, (540, 4), (541, 0)), (6, (1365, 0), (1366, BAD_ARG)),
    (32, (146, 6), (147, 5)), (32, (301, 5), (302, 4)), (32, (510, 4), (511, 0)), (32, (1365, 0), (1366, BAD_ARG))])
def test_pool_plan_on_both_sides_of_every_boundary(d, below, above):
    lib = _lib.load()
    for nb, want in (below, above):
        assert lib.gapro_partition_pool_plan(d, nb) == want == _plan_rule(d, nb), (d, nb)


def test_pool_plan_agrees_with_the_lds_rule_everywhere():
    lib = _lib.load()
    for d in (1, 3, 6, 7, 8, 9, 32, 33, 64, 256, 2000):
        got = [lib.gapro_partition_pool_plan(d, nb) for nb in range(1, 1400)]
        assert got == [_plan_rule(d, nb) for nb in range(1, 1400)], d
    for d, nb in ((0, 5), (-1, 5), (6, 0), (6, -3), (6, 2 ** 31 - 1), (2 ** 31 - 1, 1)):
        assert lib.gapro_partition_pool_plan(d, nb) == (BAD_ARG if min(d, nb) <= 0 or nb > 1365 else 0), (d, nb)


def test_pool_plan_honours_the_global_atomics_switch():
    """GAPRO_POOL_GLOBAL_ATOMICS is read once per process, as the launcher reads it: a fresh process with it set."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("from gapro_amd import _lib; lib = _lib.load(); "
            "assert [lib.gapro_partition_pool_plan(6, nb) for nb in (1, 190, 541, 1365, 1366)] == [0, 0, 0, 0, -1]")
    env = dict(os.environ, GAPRO_POOL_GLOBAL_ATOMICS="1")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=root, env=env)


# ------------------------------------------------------------------------------------------ the case tables
@pytest.mark.parametrize("case", pc.SWEEP, ids=pc.SWEEP_IDS)
def test_sweep_case_is_what_it_claims(case):
    lib = _lib.load()
    assert lib.gapro_partition_pool_plan(case.d, case.boxes) == case.plan
    kw = pc.sweep_scene(case)
    boxes, _, _, part = pc.oracle_partition(kw, pc.SWEEP_THRESH)
    assert len(boxes) == case.boxes
    spp, n = kw["spp"], len(kw["spp"])
    per_run = [len(np.unique(spp[i:i + pc.K_POOL_RUN])) for i in range(0, n, pc.K_POOL_RUN)]
    if case.order == "coherent":  # the shuffle-reduced branch: eight consecutive points of one superpoint are common
        assert n / part.n_spps >= 16 and max(per_run) <= 48, (n / part.n_spps, per_run)
        assert (np.diff(spp) >= 0).all()
    else:  # every run overflows its table: the global-atomics branch of k_pool_lds
        assert min(per_run) > (1 << max(case.plan, 4)), per_run
    assert part.occ_spp[:, -1].sum() >= 5  # the last bit of the last word is in use
    if case.boxes > 64:
        high = part.occ_spp[:, 64:].any(1)
        assert high.sum() >= 5
        words = np.stack([part.occ_spp[:, w:w + 64].any(1) for w in range(0, case.boxes, 64)], 1)
        assert (words.sum(1) >= 2).any()  # a superpoint with bits in two different words


def test_sweep_covers_every_tier_and_word_edge():
    assert {(c.d, c.plan) for c in pc.SWEEP} == {(d, p) for d in (6, 32) for p in (6, 5, 4, 0)}
    assert {63, 64, 65, 128, 129} <= {c.boxes for c in pc.SWEEP if c.d == 6}
    lib = _lib.load()
    assert lib.gapro_partition_pool_plan(6, pc.LIMIT_BOXES) == 0
    assert lib.gapro_partition_pool_plan(6, pc.LIMIT_BOXES + 1) == BAD_ARG


@pytest.mark.parametrize("d,n,cell", pc.WIDTH_TAILS)
def test_width_and_tail_cases(d, n, cell):
    kw = pc.width_tail_scene(d, n, cell)
    assert kw["mask_feats"].shape == (n, d) and _lib.load().gapro_partition_pool_plan(d, 6) == 6
    spp = kw["spp"]
    if cell == 1.0:  # 32 superpoints: whole waves of eight points share one (the shuffle-reduced branch at this width)
        runs = np.diff(np.flatnonzero(np.r_[True, np.diff(spp) != 0, True]))
        assert n / len(np.unique(spp)) >= 16 and (runs >= 16).sum() >= 16


def test_width_and_tail_table_covers_what_it_must():
    half = [(d, n) for d, n, cell in pc.WIDTH_TAILS if cell == 0.5]
    assert {d for d, _ in half} == {1, 3, 7, 8, 9, 33}
    assert [n for _, n in half] == [1, 7, 8, 9, 1023, 1024, 1025, 2049]
    # a run of k_pool_lds that ends off a multiple of eight points, and one that does not
    assert any(n % pc.K_POOL_RUN % 8 for _, n in half) and any(n % pc.K_POOL_RUN % 8 == 0 for _, n in half)


def test_fraction_ladder_separates_float32_division_from_its_neighbours():
    """Per threshold t, with t32 = float32(t) as the kernel receives it:

    * some superpoint's float32 quotient EQUALS t32 (the closed side of >=);
    * where t32 > t (0.6, 0.8, 0.999, 1/3) the superpoint with k / n = t exactly has a float32 quotient that rounds up to
      t32 and a float64 quotient below it: a division in double decides it differently.  Where t32 <= t no (n, k) can do
      that: rounding to float32 is monotone, so the two quotients part only for k / n in [t32 - ulp / 2, t32), which at
      t = 0.7 (t32 = 0.7 - 1.2e-8) needs k / n != 7 / 10 within 4.2e-8 of it, i.e. n > 2 000 000 points in one
      superpoint; 0.5 and 1.0 are exact in both formats.  That impossibility is asserted for the ladder;
    * some superpoint's quotient differs from count * (1 / points) in float32 on the two sides of some threshold."""
    pairs = np.array(pc.ladder_pairs())
    n, k = pairs[:, 0], pairs[:, 1]
    q32 = k.astype(np.float32) / n.astype(np.float32)
    q64 = k.astype(np.float64) / n.astype(np.float64)
    recip = k.astype(np.float32) * (np.float32(1) / n.astype(np.float32))
    assert q32.dtype == np.float32 and recip.dtype == np.float32
    recip_differs = False
    for t in pc.LADDER_THRESHOLDS:
        t32 = np.float32(t)
        assert (q32 == t32).any(), t
        differs = (q32 >= t32) != (q64 >= np.float64(t32))
        if t in (0.5, 1.0):
            assert not differs.any()
        elif np.float64(t32) > t:
            assert differs.any(), t
        else:
            assert t == 0.7 and not differs.any()
        recip_differs |= bool(((q32 >= t32) != (recip >= t32)).any())
    assert (q32[(n == 1000) & (k == 999)] == np.float32(0.999)).all()
    assert recip_differs
    # the scene holds exactly these superpoints
    kw = pc.ladder_scene()
    _, _, _, part = pc.oracle_partition(kw, 0.5)
    np.testing.assert_array_equal(part.point_count, n)
    np.testing.assert_array_equal(part.occ_count[:, 0], k)


@pytest.mark.parametrize("b,mode", pc.FACE_CASES)
def test_face_scene_membership_is_what_the_construction_dictates(b, mode):
    kw, want, rank, rep = pc.face_scene(b, mode)
    assert want.sum() == 12 and len(want) == 18
    boxes, _, _, part = pc.oracle_partition(kw, 0.5)
    n_inst = len(kw["instance_box"])
    assert len(boxes) == n_inst + 1 and n_inst == (600 if mode == "k_pool" else pc.FACE_N_BOXES)
    assert _lib.load().gapro_partition_pool_plan(6, n_inst + 1) == (0 if mode == "k_pool" else 6)
    np.testing.assert_array_equal(part.occ_spp[rank, b], want)
    np.testing.assert_array_equal(part.occ_count[rank, b], want * rep)
    assert not np.delete(part.occ_spp[:, :n_inst], b, axis=1).any()
    if mode == "waves":  # whole waves of eight points of one superpoint
        assert (kw["spp"].reshape(-1, 8) == kw["spp"][::8, None]).all()
    if mode == "crowded":  # the table of 64 slots is full before the probe points come
        assert len(np.unique(kw["spp"][:-18])) == 600 and part.n_spps == 618


def test_face_cases_cover_the_issue_set_boxes():
    assert [b for b, mode in pc.FACE_CASES if mode == "own"] == [0, 63, 64, 65]
    assert {mode for _, mode in pc.FACE_CASES} == {"own", "waves", "crowded", "k_pool"}


# ------------------------------------------------------------------------------------------ scheduler + merge, W > 1
SCHED_TOTALS = (64, 65, 128, 129)


def _synthetic_fit_results(events, seed):
    """Seeded stand-ins for the GP outputs of every fit event: float32 probs_new in (0.5, 1), random labels, mu, var."""
    rng = np.random.default_rng(seed)
    res = []
    for e in events:
        if e.kind != "fit":
            continue
        m = len(e.intersect_inds)
        p_new = rng.uniform(0.5, 1.0, m).astype(np.float32)
        p_new = np.where(p_new <= np.float32(0.5), np.float32(0.75), p_new)
        res.append((p_new.copy(), p_new, rng.integers(0, 2, m).astype(np.uint8), rng.standard_normal(m).astype(np.float32),
                    rng.uniform(0.1, 2.0, m).astype(np.float32)))
    return res


@lru_cache(maxsize=None)
def _sched_case(total):
    """The oracle's side of one case: a grid scene with `total` boxes (floor included), its schedule, synthetic fit
    results and the merged state.  Every instance box is foreground: n_fg_instances = 63 and 64 sit below / at the word
    edge, 127 and 128 above it."""
    kw = pc.grid_scene(400 + total, 6000, total - 1, 6, 0.25, "shuffled")
    boxes, cls, vol, part = pc.oracle_partition(kw, 0.8)
    events = O.enumerate_schedule(boxes, part.occ_spp, part.n_bbs_per_spp)
    results = _synthetic_fit_results(events, total)
    n_fg = total - 1
    _, state = O.merge_and_label(part, events, results, n_fg_instances=n_fg)
    return boxes, cls, vol, part, events, results, n_fg, state


@pytest.mark.parametrize("total", SCHED_TOTALS)
def test_cxx_schedule_and_merge_on_multiword_rows(total):
    """gapro_schedule_build / _export_fits / _export_events / _merge on the oracle's occupancy of a grid scene with
    `total` boxes (floor included; W = 1, 2, 2, 3 words per row): events, index sets and their order against
    O.enumerate_schedule, the merged per-superpoint tables against O.merge_and_label on the same synthetic fit results."""
    lib = _lib.load()
    boxes, cls, vol, part, events, results, n_fg, state = _sched_case(total)
    assert len(boxes) == total
    fits = [e for e in events if e.kind == "fit"]
    bits = np.ascontiguousarray(_occ_bits(part.occ_spp))
    assert bits.shape[1] == (total + 63) // 64
    n_bbs = np.ascontiguousarray(part.n_bbs_per_spp.astype(np.int32))
    boxes = np.ascontiguousarray(boxes)
    sched = C.c_void_p()
    assert lib.gapro_schedule_build(part.n_spps, total, _p(boxes), _p(bits), _p(n_bbs), C.byref(sched)) == 0
    try:
        cnt = _lib.ScheduleCounts()
        assert lib.gapro_schedule_get_counts(sched, C.byref(cnt)) == 0
        assert (cnt.n_fits, cnt.n_events) == (len(fits), len(events))
        assert cnt.n_fit_out == sum(len(e.intersect_inds) for e in fits)
        descs = (_lib.FitDesc * max(cnt.n_fits, 1))()
        idx = np.zeros(max(cnt.n_fit_idx, 1), dtype=np.int32)
        assert lib.gapro_schedule_export_fits(sched, 0, 0, 0, 3, C.cast(descs, C.c_void_p), _p(idx)) == 0
        for i, e in enumerate(fits):
            d = descs[i]
            o = d.idx_offset
            assert (d.b1, d.b2, d.scene) == (e.b1, e.b2, 3)
            np.testing.assert_array_equal(idx[o:o + d.m1], e.b1_inds)
            np.testing.assert_array_equal(idx[o + d.m1:o + d.m1 + d.m2], e.b2_inds)
            np.testing.assert_array_equal(idx[o + d.m1 + d.m2:o + d.m1 + d.m2 + d.t], e.intersect_inds)
        kind = np.zeros(max(cnt.n_events, 1), np.uint8)
        b1 = np.zeros(max(cnt.n_events, 1), np.int32)
        b2, aux = np.zeros_like(b1), np.zeros_like(b1)
        offs = np.zeros(cnt.n_events + 1, np.int64)
        eidx = np.zeros(max(cnt.n_event_idx, 1), np.int32)
        assert lib.gapro_schedule_export_events(sched, _p(kind), _p(b1), _p(b2), _p(aux), _p(offs), _p(eidx)) == 0
        for i, e in enumerate(events):
            assert (kind[i] == 1) == (e.kind == "fit")
            assert (b1[i], b2[i]) == (e.b1, e.b2)
            if e.kind == "contain":
                assert aux[i] == e.winner
            np.testing.assert_array_equal(eidx[offs[i]:offs[i + 1]], e.intersect_inds)
        cat = lambda j, dt: np.ascontiguousarray(np.concatenate([r[j] for r in results]).astype(dt))  # noqa: E731
        a_pn, a_lb, a_mu, a_var = cat(1, np.float32), cat(2, np.uint8), cat(3, np.float32), cat(4, np.float32)
        S = part.n_spps
        sem_spp, inst_spp = np.empty(S, np.int32), np.empty(S, np.int32)
        prob_spp, mu_spp, var_spp = np.empty(S, np.float32), np.empty(S, np.float32), np.empty(S, np.float32)
        cls64, vol64 = np.ascontiguousarray(cls.astype(np.int64)), np.ascontiguousarray(vol.astype(np.float64))
        assert lib.gapro_schedule_merge(sched, _p(a_pn), _p(a_lb), _p(a_mu), _p(a_var), _p(cls64), _p(vol64), n_fg, 18,
                                        _p(sem_spp), _p(inst_spp), _p(prob_spp), _p(mu_spp), _p(var_spp)) == 0
        np.testing.assert_array_equal(sem_spp, state["sem_spp"])
        np.testing.assert_array_equal(inst_spp, state["inst_spp"])
        np.testing.assert_array_equal(prob_spp, state["prob"])
        np.testing.assert_array_equal(mu_spp, state["mu"])
        np.testing.assert_array_equal(var_spp, state["var"])
    finally:
        lib.gapro_schedule_free(sched)


def test_multiword_schedule_cases_cover_every_merge_path():
    """Across the cases above: a contain event, a volume-fallback superpoint, fits across the word boundary, an instance
    id >= 64 that survives, a box index >= n_fg_instances that is dropped, n_fg_instances on both sides of 64."""
    seen = {}
    for total in SCHED_TOTALS:
        _, _, _, part, events, _, n_fg, state = _sched_case(total)
        fits = [e for e in events if e.kind == "fit"]
        left = (part.n_bbs_per_spp > 1) & (state["determined"] == 0)
        seen[total] = dict(
            contain=sum(e.kind == "contain" for e in events), fallback=int(left.sum()),
            fits_high=sum(max(e.b1, e.b2) >= 64 for e in fits), fits_cross=sum(e.b1 < 64 <= e.b2 for e in fits),
            inst_high=int((state["inst_spp"] >= 64).sum()), dropped=int((state["inst"] >= n_fg).sum()), n_fg=n_fg)
    assert sum(s["contain"] for s in seen.values()) >= 1, seen
    assert sum(s["fallback"] for s in seen.values()) >= 1, seen
    assert all(seen[t]["fits_high"] >= 5 and seen[t]["fits_cross"] >= 1 for t in (128, 129)), seen
    assert seen[128]["inst_high"] >= 1 and seen[129]["inst_high"] >= 1, seen
    assert seen[65]["dropped"] >= 1 and seen[129]["dropped"] >= 1, seen  # the floor box, index 64 / 128
    assert min(s["n_fg"] for s in seen.values()) < 64 < max(s["n_fg"] for s in seen.values())
