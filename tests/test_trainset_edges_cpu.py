"""The inputs of tests/test_trainset_edges_gpu.py meet the conditions they were built for: every assertion here uses the
NumPy restatement of the training-set assembly (tests/fit_gp_ref.py) and exact integer / rational arithmetic only, so it
runs without a GPU.  What a case is for is said in tests/trainset_cases.py."""
from fractions import Fraction

import numpy as np
import pytest

import fit_gp_ref as R
import trainset_cases as tc
from oracle.gen_ps_oracle import fixed_point_shift


def _sel(case, s):
    """the restatement's `sel` of side number s of a case built with pair_up"""
    return case.reference()[s // 2][3 + s % 2]


def _side(case, s):
    """(list, intersection) of side number s"""
    p = case.problems[s // 2]
    return p[s % 2], p[2]


# ---------------------------------------------------------------------------------------------- pool
@pytest.mark.parametrize("d", tc.POOL_WIDTHS)
def test_every_accumulate_branch_is_taken_as_stated(d):
    case = tc.pool_width_case(d)
    names, lists = case.info["sides"], case.info["side_lists"]
    assert case.feats.shape[1] == d and len(names) == len(lists) == 9 + 8 * 9 + 2
    seen = set()
    for (name, want), side in zip(names, lists):
        census = tc.wave_census(case.spp[side])
        if want is not None:
            assert census == want, name
        seen.add((census[0] > 0, census[1] > 0, census[2] > 0))
    # the branches apart: sides of wave-shared waves alone, of per-point waves alone, with and without a partial wave
    assert {(True, False, False), (True, False, True), (False, True, False), (False, True, True),
            (False, False, True)} <= seen
    one, mixed, tail = tc.wave_census(case.spp[lists[-1]])
    assert len(lists[-1]) == 2 * len(case.spp) > 2 * tc.ACCUM_STRIDE and tail == 0  # exactly 2 N; the grid strides twice
    assert one > 1000 and mixed > 1000
    # both kinds of wave in every round of the grid
    rows = case.spp[lists[-1]]
    for a in range(0, len(rows), tc.ACCUM_STRIDE):
        o, m, _ = tc.wave_census(rows[a:a + tc.ACCUM_STRIDE])
        assert o > 100 and m > 100
    assert d % 8 in (0, 1, 3, 7)  # the count lane: idle feature lanes (D < 8), lane 0 beside feature 0 (D = 8, 16), ...
    for prob, ref in zip(case.problems, case.reference()):
        assert np.array_equal(ref[3], np.unique(case.spp[prob[0]])) and np.array_equal(ref[4], np.unique(case.spp[prob[1]]))


def test_the_count_lanes_cover_every_residue_the_widths_can_give():
    assert sorted({d % 8 for d in tc.POOL_WIDTHS}) == [0, 1, 3, 7]
    assert {d for d in tc.POOL_WIDTHS if d < 8} == {1, 3, 7} and {8, 9, 15, 16, 17, 33} <= set(tc.POOL_WIDTHS)


def test_the_rounding_ties_are_ties():
    case = tc.pool_rounding_case()
    shift = fixed_point_shift(float(np.abs(case.feats).max()), len(case.feats))
    assert shift == case.info["shift"] == 50
    col0 = [Fraction(float(v)) * 2 ** shift for v in case.feats[:, 0]]
    assert all(q.denominator == 2 for q in col0)  # every term halfway between two integers
    assert min(col0) < 0 < max(col0)
    assert all((Fraction(float(v)) * 2 ** shift).denominator == 4 for v in case.feats[:, 3])
    b1, b2, _ = case.problems[0]
    assert tc.wave_census(case.spp[b1]) == (64, 0, 0) and tc.wave_census(case.spp[b2]) == (0, 64, 0)
    x, m1, m2, s1, s2, _ = case.reference()[0]
    for side, sid, lo, hi, even in case.info["mean_ties"]:
        lst, sel, rows = (b1, s1, x[:m1]) if side == 0 else (b2, s2, x[m1:])
        pts = lst[case.spp[lst] == sid]
        mean = sum(Fraction(float(v)) for v in case.feats[pts, 1]) / len(pts)  # the fixed-point terms are exact here
        assert all((Fraction(float(v)) * 2 ** shift).denominator == 1 for v in case.feats[pts, 1])
        assert np.float32(lo) == lo and np.float32(hi) == hi and np.nextafter(np.float32(lo), np.float32(np.inf)) == hi
        assert mean - Fraction(lo) == Fraction(hi) - mean  # halfway between two neighbouring float32
        assert rows[list(sel).index(sid), 1] == np.float32(even)
        assert int(np.float32(even).view(np.uint32)) % 2 == 0
    # what the case tells apart: truncation and rounding half away from zero give other rows on BOTH sides
    q = np.ldexp(case.feats.astype(np.float64), shift)
    for other in (np.trunc, lambda v: np.sign(v) * np.floor(np.abs(v) + 0.5)):
        for lst, sel, rows in ((b1, s1, x[:m1]), (b2, s2, x[m1:])):
            ids, inv = np.unique(case.spp[lst], return_inverse=True)
            sums = np.zeros((len(ids), 4))
            np.add.at(sums, inv.reshape(-1), other(q[lst]))
            alt = (np.ldexp(sums, -shift) / np.bincount(inv.reshape(-1))[:, None]).astype(np.float32)
            assert (alt[:, 0] != rows[:, 0]).any() or (alt[:, 3] != rows[:, 3]).any()


@pytest.mark.parametrize("s", tc.RANK_S)
def test_the_rank_cases_touch_the_stated_ranks(s):
    case = tc.rank_case(s)
    ids = np.unique(case.spp)
    assert len(ids) == s == case.info["n_spps"]
    sets = case.info["rank_sets"]
    assert [0] in sets and [s - 1] in sets and list(range(s)) in sets and list(range(0, s, 2)) in sets
    for e in range(tc.SCAN, s, tc.SCAN):  # the last slot of a scan round and the first of the next
        assert [e - 1, e] in sets
    assert ([255, 256] in sets) == (s > 256)
    for i, ranks in enumerate(sets):
        sel = _sel(case, i)
        assert np.array_equal(sel, ids[ranks]) and (np.diff(sel) > 0).all()
        assert len(_side(case, i)[0]) >= 2 * len(ranks)  # more points than rows: the pooling pools


@pytest.mark.parametrize("n,kind", tc.HEADROOM)
def test_the_headroom_cases_fill_the_sums(n, kind):
    case = tc.headroom_case(n, kind)
    fmax, top = case.info["fmax"], case.info["top"]
    assert len(case.feats) == n and float(np.abs(case.feats).max()) == fmax == float(case.feats[top, 0])
    assert fmax == (tc.FLT_MAX if kind == "flt_max" else 2.0 ** -149)
    k = fixed_point_shift(fmax, n)
    q = Fraction(fmax) * Fraction(2) ** k
    assert q.denominator == 1
    total = 2 * n * int(q)
    assert 2 ** 60 <= total < 2 ** 63  # the sum of 2 N such terms fits int64, and only just
    assert fixed_point_shift(fmax, 1025) == fixed_point_shift(fmax, 1024) - 1
    b1, b2, _ = case.problems[0]
    assert len(b1) == len(b2) == 2 * n and (b1 == top).all() and (b2 == top).sum() == n
    full, tail = 2 * n // 8, 2 * n % 8  # N = 1025 leaves a partial wave of two entries
    assert tc.wave_census(case.spp[b1]) == (full, 0, tail) and tc.wave_census(case.spp[b2]) == (0, full, tail)
    x, m1, m2, s1, s2, _ = case.reference()[0]
    assert m1 == 1 and np.array_equal(x[0, :2], np.float32([fmax, -fmax])) and np.isfinite(x).all()
    assert np.array_equal(case.reference()[1][0][-1, :2], np.float32([fmax, -fmax]))  # as side 2


def test_the_ragged_batch_is_as_stated():
    case = tc.ragged_case()
    n = len(case.spp)
    assert len(case.problems) == 300
    small = [p for i, p in enumerate(case.problems) if i not in (150, 151)]
    assert len(small) == 298 and all(1 <= len(p[0]) <= 3 and 1 <= len(p[1]) <= 3 for p in small)
    big = case.problems[150]
    assert len(big[0]) == len(big[1]) == 40000 == 2 * n
    same = case.problems[151]
    assert np.array_equal(same[0], same[1])
    x, m1, m2, s1, s2, _ = case.reference()[151]
    assert m1 == m2 and np.array_equal(x[:m1], x[m1:]) and np.array_equal(s1, s2)
    assert case.reference()[150][1] == len(np.unique(case.spp)) == 300


# ---------------------------------------------------------------------------------------------- nearest
def test_the_pinned_centroid_and_the_ladder_are_exact():
    """An intersection of the one point (0, 0, 0) has the centroid (0, 0, 0) whatever else the scene holds, and the
    points (1, a 2^-26, b 2^-26) have the distance 1 + (a^2 + b^2) 2^-52 with no rounding."""
    for far in (1.0, 1e300, 1e-300):
        coords = np.array([(0.0, 0.0, 0.0), (far, -far, far), (3.0, 1.0, 2.0)])
        assert np.array_equal(R.centroid(coords, [0]), np.zeros(3))
        assert np.array_equal(R.centroid(coords, [0, 0, 0]), np.zeros(3))
    ab = [(a, b) for a in range(16) for b in range(16)]
    coords = np.array([(1.0, a * 2.0 ** -26, b * 2.0 ** -26) for a, b in ab])
    keys = R.distances(coords, np.arange(len(ab)), np.zeros(3)).view(np.uint64)
    assert [int(v) for v in keys] == [0x3FF0000000000000 + a * a + b * b for a, b in ab]
    assert all(Fraction(float(v)) == 1 + Fraction(a * a + b * b, 2 ** 52)
               for v, (a, b) in zip(keys.view(np.float64), ab))
    low = {int(v) for v in keys if int(v) < 0x3FF0000000000100}
    assert len(low) == 97 and len({v >> 8 for v in low}) == 1  # 97 keys that share their top 56 bits


def test_every_radix_pass_decides_a_cut():
    case = tc.radix_case()
    assert case.k == tc.RADIX_K and case.info["n_sides"] == 10
    for p in range(8):
        side = _side(case, p)
        v, n_less, r_eq, group, byte = tc.cut_of(tc.keys_of(case, side), case.k)
        assert (v, n_less, r_eq, group, byte) == (0x3FF0000000000000, case.k - 1, 1, 1, p), p
        assert [(v >> (8 * q)) & 255 for q in range(6)] == [0] * 6  # the chosen bin is 0 in the six lower passes
        assert len(side[0]) > case.k + 8 - p
    for s, pass_255, byte_cut in case.info["bin255"]:
        v, n_less, r_eq, group, byte = tc.cut_of(tc.keys_of(case, _side(case, s)), case.k)
        assert (v >> (8 * pass_255)) & 255 == 255 and byte == byte_cut < pass_255 and (r_eq, group) == (1, 1)
        nxt = int(np.sort(tc.keys_of(case, _side(case, s)))[case.k])
        assert (nxt >> (8 * pass_255)) & 255 == 255  # the next distance shares the bin: the pass below has to decide


@pytest.mark.parametrize("k", [1024, 100])
def test_the_tie_groups_sit_on_the_cut_and_on_the_edges(k):
    case = tc.tie_case(k)
    names, lists = case.info["sides"], case.info["side_lists"]
    one = 0x3FF0000000000000
    seen = set()
    for s, ((name, group, r_eq, pos), side) in enumerate(zip(names, lists)):
        keys = tc.keys_of(case, _side(case, s))
        if name == "origin":
            assert int(keys.min()) == 0 and _sel(case, s)[0] == 0 and len(side) > k
            continue
        v, n_less, got_r_eq, got_group, _ = tc.cut_of(keys, k)
        assert (got_group, got_r_eq, n_less) == (group, r_eq, k - r_eq), name
        assert np.array_equal(np.nonzero(keys == v)[0], pos), name
        if name == "coincident":
            assert n_less == 0 and r_eq == k and len(np.unique(side)) == 1500
            continue
        assert v == one
        if name == "listed three times":
            assert len(np.unique(side[pos])) == 1 and list(_sel(case, s)[-2:]) == [side[pos[0]]] * 2
            continue
        assert len(np.unique(case.coords[side[pos]], axis=0)) == min(group, 6)  # distinct points, one distance
        seen.add((group, "one" if r_eq == 1 else "all" if r_eq == min(group, k) else "all but one"))
        edges = [e for e in (64, 1024, 2048) if e - 1 in pos and e in pos]
        if group == 2:
            assert edges == [int(name.split("@")[1])], name
        elif group == 65:
            assert len(edges) == 1, name
        elif name == "1025 run":
            assert 1024 in edges
        elif name == "5000":
            assert len(edges) >= 1 and pos.max() >= 5 * tc.SEL  # members in six collect rounds
    want = {(g, r) for g in (2, 65, 1025, 5000) for r in ("one", "all")} | {(65, "all but one")}
    assert want <= seen
    if k == 1024:  # r_eq = group - 1 for the group of 1025: the whole selection is ties
        assert any(g == 1025 and r == 1024 for _, g, r, _ in names)
    # the edges the members straddle, over the whole case
    straddled = {e for _, g, _, pos in names if pos is not None for e in (64, 1024, 2048) if e - 1 in pos and e in pos}
    assert straddled == {64, 1024, 2048}


@pytest.mark.parametrize("k", tc.SIZE_K)
def test_the_size_cases_hold_the_stated_sizes(k):
    case = tc.size_case(k)
    longs, short = case.info["longs"], case.info["short"]
    assert set(longs) == {m for m in (k + 1, 1024, 1025, 2048, 2049, 30000) if m > k}
    assert set(short) == {m for m in (1, k - 1, k) if m >= 1}
    sizes = [(len(p[0]), len(p[1])) for p in case.problems]
    assert {m for pair in sizes for m in pair} == set(longs) | set(short)
    assert any(a > k >= b for a, b in sizes) and any(b > k >= a for a, b in sizes) and any(a > k and b > k for a, b in sizes)
    ties = 0
    for p, ref in zip(case.problems, case.reference()):
        assert np.array_equal(R.centroid(case.coords, p[2]), np.zeros(3))
        for side, sel in ((p[0], ref[3]), (p[1], ref[4])):
            if len(side) <= k:
                assert np.array_equal(sel, side)
                assert len(side) <= 2 or not np.array_equal(side, np.sort(side))  # copied in a shuffled order
            else:
                v, n_less, r_eq, group, _ = tc.cut_of(tc.keys_of(case, (side, p[2])), k)
                ties += group > r_eq
    assert ties >= 1  # a tie group is cut on some long side


def test_the_centroid_cases_wrap_both_grids():
    case = tc.centroid_case("1")
    n = len(case.coords)
    assert n == tc.CENTROID_N and 3 * n > tc.ABSMAX_STRIDE and n > 43691
    flat = np.abs(case.coords.reshape(-1))
    assert flat.argmax() == 3 * n - 1 and (flat[:-1] < flat[-1]).all()
    ts = [len(p[2]) for p in case.problems]
    assert ts == list(tc.CENTROID_T) + [2 * n]
    assert sum(t > tc.CENTROID_STRIDE for t in ts) >= 3 and tc.CENTROID_STRIDE in ts and tc.CENTROID_STRIDE + 1 in ts
    assert (case.problems[-1][2] == n - 1).all()  # 2 N entries, all of them the farthest point
    kc = fixed_point_shift(float(flat.max()), n)
    q = [int(Fraction(float(v)) * Fraction(2) ** kc) for v in case.coords[n - 1]]
    assert 2 ** 59 <= 2 * n * max(abs(v) for v in q) < 2 ** 63
    assert np.array_equal(R.centroid(case.coords, case.problems[-1][2]), case.coords[n - 1])
    cents = [R.centroid(case.coords, p[2]) for p in case.problems]
    assert len({tuple(c) for c in cents}) == len(cents)
    for p in case.problems:
        assert len(p[0]) > case.k and len(p[1]) > case.k  # every side needs its centroid


@pytest.mark.parametrize("scale", tc.CENTROID_SCALES[1:])
def test_the_scaled_centroid_scenes_are_as_stated(scale):
    case, base = tc.centroid_case(scale), tc.centroid_case("1")
    n = len(case.coords)
    assert n == tc.CENTROID_N and [len(p[2]) for p in case.problems] == [1, 257, 20000]
    finite = np.abs(case.coords[np.isfinite(case.coords)])
    if scale == "zeros":
        assert not case.coords.any()
    elif scale == "inf elsewhere":
        used = np.concatenate([np.concatenate(p) for p in case.problems])
        assert np.isinf(case.coords).sum() == 1 and np.isfinite(case.coords[used]).all()
        assert all(r[5] == 0 for r in case.reference())
        assert abs(case.coords[n - 1, 2]) == finite.max()
    else:
        assert np.array_equal(case.coords, base.coords * float(scale)) and abs(case.coords[n - 1, 2]) == finite.max()
        kc = fixed_point_shift(float(finite.max()), n)
        assert (kc == 1000) == (scale == "1e-300") and (kc < -900) == (scale == "1e300")
    with np.errstate(over="ignore", invalid="ignore"):
        d = R.distances(case.coords, case.problems[1][0], R.centroid(case.coords, case.problems[1][2]))
    if scale in ("1e-150", "1e150"):
        assert np.isfinite(d).all() and len(np.unique(d)) == len(d) and d.min() > 0
    elif scale == "1e300":
        assert np.isinf(d).all()
    elif scale in ("1e-300", "zeros"):
        assert not d.any()
    if scale in ("1e300", "1e-300", "zeros"):  # every distance equal: the first k of the list, in its order
        for p, ref in zip(case.problems, case.reference()):
            assert np.array_equal(ref[3], p[0][:case.k]) and np.array_equal(ref[4], p[1][:case.k])


def _fused_sel(case, side, pattern):
    d = case.coords[side]  # the centroid is the origin
    return side[np.lexsort((np.arange(len(side)), tc.fused_distances(d, pattern)))[:case.k]]


def test_a_contracted_distance_changes_the_selection():
    """Every pair ties under the stated arithmetic and is parted by the fusions it was built for; on this case the
    restatement's `sel` differs from the selection by fused distances, whichever way the compiler might fuse."""
    case = tc.contraction_case()
    sides = case.info["side_lists"]
    assert len(sides) == 4 and len(sides[0]) == 24 and len(sides[2]) >= 2 * 6 and len(tc.last_add_pairs()) == 12
    for p in case.problems:
        assert np.array_equal(R.centroid(case.coords, p[2]), np.zeros(3))
    for s, side in enumerate(sides):
        d = case.coords[side]
        plain = tc.plain_distances(d)
        assert np.array_equal(plain, R.distances(case.coords, side, np.zeros(3)))
        pairs = plain.reshape(-1, 2)
        assert (pairs[:, 0] == pairs[:, 1]).all() and len(np.unique(pairs[:, 0])) == len(pairs)  # ties, and only in pairs
        for pattern in (("all", "all_x", "xy") if s < 2 else ("all", "all_x", "z")):
            f = tc.fused_distances(d, pattern).reshape(-1, 2)
            assert (f[:, 0] != f[:, 1]).all(), (s, pattern)
            assert np.array_equal(np.argsort(f.min(1)), np.argsort(pairs[:, 0]))  # no pair overtakes another
        v, n_less, r_eq, group, _ = tc.cut_of(plain.view(np.uint64), case.k)
        assert (n_less, r_eq, group) == (case.k - 1, 1, 2)  # four pairs inside the selection, the fifth on the cut
    assert np.array_equal(np.sort(sides[0]), np.sort(sides[1])) and not np.array_equal(sides[0], sides[1])
    for pattern in tc.FUSED_PATTERNS:
        moved = [s for s, side in enumerate(sides) if not np.array_equal(_fused_sel(case, side, pattern), _sel(case, s))]
        assert moved, pattern
        if pattern != "z":  # a mirrored pair is parted either way round: both list orders show it
            assert {0, 1} <= set(moved), pattern
        if pattern != "xy":  # (1, 0, z) only ever comes nearer: the side that lists it second shows it
            assert 2 in moved and 3 not in moved, pattern
            fused = _fused_sel(case, sides[2], pattern)
            assert set(fused) != set(_sel(case, 2)) and not np.array_equal(fused[:8], _sel(case, 2)[:8])  # cut and order
    # the two kinds are both needed: the mirrored pairs stay tied when only the last addition is fused, the others when
    # only the first is
    assert np.array_equal(_fused_sel(case, sides[0], "z"), _sel(case, 0))
    assert np.array_equal(_fused_sel(case, sides[2], "xy"), _sel(case, 2))


# ---------------------------------------------------------------------------------------------- host-only refusals
def _descs(sizes):
    from gapro_amd import _lib

    descs = (_lib.TrainsetDesc * len(sizes))()
    for d, (n1, n2, t) in zip(descs, sizes):
        d.n1, d.n2, d.t = n1, n2, t
    return descs


def test_workspace_bytes_is_zero_for_what_the_calls_refuse():
    import ctypes as C

    from gapro_amd import _lib

    lib = _lib.load()

    def ws(mode, sizes, n_spps=100, d=6, n=None):
        return lib.gapro_trainset_workspace_bytes(mode, C.cast(_descs(sizes), C.c_void_p), len(sizes) if n is None else n,
                                                  n_spps, d)

    ok = [(5, 7, 3), (2000, 1, 0)]
    assert _lib.TRAINSET_MAX_PROBLEMS == 32767
    for mode in (_lib.TRAINSET_POOL, _lib.TRAINSET_NEAREST):
        assert ws(mode, ok) > 0
        many = [(1, 1, 0)] * 32768
        assert ws(mode, many) == 0 and ws(mode, many[:-1]) > 0  # one problem more than the limit
        assert ws(mode, ok, d=0) == 0
        assert ws(mode, [(5, 0, 3)]) == 0 and ws(mode, [(0, 5, 3)]) == 0  # a side of no point
        assert ws(mode, [(5, 7, -1)]) == 0  # a negative T
        assert ws(mode, ok, n=0) == 0
    for mode in (-1, 2, 7):
        assert ws(mode, ok) == 0
    assert ws(_lib.TRAINSET_POOL, ok, n_spps=0) == 0 and ws(_lib.TRAINSET_NEAREST, ok, n_spps=0) > 0


@pytest.mark.parametrize("sizes,n_spps,d", [([(5, 7, 3), (2000, 1, 0)], 100, 6), ([(1, 1, 0)], 1, 1),
                                            ([(40000, 40000, 9)] + [(2, 3, 1)] * 299, 300, 33),
                                            ([(3, 1025, 2)] * 7, 1025, 17)])
def test_workspace_bytes_is_the_documented_layout(sizes, n_spps, d):
    import ctypes as C

    from gapro_amd import _lib

    lib = _lib.load()
    for pool in (True, False):
        got = lib.gapro_trainset_workspace_bytes(_lib.TRAINSET_POOL if pool else _lib.TRAINSET_NEAREST,
                                                 C.cast(_descs(sizes), C.c_void_p), len(sizes), n_spps, d)
        assert got == tc.workspace_layout(sizes, n_spps, d, pool)
