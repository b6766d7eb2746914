"""Inputs of the edge tests of the training-set assembly (csrc/trainset.hip): scenes and problem lists
that put each of its seven kernels on its chunk, wave and word edges, and the helpers both test files share.

tests/test_trainset_edges_cpu.py asserts, with the NumPy restatement alone (tests/fit_gp_ref.py), that every case meets
the condition it was built for; tests/test_trainset_edges_gpu.py runs the same cases through gp_train_sets and compares
bit for bit (`same_sets`).  A case is built once per process (the builders are cached) and so is its reference.

The shapes the cases speak of, read from the kernels: k_ts_accum gives a point eight lanes, so a wave holds the eight
list entries [8 g, 8 g + 8) and its grid strides by 8 192 entries; k_ts_rank scans 256 flags a round; k_ts_nearest is one
workgroup of 1024 threads, i.e. 16 waves and collect rounds of 1024 list entries; the centroid grid holds at most
64 x 256 entries a round and the abs-max grid 512 x 256 coordinates."""
import functools
import itertools
from fractions import Fraction

import numpy as np

import fit_gp_ref as R

WAVE_POINTS = 8
ACCUM_STRIDE = 256 * 32  # list entries one round of k_ts_accum's grid covers
SCAN = 256
SEL = 1024
CENTROID_STRIDE = 64 * 256
ABSMAX_STRIDE = 512 * 256
FLT_MAX = float(np.finfo(np.float32).max)
FLT_DENORM = float(np.float32(1e-45))


class Case:
    """A scene, its problems and how gp_train_sets is to be called; `sides` names the sides the conditions speak of."""

    def __init__(self, name, coords, feats, spp, problems, k=800, pool=True, **info):
        self.name, self.k, self.pool, self.info = name, k, pool, info
        self.coords = np.ascontiguousarray(coords, dtype=np.float64)
        self.feats = np.ascontiguousarray(feats, dtype=np.float32)
        self.spp = np.ascontiguousarray(spp, dtype=np.int64)
        self.problems = [tuple(np.asarray(x, dtype=np.int64).reshape(-1) for x in p) for p in problems]
        self._ref = None

    def reference(self):
        """R.train_set of every problem, computed once."""
        if self._ref is None:
            with np.errstate(over="ignore", invalid="ignore"):
                self._ref = [R.train_set(self.coords, self.feats, self.spp, p, self.k, self.pool) for p in self.problems]
        return self._ref

    def run(self):
        from gapro_amd import gp_train_sets

        return gp_train_sets(self.coords, self.feats, self.spp, self.problems, npoint_nearest=self.k, spp_pool=self.pool)


def same_sets(got, coords, feats, spp, problems, k=800, pool=True, what="", ref=None):
    """gp_train_sets' result against the restatement: row counts, dtypes, `sel` (order included) and rows, bit for bit."""
    assert len(got) == len(problems)
    for i, (g, prob) in enumerate(zip(got, problems)):
        x, m1, m2, s1, s2, _ = ref[i] if ref is not None else R.train_set(coords, feats, spp, prob, k, pool)
        tag = "%s problem %d" % (what, i)
        assert (g[1], g[2]) == (m1, m2), tag
        assert g[0].dtype == np.float32 and g[3].dtype == np.int64 and g[4].dtype == np.int64, tag
        assert np.array_equal(g[3], s1) and np.array_equal(g[4], s2), tag
        assert np.array_equal(g[0], x), tag


def check(case, got):
    same_sets(got, case.coords, case.feats, case.spp, case.problems, case.k, case.pool, case.name, case.reference())


def pair_up(sides, inter):
    """Problems of two sides each from a list of sides (the last one is paired with the first when their number is odd)."""
    sides = list(sides)
    if len(sides) % 2:
        sides.append(sides[0])
    return [(sides[i], sides[i + 1], inter) for i in range(0, len(sides), 2)]


# ---------------------------------------------------------------------------------------------- pool 1: k_ts_accum
POOL_WIDTHS = (1, 3, 7, 8, 9, 15, 16, 17, 33)
POOL_SIDE_N = (1, 7, 8, 9, 63, 64, 65, 1023, 1025)


def wave_census(rows):
    """(waves that take the wave-shared branch, full waves that take the per-point branch, entries of the partial last
    wave) of k_ts_accum on a side whose list entries pool to `rows`: a wave is the entries [8 g, 8 g + 8) and shares its
    row only when it is full and all eight agree."""
    rows = np.asarray(rows)
    full = len(rows) // WAVE_POINTS
    g = rows[:full * WAVE_POINTS].reshape(full, WAVE_POINTS)
    one = int((g == g[:, :1]).all(axis=1).sum())
    return one, full - one, len(rows) - full * WAVE_POINTS


@functools.lru_cache(maxsize=None)
def pool_width_case(d):
    """One call per feature width: every POOL_SIDE_N inside one superpoint, the same with an entry of another superpoint
    at offset p of every group of eight (p = 0 .. 7), a side that alternates both kinds of wave, and a side of 2 N =
    20 000 entries that mixes them and strides twice.  info["sides"] = (name, expected census or None)."""
    rng = np.random.default_rng(500 + d)
    n = 10000
    spp = np.empty(n, np.int64)
    spp[:1200], spp[1200:2400] = 11, 5  # the superpoint met first has the larger id
    spp[2400:] = 20 + rng.integers(0, 8, n - 2400)
    feats = rng.normal(size=(n, d)).astype(np.float32)
    a, b = np.arange(1200), np.arange(1200, 2400)
    sides, names = [], []
    for m in POOL_SIDE_N:
        sides.append(rng.permutation(a)[:m])
        names.append(("one n=%d" % m, (m // 8, 0, m % 8)))
    for p in range(WAVE_POINTS):
        for m in POOL_SIDE_N:
            s = rng.permutation(a)[:m]
            at = np.arange(p, m, WAVE_POINTS)
            s[at] = rng.permutation(b)[:len(at)]
            sides.append(s)
            names.append(("other at %d n=%d" % (p, m), (0, m // 8, m % 8)))
    groups = []
    for g in range(25):  # even waves share a row, odd ones do not
        groups.append(rng.choice(a, 8) if g % 2 == 0 else np.r_[rng.choice(a, 3), rng.choice(b, 5)][rng.permutation(8)])
    sides.append(np.concatenate(groups + [rng.choice(b, 3)]))
    names.append(("alternating", (13, 12, 3)))
    members = [np.nonzero(spp == u)[0] for u in np.unique(spp)]
    groups = []
    for g in range(2 * n // WAVE_POINTS):
        if rng.random() < 0.5:
            groups.append(rng.choice(members[rng.integers(len(members))], 8))
        else:
            two = rng.choice(len(members), 2, replace=False)
            groups.append(np.r_[rng.choice(members[two[0]], 1), rng.choice(members[two[1]], 1),
                                rng.choice(np.r_[members[two[0]], members[two[1]]], 6)][rng.permutation(8)])
    sides.append(np.concatenate(groups))
    names.append(("2 N entries", None))
    return Case("pool D=%d" % d, rng.normal(size=(n, 3)), feats, spp, pair_up(sides, np.arange(3)), sides=names,
                side_lists=sides)


# ---------------------------------------------------------------------------------------------- pool 2: rounding
@functools.lru_cache(maxsize=None)
def pool_rounding_case():
    """N = 1024 and |f|max = 1: fixed_shift 50.  Column 0 holds odd multiples of 2^-51 of both signs (every term an exact
    tie of to_fixed), column 3 odd multiples of 2^-52 (quarters: truncation shows), column 1 the float32 ties of the mean.
    Side 0 lists 63 waves of superpoint 3 and one wave of superpoint 103 (the wave-shared branch throughout); side 1 lists
    points whose superpoint changes with every entry (the per-point branch) and, at its end, three pairs whose mean is a
    float32 tie.  info["mean_ties"] = (side, superpoint id, the two float32 neighbours, the even one)."""
    rng = np.random.default_rng(77)
    n = 1024
    f = np.zeros((n, 4), np.float64)
    f[:, 0] = np.ldexp((2 * rng.integers(-2 ** 20, 2 ** 20, n) + 1).astype(np.float64), -51)
    f[:, 3] = np.ldexp(4.0 * rng.integers(-1000, 1000, n) + rng.choice([1.0, 3.0], n), -52)
    f[5, 2] = 1.0
    f[:, 1] = (rng.standard_normal(n) * 0.1).astype(np.float32)
    u = 2.0 ** -24  # the spacing of float32 in [0.5, 1)
    spp = np.empty(n, np.int64)
    spp[:504] = 3
    spp[504:512] = 103
    f[504:512, 1] = np.tile([0.5, 0.5 + u], 4)           # mean 0.5 + u/2 -> 0.5 (even)
    spp[512:1018] = 10 + np.arange(506) % 7
    spp[1018:1020], f[1018:1020, 1] = 100, [0.5, 0.5 + u]            # -> 0.5
    spp[1020:1022], f[1020:1022, 1] = 101, [0.5 + u, 0.5 + 2 * u]    # mean 0.5 + 1.5 u -> 0.5 + 2 u (even)
    spp[1022:1024], f[1022:1024, 1] = 102, [-0.5, -0.5 - u]          # -> -0.5
    feats = f.astype(np.float32)
    assert (feats.astype(np.float64) == f).all()
    ties = ((0, 103, 0.5, 0.5 + u, 0.5), (1, 100, 0.5, 0.5 + u, 0.5), (1, 101, 0.5 + u, 0.5 + 2 * u, 0.5 + 2 * u),
            (1, 102, -0.5 - u, -0.5, -0.5))
    return Case("pool rounding", rng.normal(size=(n, 3)), feats, spp, [(np.arange(512), np.arange(512, 1024), [0])],
                mean_ties=ties, shift=50)


# ---------------------------------------------------------------------------------------------- pool 3: k_ts_rank
RANK_S = (1, 2, 255, 256, 257, 511, 512, 513, 1025)


@functools.lru_cache(maxsize=None)
def rank_case(s):
    """A scene of S superpoints (ids 7 + 3 rank, two or more points each) and sides that touch exactly the ranks of
    info["rank_sets"]: the first, the last, the two slots on either side of every 256-wide scan round, all, and every
    other one from 0 and from 1."""
    rng = np.random.default_rng(900 + s)
    n = max(2 * s + 5, 16)
    rank = rng.permutation(np.arange(n) % s)
    spp = 7 + 3 * rank.astype(np.int64)
    sets = [[0], [s - 1]] + [[e - 1, e] for e in range(SCAN, s, SCAN)] + [list(range(s)), list(range(0, s, 2))]
    if s > 1:
        sets.append(list(range(1, s, 2)))
    sides = [rng.permutation(np.nonzero(np.isin(rank, r))[0]) for r in sets]
    return Case("rank S=%d" % s, rng.normal(size=(n, 3)), rng.normal(size=(n, 5)).astype(np.float32), spp,
                pair_up(sides, [0]), rank_sets=sets, n_spps=s)


# ---------------------------------------------------------------------------------------------- pool 4: headroom
HEADROOM = tuple((n, m) for m in ("flt_max", "denormal") for n in (1024, 1025))


@functools.lru_cache(maxsize=None)
def headroom_case(n, kind):
    """The point that holds +|f|max in column 0 and -|f|max in column 1 listed 2 N times: alone (the wave-shared branch),
    alternating with a point of another superpoint (the per-point branch: N terms in the row), and as side 2."""
    rng = np.random.default_rng(n + len(kind))
    fmax = FLT_MAX if kind == "flt_max" else FLT_DENORM
    if kind == "flt_max":
        f = (rng.uniform(-1, 1, (n, 3)) * fmax).astype(np.float32)
    else:
        f = (rng.integers(-1, 2, (n, 3)) * fmax).astype(np.float32)
    spp = rng.integers(0, 20, n).astype(np.int64) * 5
    top, other = n // 3, n // 3 + 1
    spp[top], spp[other] = 1000, 2000
    spp[[top + 2, top + 3]] = 1000, 2000  # both superpoints hold a second point
    f[top, 0], f[top, 1] = fmax, -fmax
    assert np.abs(f).max() == np.float32(fmax)
    few = rng.permutation(n)[:40]
    problems = [(np.full(2 * n, top), np.tile([top, other], n), [0]), (few, np.full(2 * n, top), [0]),
                (np.r_[np.full(2 * n - 2, top), top + 2, top + 2], few, [])]
    return Case("headroom N=%d %s" % (n, kind), rng.normal(size=(n, 3)), f, spp, problems, fmax=fmax, top=top)


# ---------------------------------------------------------------------------------------------- pool 5: ragged batch
@functools.lru_cache(maxsize=None)
def ragged_case():
    """300 problems in one call (grid.y = 600): sides of 1 .. 3 points, problem 150 with two sides of 2 N = 40 000
    entries, problem 151 with both sides the same list."""
    rng = np.random.default_rng(300)
    n = 20000
    spp = rng.integers(0, 300, n).astype(np.int64) * 11 + 2
    problems = []
    for i in range(300):
        if i == 150:
            problems.append((rng.integers(0, n, 2 * n), rng.integers(0, n, 2 * n), rng.integers(0, n, 9)))
        elif i == 151:
            s = rng.permutation(n)[:500]
            problems.append((s, s.copy(), s[:4]))
        else:
            problems.append((rng.integers(0, n, rng.integers(1, 4)), rng.integers(0, n, rng.integers(1, 4)),
                             rng.integers(0, n, rng.integers(0, 3))))
    return Case("ragged", rng.normal(size=(n, 3)), rng.normal(size=(n, 6)).astype(np.float32), spp, problems)


# ---------------------------------------------------------------------------------------------- nearest: helpers
class Points:
    """Collects the points of a crafted scene; point 0 is the origin, the one-point intersection that pins the centroid
    at (0, 0, 0) exactly, whatever the scale of the other coordinates."""

    def __init__(self):
        self.xyz = [(0.0, 0.0, 0.0)]

    def add(self, pts):
        pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
        first = len(self.xyz)
        self.xyz.extend(map(tuple, pts))
        return np.arange(first, first + len(pts))

    def scene(self, seed, d=3):
        rng = np.random.default_rng(seed)
        n = len(self.xyz)
        return np.array(self.xyz, dtype=np.float64), rng.normal(size=(n, d)).astype(np.float32), np.arange(n) % 5


ORIGIN = np.array([0])


def on_x(v):
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    return np.stack([v, np.zeros_like(v), np.zeros_like(v)], axis=1)


def keys_of(case, side):
    """The 64-bit patterns of a side's distances to its problem's centroid, in list order (the restatement's)."""
    c = R.centroid(case.coords, np.asarray(side[1], dtype=np.int64)) if len(side[1]) else np.zeros(3)
    with np.errstate(over="ignore", invalid="ignore"):
        return R.distances(case.coords, side[0], c).view(np.uint64)


def cut_of(keys, k):
    """(V, n_less, r_eq, size of V's tie group, byte in which the k-th and (k + 1)-th smallest keys first differ or None)"""
    s = np.sort(keys)
    v = int(s[k - 1])
    n_less = int((s < v).sum())
    x = v ^ int(s[k]) if k < len(s) else 0
    return v, n_less, k - n_less, int((s == v).sum()), (x.bit_length() - 1) // 8 if x else None


def three_squares(m):
    """(a, b, c), a >= b >= c >= 0, with a^2 + b^2 + c^2 = m; None when there is none (m = 4^i (8 j + 7))."""
    for a in range(int(m ** 0.5), -1, -1):
        for b in range(min(a, int((m - a * a) ** 0.5)), -1, -1):
            c2 = m - a * a - b * b
            c = int(round(c2 ** 0.5))
            if c <= b and c * c == c2:
                return a, b, c
    return None


# ---------------------------------------------------------------------------------------------- nearest 6: radix passes
RADIX_K = 40
# the point whose distance is the (k + 1)-th smallest when the k-th is exactly 1 and the two first differ in byte p
RADIX_NEXT = {0: (1.0, 2.0 ** -26, 0.0), 1: (1.0, 2.0 ** -22, 0.0), 2: (1.0, 2.0 ** -18, 0.0), 3: (1.0, 2.0 ** -14, 0.0),
              4: (1.0, 2.0 ** -10, 0.0), 5: (1.0, 2.0 ** -6, 0.0), 6: (1.0, 0.5, 0.0), 7: (256.0, 0.0, 0.0)}


@functools.lru_cache(maxsize=None)
def radix_case():
    """Sides of 39 distances below 1, the distance 1 itself (pattern 0x3FF0 0000 0000 0000: bin 0 in six passes) and, as
    the next one, 1 + 2^-52 .. 1 + 2^-12, 1.25 or 65 536: the cut between the 40th and 41st is decided in pass p = 0 .. 7
    (sides 0 .. 7), every larger such distance lying behind it.  Sides 8 and 9 choose bin 255: in pass 6 (504/256 against
    505/256: 0x3FFF 8.. | 0x3FFF 9..) and in pass 5 (1 + 255/4096 + 1/16384 against + 2/16384)."""
    pts = Points()
    low = pts.add(on_x(1.0 - np.arange(1, RADIX_K) / 1024.0))
    one = pts.add([(1.0, 0.0, 0.0)])
    nxt = {p: pts.add([RADIX_NEXT[p]]) for p in range(8)}
    far = pts.add(on_x(300.0 + np.arange(1, 31)))
    rng = np.random.default_rng(6)
    sides = [rng.permutation(np.concatenate([low, one, far] + [nxt[q] for q in range(p, 8)])) for p in range(8)]
    for den, m_a, m_b in ((16, 504, 505), (128, 17405, 17406)):
        a, b = three_squares(m_a), three_squares(m_b)
        pa, pb = pts.add([np.array(a) / den]), pts.add([np.array(b) / den])
        sides.append(rng.permutation(np.concatenate([low, one, far, pa, pb])[1:]))  # 38 below 1, 1, then a | b
    coords, feats, spp = pts.scene(6)
    return Case("radix", coords, feats, spp, pair_up(sides, ORIGIN), k=RADIX_K, pool=False, n_sides=len(sides),
                bin255=((8, 6, 5), (9, 5, 4)))  # (side, pass whose chosen bin is 255, byte of the cut)


# ---------------------------------------------------------------------------------------------- nearest 7: ties
def _tie_positions():
    """(name, n, positions of the tie group's members in the list)"""
    rng = np.random.default_rng(70)
    out = [("2@%d" % e, 2100, np.array([e - 1, e])) for e in (64, 1024, 2048)]
    out += [("65@%d" % a, 2100, np.arange(a, a + 65)) for a in (30, 1000, 2020)]
    out += [("1025 run", 2100, np.arange(500, 1525)), ("1025 odd", 2100, 2 * np.arange(1025) + 1)]
    out += [("5000", 6100, np.sort(rng.permutation(6100)[:5000]))]
    return out


TIE_LAYOUTS = _tie_positions()


@functools.lru_cache(maxsize=None)
def tie_case(k):
    """Tie groups at the cut, k = 1024 or 100: for every layout of TIE_LAYOUTS and every r_eq of {1, group - 1, group}
    that k allows (r_eq <= k: a group of 1025 or 5 000 cannot lie inside the selection as a whole), a side whose group
    members (six distinct points at distance exactly 1) stand at the stated list positions, k - r_eq nearer points and
    farther ones around them.  Then: 1500 coincident points (n_less = 0, r_eq = k); the origin itself (key 0) among
    others; an index listed three times of which two are kept.  info["sides"] = (name, group, r_eq, positions)."""
    pts = Points()
    rng = np.random.default_rng(700 + k)
    unit = pts.add(np.tile(np.r_[np.eye(3), -np.eye(3)], (834, 1))[:5000])
    near = pts.add(on_x(np.arange(1, 1024) / 2048.0))
    far = pts.add(on_x(1.0 + np.arange(1, 6001) / 1024.0))
    same = pts.add(np.tile([[0.5, 0.25, 0.125]], (1500, 1)))
    sides, names = [], []
    for name, n, pos in TIE_LAYOUTS:
        group = len(pos)
        for r_eq in sorted({1, min(group - 1, k - 1), min(group, k)} - {0}):
            n_less = k - r_eq
            rest = np.r_[rng.permutation(near)[:n_less], rng.permutation(far)[:n - group - n_less]]
            s = np.empty(n, np.int64)
            mask = np.zeros(n, bool)
            mask[pos] = True
            s[mask] = rng.permutation(unit[:group])  # the six unit points in turn
            s[~mask] = rng.permutation(rest)
            sides.append(s)
            names.append((name, group, r_eq, pos))
    sides.append(rng.permutation(same))
    names.append(("coincident", 1500, k, np.arange(1500)))
    s = rng.permutation(np.r_[near[:k - 1], far[:200]])
    s[len(s) // 2] = 0  # the origin: key 0, the nearest of all
    sides.append(s)
    names.append(("origin", None, None, None))
    s = rng.permutation(np.r_[near[:k - 2], far[:300]])
    at = np.nonzero(np.isin(s, far))[0][[0, 150, -1]]  # three farther points give way to one index at distance 1
    s[at] = unit[0]
    sides.append(s)
    names.append(("listed three times", 3, 2, at))
    coords, feats, spp = pts.scene(7)
    return Case("ties k=%d" % k, coords, feats, spp, pair_up(sides, ORIGIN), k=k, pool=False, sides=names,
                side_lists=sides)


# ---------------------------------------------------------------------------------------------- nearest 8: sizes
SIZE_K = (1, 2, 63, 64, 65, 1023, 1024)


@functools.lru_cache(maxsize=None)
def _size_scene():
    rng = np.random.default_rng(8)
    n = 31000
    coords = rng.integers(-12, 13, size=(n, 3)) / 4.0  # a coarse grid: exact distances from the origin and many ties
    coords[0] = 0.0
    return coords, rng.normal(size=(n, 6)).astype(np.float32), rng.integers(0, 100, n).astype(np.int64)


@functools.lru_cache(maxsize=None)
def size_case(k):
    """Long sides of n in {k + 1, 1024, 1025, 2048, 2049, 30 000} (those above k) and copied ones of {1, k - 1, k} points
    in shuffled order, a long and a copied side in one problem in either order, and two long ones together."""
    coords, feats, spp = _size_scene()
    rng = np.random.default_rng(80 + k)
    longs = sorted({m for m in (k + 1, 1024, 1025, 2048, 2049, 30000) if m > k})
    short = sorted({m for m in (1, k - 1, k) if m >= 1})
    problems, kinds = [], []
    for i, (m, c) in enumerate(zip(longs, itertools.cycle(short))):
        a, b = rng.permutation(len(spp))[:m], rng.permutation(len(spp))[:c]
        problems.append((a, b, ORIGIN) if i % 2 == 0 else (b, a, [0, 0, 0]))
        kinds.append((m, c) if i % 2 == 0 else (c, m))
    problems.append((rng.permutation(len(spp))[:longs[0]], rng.permutation(len(spp))[:longs[-1]], ORIGIN))
    kinds.append((longs[0], longs[-1]))
    return Case("sizes k=%d" % k, coords, feats, spp, problems, k=k, pool=False, kinds=kinds, longs=longs, short=short)


# ---------------------------------------------------------------------------------------------- nearest 9: centroid
CENTROID_T = (1, 255, 256, 257, 1024, 1025, 16384, 16385, 40000)
CENTROID_N = 45000
CENTROID_SCALES = ("1", "1e-300", "1e-150", "1e150", "1e300", "zeros", "inf elsewhere")


@functools.lru_cache(maxsize=None)
def centroid_case(scale="1"):
    """N = 45 000 (3 N coordinates: the abs-max grid strides), the largest |coordinate| in the array's last element, sides
    of 300 points at k = 40.  Scale "1": intersections of CENTROID_T entries (indices may repeat) in one call, and one of
    2 N entries that all name the last point.  The other scales: T = 1, 257 and 20 000 with every coordinate multiplied
    (1e+-300: the squares overflow / vanish and the list order decides; 1e+-150: they do not), all coordinates zero, or
    an infinite coordinate at a point of no problem."""
    rng = np.random.default_rng(9)
    n = CENTROID_N
    coords = rng.normal(scale=3.0, size=(n, 3))
    coords[n - 1] = (99.0, -99.5, 100.0)
    ts = CENTROID_T if scale == "1" else (1, 257, 20000)
    problems = [(rng.permutation(n - 10)[:300], rng.permutation(n - 10)[:300], rng.integers(0, n - 10, t)) for t in ts]
    if scale == "1":
        problems.append((rng.permutation(n - 10)[:300], rng.permutation(n - 10)[:300], np.full(2 * n, n - 1)))
    elif scale == "zeros":
        coords[:] = 0.0
    elif scale == "inf elsewhere":
        coords[n - 5, 1] = np.inf
    else:
        coords *= float(scale)
    return Case("centroid %s" % scale, coords, rng.normal(size=(n, 4)).astype(np.float32),
                rng.integers(0, 50, n).astype(np.int64), problems, k=40, pool=False, ts=ts)


# ---------------------------------------------------------------------------------------------- nearest 10: contraction
def _rn(x):
    """A rational rounded once to float64 (nearest, ties to even) -- what a fused multiply-add does with its exact sum."""
    return float(x)  # Fraction.__float__ divides exactly and rounds once


def fused_distances(d, pattern):
    """The distance of the offsets d[n, 3] if the compiler contracted (dx dx + dy dy) + dz dz into fused multiply-adds:
    "all"  fma(dz, dz, fma(dy, dy, dx dx));  "all_x"  fma(dz, dz, fma(dx, dx, dy dy));
    "xy"   fma(dx, dx, dy dy) + dz dz;        "z"      fma(dz, dz, dx dx + dy dy).    Exact rational arithmetic."""
    out = np.empty(len(d))
    for i, (x, y, z) in enumerate(np.asarray(d, dtype=np.float64)):
        fx, fy, fz = Fraction(x), Fraction(y), Fraction(z)
        if pattern == "all":
            out[i] = _rn(fz * fz + Fraction(_rn(fy * fy + Fraction(x * x))))
        elif pattern == "all_x":
            out[i] = _rn(fz * fz + Fraction(_rn(fx * fx + Fraction(y * y))))
        elif pattern == "xy":
            out[i] = _rn(fx * fx + Fraction(y * y)) + z * z
        elif pattern == "z":
            out[i] = _rn(fz * fz + Fraction(x * x + y * y))
        else:
            raise ValueError(pattern)
    return out


FUSED_PATTERNS = ("all", "xy", "z", "all_x")


def plain_distances(d):
    d = np.asarray(d, dtype=np.float64)
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def mirrored_pairs(count, seed=10):
    """Pairs (x, y, z) / (y, x, z): equal distances from a centroid with cx = cy when every operation is rounded on its
    own (the sum of the two rounded squares commutes), parted by one ulp under every contraction that fuses one of the x / y
    squares into the sum.  Random coordinates in [1, 2); only pairs parted under "all", "all_x" and "xy" are kept."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        x, y, z = 1.0 + rng.random(3)
        d = np.array([(x, y, z), (y, x, z)])
        assert plain_distances(d)[0] == plain_distances(d)[1]
        if all(np.diff(fused_distances(d, p))[0] != 0 for p in ("all", "all_x", "xy")):
            out.append(d)
    return out


def last_add_pairs():
    """Pairs parted by the fusion of the last addition alone.  (1, 0, z) with z z rounding UP to (j + 1/2) 2^-52, j odd:
    unfused, 1 + that is a tie and goes to the even 1 + (j + 1) 2^-52; fused, the exact z z lies below the tie and the sum
    goes to 1 + j 2^-52.  Its partner (1, a 2^-26, b 2^-26), a^2 + b^2 = j + 1, has the distance 1 + (j + 1) 2^-52 with no
    rounding anywhere, fused or not."""
    out = []
    for j in range(1, 255, 2):
        ab = next(((a, b) for a in range(16) for b in range(a + 1) if a * a + b * b == j + 1), None)
        if ab is None:
            continue
        tie = Fraction(2 * j + 1, 2) / 2 ** 52
        z0 = float(np.sqrt(float(tie)))
        for z in (np.nextafter(z0, 0), z0, np.nextafter(z0, 1)):
            z = float(z)
            if Fraction(z) ** 2 < tie and Fraction(z * z) == tie:
                out.append(np.array([(1.0, ab[0] * 2.0 ** -26, ab[1] * 2.0 ** -26), (1.0, 0.0, z)]))
                break
    return out


CONTRACT_K = 9


@functools.lru_cache(maxsize=None)
def contraction_case():
    """Four sides at k = 9, each of pairs that tie under the stated arithmetic: twelve mirrored pairs listed (first,
    second) and, in side 1, (second, first); the pairs of last_add_pairs() likewise in sides 2 and 3.  Four pairs lie inside
    the selection and the fifth on the cut, so a contraction that parts a pair swaps two rows or changes the last one."""
    pts = Points()
    rng = np.random.default_rng(10)
    sides = []
    for pairs in (mirrored_pairs(12), last_add_pairs()):
        idx = [pts.add(p) for p in pairs]
        order = rng.permutation(len(idx))
        sides.append(np.concatenate([idx[i] for i in order]))
        sides.append(np.concatenate([idx[i][::-1] for i in order]))
    coords, feats, spp = pts.scene(10)
    return Case("contraction", coords, feats, spp, pair_up(sides, ORIGIN), k=CONTRACT_K, pool=False, side_lists=sides)


# ---------------------------------------------------------------------------------------------- the calls of the GPU file
def workspace_layout(descs, n_spps, d, pool=True):
    """gapro_trainset_workspace_bytes as DESIGN.md 4.4 states it: pool  i32 marks[2 P S] | i64 sums[R D] | i32 counts[R]
    with R = sum over the sides of min(n, S), nearest  i64 centroid sums[3 P] | u64 max |coordinate|; every region
    rounded up to 256 bytes."""
    def up(x):
        return (x + 255) // 256 * 256

    p = len(descs)
    if not pool:
        return up((3 * p + 1) * 8)
    rows = sum(min(n1, n_spps) + min(n2, n_spps) for n1, n2, _ in descs)
    return up(2 * p * n_spps * 4) + up(rows * d * 8) + up(rows * 4)
