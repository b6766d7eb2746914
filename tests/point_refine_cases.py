"""Inputs and NumPy references of the edge tests of the point-level refine kernels (gapro_amd/csrc/point_refine.hip;
DESIGN.md 4.5): cases that put k_refine_gather, k_refine_mu_var, k_refine_apply, k_refine_expand, k_refine_compete and
k_refine_vote on their grid caps, their table edges and the ways block_of_row returns -1.

tests/test_point_refine_edges_cpu.py asserts that every constant below is the number in the source, that every case is
what its name says and passes the library's host checks (`check_blocks` restated here), and that every reference agrees
with a per-row loop; tests/test_point_refine_edges_gpu.py runs the cases through the entry points and compares bit for
bit.  The references are vectorised over rows (the cases reach half a million rows) and take a LIMIT (items, models,
candidates, blocks): the reference of a kernel that forgot to wrap its grid, which must differ from the full one.
A case is built once per process (the builders are cached); nobody may write into what they return."""
import functools

import numpy as np

import vote_ref
from gapro_amd import _lib

# ---------------------------------------------------------------------------------------------- what the source says
THREADS = 256            # constexpr int kThreads = 256; (and grid_for's 256 threads a workgroup, launch_util.h)
GATHER_CAP_FEW = 2048    # k_refine_gather / k_refine_mu_var: grid_for(n_max, 1, n_scenes >= 8 ? 256 : 2048), the ": 2048"
GATHER_CAP_MANY = 256    # ... the "? 256"
MANY_SCENES = 8          # ... the "n_scenes >= 8"
APPLY_CAP_FEW = 1024     # k_refine_apply: grid_for(t_max, 1, n_models >= 64 ? 64 : 1024), the ": 1024"
APPLY_CAP_MANY = 64      # ... the "? 64"
MANY_MODELS = 64         # ... the "n_models >= 64"
GRID_Y = 65535           # constexpr int kMaxGridY = 65535; the models of one k_refine_apply launch (lo += kMaxGridY)
ROW_CAP = 2048           # k_refine_expand / k_refine_compete: grid_for(n_rows, 1, 2048)
VOTE_MAX_SEG = 2048      # constexpr int kVoteMaxSeg = 2048;
VOTE_GRID = 1 << 18      # k_refine_vote: dim3((unsigned)std::min(n_blocks, 1 << 18))

SENT = -7                # what the tests fill integer outputs with
SENT_F = np.float32(-7.0)
SPARE = 8                # elements behind every output buffer that must keep the sentinel

BLOCK_DT = np.dtype(_lib.PointRefineBlock)
SEGMENT_DT = np.dtype(_lib.PointRefineSegment)
MODEL_DT = np.dtype(_lib.PointRefineModel)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def wide(rng, shape):
    """Magnitudes from 1e-30 to 1e6, either sign (tests/test_point_vote_gpu.py's _wide)."""
    return (rng.choice([-1.0, 1.0], size=shape) * 10.0 ** rng.uniform(-30, 6, size=shape)).astype(np.float32)


def block_table(blocks):
    out = np.zeros(len(blocks), BLOCK_DT)
    b = np.asarray(blocks, np.int64).reshape(-1, 5)
    out["row_start"], out["n_rows"], out["scene"], out["seg_start"], out["n_seg"] = b.T
    return out


def segment_table(segs):
    out = np.zeros(len(segs), SEGMENT_DT)
    g = np.asarray(segs, np.int64).reshape(-1, 2)
    out["out_start"], out["model"] = g.T
    return out


def model_table(pairs, scene, row_offset=None, t=None):
    out = np.zeros(len(pairs), MODEL_DT)
    p = np.asarray(pairs, np.int64).reshape(-1, 4)
    out["sem1"], out["inst1"], out["sem2"], out["inst2"] = p.T
    out["scene"] = scene
    if row_offset is not None:
        out["row_offset"], out["t"] = row_offset, t
    return out


# ---------------------------------------------------------------------------------------------- gather
def _gather_scene(rng, n, s, d, refined, inv=None):
    if inv is None:
        inv = rng.integers(0, s, size=n)
    return dict(n=int(n), S=int(s), inv=np.ascontiguousarray(inv, np.int32),
                feats=rng.normal(size=(n, d)).astype(np.float32), refined=[int(x) for x in refined])


def _gather_case(name, d, scenes, short=0):
    """Lays the blocks of the refined superpoints out in scene order, each as long as the superpoint has points with its
    id (ids outside [0, S) belong to nobody); `short` rows are cut off the end of the plan passed to the call."""
    rows = 0
    for sc in scenes:
        ok = (sc["inv"] >= 0) & (sc["inv"] < sc["S"])
        cnt = np.bincount(sc["inv"][ok], minlength=sc["S"])
        sp_row = np.full(sc["S"], -1, np.int64)
        for sp in sc["refined"]:
            assert cnt[sp] > 0 and sp_row[sp] < 0
            sp_row[sp] = rows
            rows += int(cnt[sp])
        sc["sp_row"], sc["count"] = sp_row, cnt
    return dict(name=name, d=d, scenes=scenes, R=rows, n_rows=rows - short)


GATHER_WIDTHS = (1, 6, 7, 32, 33)
GATHER_LENGTHS = (1, 255, 256, 257)
GATHER_MANY_LENGTHS = (1, 255, 256, 257, 1000, 3, GATHER_CAP_MANY * THREADS + 257, 2000)
GATHER_MANY_SPPS = (1, 5, 6, 7, 23, 2, 40, 31)
BIG_N = GATHER_CAP_FEW * THREADS + 300
BIG_SPP = 70000


@functools.lru_cache(maxsize=None)
def gather_width_case(d):
    """One scene of 1000 points at feature width d: the j / d regrouping through LDS."""
    rng = np.random.default_rng(100 + d)
    return _gather_case("width %d" % d, d, [_gather_scene(rng, 1000, 23, d, (0, 5, 6, 22))])


@functools.lru_cache(maxsize=None)
def gather_length_case(n):
    """One scene of n points (n % 256 in 0, 1, 255): the partial last run of kThreads points."""
    rng = np.random.default_rng(200 + n)
    s = min(n, 5)
    inv = rng.integers(0, s, size=n)
    inv[0], inv[-1] = 0, s - 1
    return _gather_case("length %d" % n, 6, [_gather_scene(rng, n, s, 6, sorted({0, s - 1}), inv)])


@functools.lru_cache(maxsize=None)
def gather_big_case():
    """One scene of GATHER_CAP_FEW * 256 + 300 points at D = 1: the 2048-workgroup grid wraps.  Superpoint 198 holds the
    first point alone, 199 the last point and four more of the 300 behind the cap, 7 holds 70 000 points (half of them
    one run, half scattered over the scene): one cursor for all of them."""
    rng = np.random.default_rng(300)
    n, s = BIG_N, 200
    inv = rng.integers(0, 198, size=n)
    inv[inv == 7] = 8
    at = np.r_[np.arange(100000, 100000 + BIG_SPP // 2), 150000 + rng.permutation(n - 150000 - 400)[:BIG_SPP // 2]]
    inv[at] = 7
    inv[0] = 198
    inv[[n - 1, n - 2, n - 77, n - 150, n - 299]] = 199
    return _gather_case("big", 1, [_gather_scene(rng, n, s, 1, (198, 199, 7, 50), inv)])


@functools.lru_cache(maxsize=None)
def gather_many_case():
    """Eight scenes in one call (the n_scenes >= 8 branch, 256 workgroups a scene): scene 6 is longer than the grid covers
    in one round while scenes 0 .. 5 are shorter than one workgroup or a few; scenes 0 and 5 refine nothing."""
    rng = np.random.default_rng(400)
    scenes = []
    for si, (n, s) in enumerate(zip(GATHER_MANY_LENGTHS, GATHER_MANY_SPPS)):
        inv = rng.integers(0, s, size=n)
        inv[0], inv[-1] = 0, s - 1
        refined = () if si in (0, 5) else sorted({0, s // 2, s - 1})
        scenes.append(_gather_scene(rng, n, s, 7, refined, inv))
    return _gather_case("many", 7, scenes)


@functools.lru_cache(maxsize=None)
def gather_short_case():
    """A plan one row short: the call gets n_rows = R - 1 and the last block's last position is row R - 1."""
    rng = np.random.default_rng(500)
    scenes = [_gather_scene(rng, 2000, 41, 7, (0, 9, 10, 40)), _gather_scene(rng, 2137, 37, 7, (3, 4, 25))]
    return _gather_case("short", 7, scenes, short=1)


@functools.lru_cache(maxsize=None)
def gather_guard_case():
    """Ids -1 and S in spp_inv at a few points (k_refine_gather's `sp >= 0 && sp < S`): those points get no row."""
    rng = np.random.default_rng(600)
    inv = rng.integers(0, 23, size=1000)
    inv[[0, 100, 255, 256, 999]] = -1
    inv[[1, 511, 998]] = 23
    return _gather_case("guard", 6, [_gather_scene(rng, 1000, 23, 6, (0, 5, 22), inv)])


def gather_reference(case, limit=None):
    """Per row of the plan: `scene` and `spp` of its block (-1 outside every block), `canon` = the points of the block's
    superpoint in ascending order (SENT where the block has no point left), `feats` = the bits of the canon point's
    features.  Only the first `limit` points of every scene exist (None: all)."""
    R, d = case["R"], case["d"]
    scene, spp = np.full(R, -1, np.int32), np.full(R, -1, np.int32)
    canon, feats = np.full(R, SENT, np.int32), np.full((R, d), bits(np.array([SENT_F]))[0], np.uint32)
    for si, sc in enumerate(case["scenes"]):
        ref = np.nonzero(sc["sp_row"] >= 0)[0]
        first = sc["sp_row"][ref]
        scene[np.repeat(first, sc["count"][ref]) + _ramp(sc["count"][ref])] = si
        spp[np.repeat(first, sc["count"][ref]) + _ramp(sc["count"][ref])] = np.repeat(ref, sc["count"][ref])
        inv = sc["inv"][:limit].astype(np.int64)
        ok = (inv >= 0) & (inv < sc["S"])
        ok[ok] = sc["sp_row"][inv[ok]] >= 0
        pts = np.nonzero(ok)[0]
        pts = pts[np.argsort(inv[pts], kind="stable")]  # by superpoint, ascending point inside
        ids, cnt = np.unique(inv[pts], return_counts=True)
        rows = np.repeat(sc["sp_row"][ids], cnt) + _ramp(cnt)
        canon[rows] = pts
        feats[rows] = bits(sc["feats"])[pts]
    return dict(scene=scene, spp=spp, canon=canon, feats=feats)


def _ramp(counts):
    """0 .. c - 1 for every c of counts, concatenated."""
    counts = np.asarray(counts, np.int64)
    return np.arange(int(counts.sum()), dtype=np.int64) - np.repeat(np.cumsum(counts) - counts, counts)


def check_gather(case, row_point, row_feats, cursors, ref=None):
    """What the contract says of a gather's outputs (arrays of R + SPARE rows, filled with the sentinels before the
    call; cursors = every scene's cursor table): inside [0, n_rows) every row of a block holds a point of the block's
    superpoint, no point twice, and that point's feature bits; everything else keeps the sentinel; a cursor counts the
    points of its refined superpoint.  Where the plan is complete the sorted points of a block are all of its points."""
    ref = ref or gather_reference(case)
    R, n_rows = case["R"], case["n_rows"]
    row_point, row_feats = np.asarray(row_point), bits(np.asarray(row_feats)).reshape(len(row_point), -1)
    assert row_point.dtype == np.int32 and len(row_point) == R + SPARE and row_feats.shape == (R + SPARE, case["d"])
    sent_f = bits(np.array([SENT_F]))[0]
    written = np.zeros(R + SPARE, bool)
    written[:n_rows] = ref["scene"][:n_rows] >= 0
    assert np.array_equal(row_point != SENT, written), "%d rows written, %d expected" % ((row_point != SENT).sum(),
                                                                                        written.sum())
    assert (row_feats[~written] == sent_f).all()
    seen = 0
    for si, sc in enumerate(case["scenes"]):
        rows = np.nonzero(written[:R] & (ref["scene"] == si))[0]
        pts = row_point[rows].astype(np.int64)
        assert ((pts >= 0) & (pts < sc["n"])).all(), si
        assert np.array_equal(sc["inv"][pts], ref["spp"][rows]), "scene %d: a point in another superpoint's block" % si
        assert len(np.unique(pts)) == len(pts), "scene %d: a point gathered twice" % si
        assert np.array_equal(row_feats[rows], bits(sc["feats"])[pts]), "scene %d: feature bits" % si
        assert np.array_equal(cursors[si], np.where(sc["sp_row"] >= 0, sc["count"], 0)), "scene %d: cursors" % si
        seen += len(rows)
    assert seen == written.sum()
    if n_rows == R:  # the order inside a block is free: sorted by (block, point) the rows are the canonical ones
        first = np.zeros(R, np.int64)
        for si, sc in enumerate(case["scenes"]):
            m = ref["scene"] == si
            first[m] = sc["sp_row"][ref["spp"][m]]
        inside = ref["scene"] >= 0
        got = row_point[:R].copy()
        order = np.lexsort((got[inside], first[inside]))
        got[inside] = got[inside][order]
        assert np.array_equal(got, ref["canon"])
    return int(written.sum())


def gather_loop(case, order_seed=0, limit=None):
    """k_refine_gather one point at a time, the points of a scene in a shuffled order (the atomics' order is free):
    (row_point, row_feats, cursors) as the device would leave them.  Slow; for small cases."""
    rng = np.random.default_rng(order_seed)
    R, d, n_rows = case["R"], case["d"], case["n_rows"]
    rp, rf = np.full(R + SPARE, SENT, np.int32), np.full((R + SPARE, d), SENT_F, np.float32)
    cursors = []
    for sc in case["scenes"]:
        cur = np.zeros(sc["S"], np.int32)
        n = sc["n"] if limit is None else min(sc["n"], limit)
        for i in rng.permutation(n):
            sp = int(sc["inv"][i])
            if sp < 0 or sp >= sc["S"] or sc["sp_row"][sp] < 0:
                continue
            row = int(sc["sp_row"][sp]) + int(cur[sp])
            cur[sp] += 1
            if row >= n_rows:
                continue
            rp[row], rf[row] = i, sc["feats"][i]
        cursors.append(cur)
    return rp, rf, cursors


# ---------------------------------------------------------------------------------------------- apply
APPLY_MANY_T = (0, 1, 255, 256, 257)
APPLY_BIG_MANY = APPLY_CAP_MANY * THREADS + 70
APPLY_BIG_FEW = APPLY_CAP_FEW * THREADS + 5
BAD_POINTS = (-1, None, 2 ** 31 - 1)  # None: the scene's n_points


def _apply_case(name, seed, ts, scene_of, failed=(), bad_rows=(), gap=3, extra_points=50, n_scenes=None):
    """Models of ts[k] rows in scene scene_of[k], laid out in model order with `gap` unused rows between two models; the
    rows of a scene's models hold distinct points of it (a permutation), except `bad_rows`, which get BAD_POINTS."""
    rng = np.random.default_rng(seed)
    ts, scene_of = np.asarray(ts, np.int64), np.asarray(scene_of, np.int64)
    nm = len(ts)
    n_scenes = n_scenes or (int(scene_of.max()) + 1 if nm else 1)
    off = np.cumsum(ts + gap) - (ts + gap)
    n_rows = int(off[-1] + ts[-1] + gap) if nm else 0
    row_model = np.full(n_rows, -1, np.int64)
    row_model[np.repeat(off, ts) + _ramp(ts)] = np.repeat(np.arange(nm), ts)
    row_point = rng.integers(0, 2, size=n_rows).astype(np.int32)  # rows of no model: never read
    n_pts, spps, inv, mu_spp, var_spp, start = [], [], [], [], [], []
    for si in range(n_scenes):
        mine = np.nonzero((row_model >= 0) & (scene_of[np.maximum(row_model, 0)] == si))[0]
        n = len(mine) + extra_points
        row_point[mine] = rng.permutation(n)[:len(mine)]
        s = 3 + 4 * si
        n_pts.append(n)
        spps.append(s)
        inv.append(rng.integers(0, s, size=n).astype(np.int32))
        mu_spp.append(rng.normal(size=s).astype(np.float32))
        var_spp.append(rng.uniform(0.1, 2, size=s).astype(np.float32))
        start.append((rng.integers(-5, 0, n).astype(np.int32), rng.integers(-9, -5, n).astype(np.int32),
                      rng.uniform(2, 3, n).astype(np.float32)))
    for r, bad in zip(bad_rows, BAD_POINTS):
        row_point[r] = n_pts[scene_of[row_model[r]]] if bad is None else bad
    status = np.zeros(nm, np.int32)
    status[list(failed)] = -5
    return dict(name=name, n_scenes=n_scenes, n_pts=n_pts, spps=spps, inv=inv, mu_spp=mu_spp, var_spp=var_spp, start=start,
                t=ts, off=off, scene_of=scene_of, pairs=rng.integers(0, 40, size=(nm, 4)).astype(np.int32), status=status,
                n_rows=n_rows, row_point=row_point, pn=rng.uniform(0.5, 1, n_rows).astype(np.float32),
                lab=rng.choice(np.array([0, 1, 255], np.uint8), size=n_rows), mu=rng.normal(size=n_rows).astype(np.float32),
                var=rng.uniform(0.1, 2, n_rows).astype(np.float32), bad_rows=tuple(bad_rows), failed=tuple(failed))


@functools.lru_cache(maxsize=None)
def apply_many_case():
    """3 scenes, 70 models (the n_models >= 64 grid of 64 workgroups): model 33 has APPLY_CAP_MANY * 256 + 70 rows, the
    others t = 0, 1, 255, 256, 257 in turn, model k in scene k % 3; models 2, 9, 13, 40 and 69 have status -5; three
    rows of model 33 (the first, one behind the cap, the last) hold points outside the scene."""
    ts = [APPLY_MANY_T[k % 5] for k in range(70)]
    ts[33] = APPLY_BIG_MANY
    off33 = sum(t + 3 for t in ts[:33])
    bad = (off33, off33 + APPLY_CAP_MANY * THREADS + 3, off33 + APPLY_BIG_MANY - 1)
    return _apply_case("many", 1, ts, [k % 3 for k in range(70)], failed=(2, 9, 13, 40, 69), bad_rows=bad)


@functools.lru_cache(maxsize=None)
def apply_few_case():
    """5 models (the 1024-workgroup grid), model 2 of APPLY_CAP_FEW * 256 + 5 rows."""
    return _apply_case("few", 2, [7, 300, APPLY_BIG_FEW, 0, 256], [0, 1, 1, 0, 0], failed=(1,))


@functools.lru_cache(maxsize=None)
def apply_grid_y_case():
    """GRID_Y + 3 models of 1 to 3 rows: the last three run in the second launch of the `lo += 65535` loop, and model
    GRID_Y + 1 has status -5 (the second launch's status pointer is offset like its model pointer); so has model 2:
    without the offset the second launch would skip model GRID_Y + 2 and run model GRID_Y + 1."""
    nm = GRID_Y + 3
    rng = np.random.default_rng(3)
    return _apply_case("grid.y", 3, rng.integers(1, 4, size=nm), rng.integers(0, 2, size=nm), failed=(2, GRID_Y + 1), gap=0)


@functools.lru_cache(maxsize=None)
def apply_no_rows_case():
    """Four models, all with t == 0 (t_max == 0: k_refine_apply is not launched)."""
    return _apply_case("t == 0", 4, [0, 0, 0, 0], [0, 1, 0, 1], gap=1)


@functools.lru_cache(maxsize=None)
def mu_var_case(many=False):
    """No model, the mu / var pass alone: scenes of 1 and of GATHER_CAP_FEW * 256 + 300 points, or (many) the eight
    scene lengths of gather_many_case."""
    lengths = GATHER_MANY_LENGTHS if many else (1, BIG_N)
    c = _apply_case("mu / var %d" % len(lengths), 5, [], [], n_scenes=len(lengths))
    rng = np.random.default_rng(55)
    for si, n in enumerate(lengths):
        s = c["spps"][si]
        c["n_pts"][si] = n
        c["inv"][si] = rng.integers(0, s, size=n).astype(np.int32)
        c["inv"][si][-1] = s - 1
        c["start"][si] = (np.full(n, -3, np.int32), np.full(n, -4, np.int32), np.full(n, 2.5, np.float32))
    return c


def apply_reference(c, use_status=True, k_limit=None, model_limit=None, point_limit=None):
    """Per scene (sem, inst, prob, mu, var) after gapro_point_refine_apply: mu / var = the superpoint's, then the five
    values of every row of every live model at the row's point.  The limits are those of a kernel that does not wrap:
    only the first k_limit rows of a model, only the first model_limit models, only the first point_limit points of
    the mu / var pass (those behind keep SENT_F)."""
    out = []
    for si in range(c["n_scenes"]):
        sem, ins, prob = (a.copy() for a in c["start"][si])
        mu, var = c["mu_spp"][si][c["inv"][si]], c["var_spp"][si][c["inv"][si]]
        if point_limit is not None:
            mu[point_limit:], var[point_limit:] = SENT_F, SENT_F
        out.append([sem, ins, prob, mu, var])
    nm = len(c["t"]) if model_limit is None else min(len(c["t"]), model_limit)
    t = c["t"][:nm].copy()
    if k_limit is not None:
        t = np.minimum(t, k_limit)
    if use_status:
        t[c["status"][:nm] != 0] = 0
    m = np.repeat(np.arange(nm), t)
    r = np.repeat(c["off"][:nm], t) + _ramp(t)
    i = c["row_point"][r].astype(np.int64)
    sc = c["scene_of"][m]
    ok = (i >= 0) & (i < np.asarray(c["n_pts"], np.int64)[sc]) if len(m) else np.zeros(0, bool)
    second = c["lab"][r] != 0
    for si in range(c["n_scenes"]):
        sel = ok & (sc == si)
        p, mm, rr, s2 = i[sel], m[sel], r[sel], second[sel]
        sem, ins, prob, mu, var = out[si]
        sem[p] = np.where(s2, c["pairs"][mm, 2], c["pairs"][mm, 0])
        ins[p] = np.where(s2, c["pairs"][mm, 3], c["pairs"][mm, 1])
        prob[p], mu[p], var[p] = c["pn"][rr], c["mu"][rr], c["var"][rr]
    return out


def apply_loop(c, use_status=True):
    """The same, one row at a time."""
    out = []
    for si in range(c["n_scenes"]):
        sem, ins, prob = (a.copy() for a in c["start"][si])
        mu, var = np.empty(c["n_pts"][si], np.float32), np.empty(c["n_pts"][si], np.float32)
        for i in range(c["n_pts"][si]):
            mu[i], var[i] = c["mu_spp"][si][c["inv"][si][i]], c["var_spp"][si][c["inv"][si][i]]
        out.append([sem, ins, prob, mu, var])
    for k in range(len(c["t"])):
        if use_status and c["status"][k] != 0:
            continue
        sem, ins, prob, mu, var = out[c["scene_of"][k]]
        for j in range(int(c["t"][k])):
            r = int(c["off"][k]) + j
            i = int(c["row_point"][r])
            if i < 0 or i >= c["n_pts"][c["scene_of"][k]]:
                continue
            second = c["lab"][r] != 0
            sem[i], ins[i] = c["pairs"][k][2 if second else 0], c["pairs"][k][3 if second else 1]
            prob[i], mu[i], var[i] = c["pn"][r], c["mu"][r], c["var"][r]
    return out


# ---------------------------------------------------------------------------------------------- blocks and segments
def check_blocks(blocks, segs, n_rows, n_rows2, n_scenes=-1, n_models=-1):
    """point_refine.hip's check_blocks: None, or the complaint of the first block that fails (blocks i64[nb, 5] =
    row_start, n_rows, scene, seg_start, n_seg; segs i64[ng, 2] = out_start, model)."""
    b, g = np.asarray(blocks, np.int64).reshape(-1, 5), np.asarray(segs, np.int64).reshape(-1, 2)
    if not len(b):
        return None
    rs, n, sc, s0, ns = b.T
    end = np.r_[0, (rs + n)[:-1]]
    code = np.zeros(len(b), np.int64)

    def mark(bad, k):
        code[(code == 0) & bad] = k

    mark((n <= 0) | (rs < end) | (rs > n_rows - n), 1)
    bad_segs = (ns < 0) | (s0 < 0) | (s0 > len(g) - ns)
    mark(bad_segs, 2)
    if n_scenes >= 0:
        mark((sc < 0) | (sc >= n_scenes), 3)
    cnt = np.where(bad_segs, 0, ns)
    of = np.repeat(np.arange(len(b)), cnt)
    sg = g[np.repeat(s0, cnt) + _ramp(cnt)]
    bad_out = (sg[:, 0] < 0) | (sg[:, 0] > n_rows2 - n[of])
    bad_model = (sg[:, 1] < 0) | (sg[:, 1] >= n_models) if n_models >= 0 else np.zeros(len(sg), bool)
    first_bad = np.full(len(b), np.iinfo(np.int64).max)
    np.minimum.at(first_bad, of[bad_out | bad_model], np.nonzero(bad_out | bad_model)[0])
    has = first_bad < np.iinfo(np.int64).max
    kind = np.zeros(len(b), np.int64)
    kind[has] = np.where(bad_out[first_bad[has]], 4, 5)
    code[(code == 0) & has] = kind[(code == 0) & has]  # the segment complaints come last inside a block
    bad = np.nonzero(code)[0]
    if not len(bad):
        return None
    return {1: "a block outside the rows or out of order", 2: "a block's segments outside the segments",
            3: "a block of no scene", 4: "a segment outside the expanded rows",
            5: "a segment of no model"}[int(code[bad[0]])]


def block_of_rows(blocks, n_rows):
    """Per gathered row the index of the block that holds it, -1 for a row in front of the first block, in a gap or
    behind the last one (point_refine.hip's block_of_row for every row)."""
    b = np.asarray(blocks, np.int64).reshape(-1, 5)
    r = np.arange(n_rows, dtype=np.int64)
    k = np.searchsorted(b[:, 0], r, side="right") - 1
    inside = (k >= 0) & (r - b[np.maximum(k, 0), 0] < b[np.maximum(k, 0), 1])
    return np.where(inside, k, -1)


def first_maximum(p):
    """The rule of "compete" for every row at once: p f32[n_seg, n]; best = 0.0f; for k in order: where best < p[k]
    (strict, float32; False for a NaN) take k.  Returns the taking position per row, -1 where nobody took it."""
    p = np.asarray(p, np.float32)
    p = p.reshape(len(p), -1)
    best, took = np.zeros(p.shape[1], np.float32), np.full(p.shape[1], -1, np.int64)
    for k in range(p.shape[0]):
        with np.errstate(invalid="ignore"):
            m = best < p[k]
        best[m], took[m] = p[k][m], k
    return took


def contract_reference(c, start, row_limit=None):
    """NumPy: d_rows, and the five arrays of both scenes (from their `start` values) and row_model after compete.
    Vectorised over the rows of a block; only the first row_limit gathered rows are looked at (None: all)."""
    rows = np.full(c["R2"], SENT, np.int32)
    outs = [[a.copy() for a in sc] for sc in start]
    row_model = np.full(c["R"], -1, np.int32)
    for r0, n, si, s0, ns in c["blocks"]:
        if row_limit is not None:
            n = min(n, max(0, row_limit - r0))
        sg = c["segs"][s0:s0 + ns]
        for o, _ in sg:
            rows[o:o + n] = np.arange(r0, r0 + n)
        live = [(o, m) for o, m in sg if c["status"][m] == 0]
        if not live or n <= 0:
            continue
        k = first_maximum(np.stack([c["pn"][o:o + n] for o, _ in live]))
        i = c["row_point"][r0:r0 + n].astype(np.int64)
        j = np.nonzero((k >= 0) & (i >= 0) & (i < c["n_pts"][si]))[0]
        o = np.array([o for o, _ in live], np.int64)[k[j]] + j
        m = np.array([m for _, m in live], np.int64)[k[j]]
        second = c["lab"][o] != 0
        sem, ins, prob, mu, var = outs[si]
        sem[i[j]] = np.where(second, c["pairs"][m, 2], c["pairs"][m, 0])
        ins[i[j]] = np.where(second, c["pairs"][m, 3], c["pairs"][m, 1])
        prob[i[j]], mu[i[j]], var[i[j]] = c["pn"][o], c["mu"][o], c["var"][o]
        row_model[r0 + j] = m
    return rows, outs, row_model


def contract_loop(c, start):
    """The same, one row and one segment at a time."""
    rows = np.full(c["R2"], SENT, np.int32)
    outs = [[a.copy() for a in sc] for sc in start]
    row_model = np.full(c["R"], -1, np.int32)
    for r0, n, si, s0, ns in c["blocks"]:
        for j in range(n):
            best, took = np.float32(0), -1
            for s in range(s0, s0 + ns):
                o, m = c["segs"][s]
                rows[o + j] = r0 + j
                if c["status"][m] != 0:
                    continue
                if best < c["pn"][o + j]:
                    best, took = c["pn"][o + j], s
            i = c["row_point"][r0 + j]
            if took < 0 or i < 0 or i >= c["n_pts"][si]:
                continue
            o, m = c["segs"][took]
            second = c["lab"][o + j] != 0
            sem, ins, prob, mu, var = outs[si]
            sem[i], ins[i] = c["pairs"][m][2 if second else 0], c["pairs"][m][3 if second else 1]
            prob[i], mu[i], var[i] = c["pn"][o + j], c["mu"][o + j], c["var"][o + j]
            row_model[r0 + j] = m
    return rows, outs, row_model


def build_blocks(spec, first_row=0, gaps=(0,), tail=0, hole=0, seed=0, quantum=None):
    """The shared block builder.  spec = [(scene, n_rows, [model per segment])]; the blocks are laid out in this order
    from `first_row` on with gaps[k % len(gaps)] unused rows behind block k and `tail` rows behind the last one; the
    segments take their expanded rows in a shuffled order with `hole` unused rows behind each.  p_new is random in
    [0.5, 1), in steps of `quantum` where given (many exact ties); labels, mu and var are random.  Fills everything of
    the dictionary the references read except models, status and the rows' points."""
    rng = np.random.default_rng(seed)
    blocks, segs, row = [], [], first_row
    for k, (si, n, ms) in enumerate(spec):
        blocks.append([row, n, si, len(segs), len(ms)])
        segs += [[-1, m] for m in ms]
        row += n + (gaps[k % len(gaps)] if k + 1 < len(spec) else 0)
    R = row + tail
    of = np.repeat(np.arange(len(blocks)), [b[4] for b in blocks])
    R2 = 0
    for g in rng.permutation(len(segs)):
        segs[g][0] = R2
        R2 += blocks[of[g]][1] + hole
    pn = rng.uniform(0.5, 1, size=R2).astype(np.float32)
    if quantum:
        pn = (np.floor(pn * quantum) / quantum).astype(np.float32)
    return dict(blocks=np.array(blocks, np.int64).reshape(-1, 5), segs=np.array(segs, np.int64).reshape(-1, 2), R=R, R2=R2,
                pn=pn, lab=rng.choice(np.array([0, 1, 255], np.uint8), size=R2),
                mu=rng.normal(size=R2).astype(np.float32), var=rng.uniform(0.1, 2, size=R2).astype(np.float32))


def _compete_fill(c, seed, n_scenes=2, models_per_scene=4):
    """Models (the last one of every scene has status -5) and the rows' points: a permutation of each scene's points,
    100 more points than rows; the rows outside every block hold a valid point that nobody may read."""
    rng = np.random.default_rng(seed)
    nm = n_scenes * models_per_scene
    c["model_scene"] = np.repeat(np.arange(n_scenes), models_per_scene).astype(np.int32)
    c["status"] = np.zeros(nm, np.int32)
    c["status"][models_per_scene - 1::models_per_scene] = -5
    c["pairs"] = rng.integers(0, 40, size=(nm, 4)).astype(np.int32)
    of = block_of_rows(c["blocks"], c["R"])
    c["row_point"] = np.zeros(c["R"], np.int32)
    c["n_pts"] = []
    for si in range(n_scenes):
        mine = np.nonzero((of >= 0) & (c["blocks"][np.maximum(of, 0), 2] == si))[0]
        n = len(mine) + 100
        c["row_point"][mine] = rng.permutation(n)[:len(mine)]
        c["n_pts"].append(n)
    return c


EDGE_SIZES = (1, 255, 256, 257)
EDGE_R = ROW_CAP * THREADS + 1000
EDGE_FIRST, EDGE_GAPS, EDGE_TAIL, EDGE_HOLE = 5, (1, 300), 40, 3


@functools.lru_cache(maxsize=None)
def compete_edge_case():
    """R = ROW_CAP * 256 + 1000 gathered rows: the first block starts at row 5, gaps of 1 and of 300 rows alternate
    between the blocks, 40 rows lie behind the last one, which is the large block that reaches over the grid's cap.
    Sizes 1, 255, 256, 257 twice over, one block of 9 rows without a segment, 2 to 3 segments elsewhere; holes of 3 rows
    behind every segment of the expanded rows.  A scene's models: three live ones and one with status -5."""
    rng = np.random.default_rng(71)
    spec = []
    for k, n in enumerate(EDGE_SIZES + EDGE_SIZES):
        si = k % 2
        spec.append((si, n, [int(m) for m in 4 * si + rng.permutation(4)[:2 + k % 2]]))
    spec.insert(3, (1, 9, []))
    used = EDGE_FIRST + sum(n for _, n, _ in spec) + sum(EDGE_GAPS[k % 2] for k in range(len(spec))) + EDGE_TAIL
    spec.append((0, EDGE_R - used, [2, 3, 0]))
    c = build_blocks(spec, EDGE_FIRST, EDGE_GAPS, EDGE_TAIL, EDGE_HOLE, seed=72, quantum=64)
    c["spec"] = spec
    return _compete_fill(c, 73)


@functools.lru_cache(maxsize=None)
def compete_single_case():
    """n_blocks == 1: rows [300, 800) of 1000, so the bisection never iterates and rows lie on both sides."""
    c = build_blocks([(0, 500, [1, 3, 0, 2])], 300, tail=200, hole=EDGE_HOLE, seed=74, quantum=64)
    return _compete_fill(c, 75, n_scenes=1)


@functools.lru_cache(maxsize=None)
def compete_small_case():
    """The edge case's layout at a size the per-row loop can run."""
    spec = [(0, 1, [0, 1]), (1, 7, [5, 4, 6]), (0, 4, []), (1, 3, [7, 5]), (0, 30, [3, 2, 0])]
    c = build_blocks(spec, EDGE_FIRST, EDGE_GAPS, EDGE_TAIL, EDGE_HOLE, seed=76, quantum=8)
    return _compete_fill(c, 77)


def compete_start(c, seed=3):
    rng = np.random.default_rng(seed)
    return [(rng.integers(-5, 0, n).astype(np.int32), rng.integers(-9, -5, n).astype(np.int32),
             np.full(n, 1, np.float32), rng.normal(size=n).astype(np.float32) - 50, np.full(n, -100, np.float32))
            for n in c["n_pts"]]


# ---------------------------------------------------------------------------------------------- vote
VOTE_SEGS = (0, 1, 127, 128, 129, 300, VOTE_MAX_SEG)
VOTE_ROWS = 300
VOTE_MODELS = 40
VOTE_BIG_ROWS = 70000
# models 0 .. 35 argue for boxes 0 .. 11; the last four are kept for the candidates the 129 and 300 blocks are about
VOTE_SPECIAL = {36: (20, 21), 37: (22, 20), 38: (23, 24), 39: (25, 26)}


def _vote_models(rng):
    boxes = np.zeros((VOTE_MODELS, 2), np.int32)
    for m in range(36):
        boxes[m] = rng.permutation(12)[:2]
    for m, b in VOTE_SPECIAL.items():
        boxes[m] = b
    cls = (np.arange(30) * 3 + 1).astype(np.int32)
    pairs = np.array([[cls[b1], b1 if b1 < 22 else -100, cls[b2], b2 if b2 < 22 else -100] for b1, b2 in boxes], np.int32)
    return boxes, pairs


def _vote_takers(c, k, plan, rng):
    """Makes the rows of block k be taken as `plan` says: [(segment, label, rows)].  The taking segment holds a p_new in
    [0.8, 1), every other segment of the row one below 0.5."""
    r0, n, _, s0, ns = c["blocks"][k]
    assert sum(cnt for _, _, cnt in plan) == n
    who = rng.permutation(np.repeat(np.arange(len(plan)), [cnt for _, _, cnt in plan]))
    for s in range(ns):
        o = c["segs"][s0 + s][0]
        c["pn"][o:o + n] = rng.uniform(0.05, 0.5, n).astype(np.float32)
    for j, w in enumerate(who):
        s, lb, _ = plan[w]
        o = c["segs"][s0 + s][0]
        c["pn"][o + j], c["lab"][o + j] = np.float32(rng.uniform(0.8, 1)), (255 if lb and j % 2 else lb)


def _random_plan(ns, n, rng, among=None, parts=12):
    segs = rng.choice(np.arange(ns) if among is None else among, size=min(parts, ns), replace=False)
    cnt = np.bincount(rng.integers(0, len(segs), n), minlength=len(segs))
    return [(int(s), int(rng.integers(0, 2)), int(k)) for s, k in zip(segs, cnt) if k]


@functools.lru_cache(maxsize=None)
def vote_edge_case():
    """Blocks of n_seg in VOTE_SEGS, 300 rows each, segments drawn from models 0 .. 35 (twelve boxes: many segments
    argue for one box, on both sides of candidate 256).  Block 129: segment 128 (candidates 256, 257) is model 36 and
    takes 101 rows with label 0 -- box 20, which nobody else argues --, segment 5 is model 38 and takes 100 for box 23,
    the other 99 rows go to boxes 0 .. 11.  Block 300: box 20 gets 60 rows from segment 200 (model 36, label 0) and 41
    from segment 250 (model 37, label 1), box 23 gets 100 from segment 3.  In both, a loop that stopped at candidate 255
    would elect box 23.  The big blocks spread their rows over segments on both sides of 128."""
    rng = np.random.default_rng(81)
    spec = []
    for k, ns in enumerate(VOTE_SEGS):
        ms = [int(m) for m in rng.integers(0, 36, size=ns)]
        if ns == 129:
            ms[128], ms[5] = 36, 38
        if ns == 300:
            ms[200], ms[250], ms[3] = 36, 37, 38
        spec.append((k % 2, VOTE_ROWS, ms))
    c = build_blocks(spec, 2, (0, 4), 6, 0, seed=82)
    c["mu"], c["var"] = wide(rng, c["R2"]), np.abs(wide(rng, c["R2"]))
    c["boxes"], c["pairs"] = _vote_models(rng)
    c["status"] = np.zeros(VOTE_MODELS, np.int32)
    c["plans"] = {}
    for k, ns in enumerate(VOTE_SEGS):
        if ns == 0:
            continue
        if ns == 129:
            others = [s for s in range(ns) if s not in (128, 5)]
            plan = [(128, 0, 101), (5, 0, 100)] + _random_plan(ns, 99, rng, others)
        elif ns == 300:
            others = [s for s in range(ns) if s not in (200, 250, 3)]
            plan = [(200, 0, 60), (250, 1, 41), (3, 0, 100)] + _random_plan(ns, 99, rng, others)
        elif ns > 129:
            plan = _random_plan(ns, VOTE_ROWS, rng, parts=40)
        else:
            plan = _random_plan(ns, VOTE_ROWS, rng)
        _vote_takers(c, k, plan, rng)
        c["plans"][ns] = plan
    n_spps, block_spp = [], np.zeros(len(spec), np.int32)
    for si in range(2):
        mine = [k for k, b in enumerate(c["blocks"]) if b[2] == si]
        block_spp[mine] = rng.permutation(len(mine) + 5)[:len(mine)]
        n_spps.append(len(mine) + 5)
    c["block_spp"], c["n_spps"], c["spec"] = block_spp, n_spps, spec
    return c


@functools.lru_cache(maxsize=None)
def vote_big_case():
    """One block of 70 000 rows and three segments, mu of mixed sign and magnitudes from 1e-30 to 1e6: the shift of the
    exact sums at a large n."""
    rng = np.random.default_rng(83)
    c = build_blocks([(0, VOTE_BIG_ROWS, [3, 36, 38])], seed=84)
    c["mu"], c["var"] = wide(rng, c["R2"]), np.abs(wide(rng, c["R2"]))
    c["boxes"], c["pairs"] = _vote_models(rng)
    c["status"] = np.zeros(VOTE_MODELS, np.int32)
    c["block_spp"], c["n_spps"] = np.array([2], np.int32), [4]
    return c


VOTE_PATTERNS = 16


@functools.lru_cache(maxsize=None)
def vote_grid_case(n_blocks=VOTE_GRID + 3):
    """n_blocks blocks of one row and one segment each over one scene with as many superpoints: block b is superpoint
    perm[b], its model b % 4 (the last three: model 36) and its row one of 16 patterns (p_new, label, mu, var)."""
    rng = np.random.default_rng(85)
    nb = n_blocks
    blocks = np.zeros((nb, 5), np.int64)
    blocks[:, 0], blocks[:, 1], blocks[:, 3], blocks[:, 4] = np.arange(nb), 1, np.arange(nb), 1
    model = (np.arange(nb) % 4).astype(np.int64)
    model[-3:] = 36
    segs = np.stack([rng.permutation(nb).astype(np.int64), model], axis=1)
    pat = rng.integers(0, VOTE_PATTERNS, size=nb)
    pat[-3:] = 0, 1, 2  # (not the pattern nobody takes)
    pats = dict(pn=rng.uniform(0.5, 1, VOTE_PATTERNS).astype(np.float32),
                lab=rng.choice(np.array([0, 1, 255], np.uint8), VOTE_PATTERNS), mu=wide(rng, VOTE_PATTERNS),
                var=np.abs(wide(rng, VOTE_PATTERNS)))
    pats["pn"][5] = np.nan  # a row nobody takes
    c = dict(blocks=blocks, segs=segs, R=nb, R2=nb, pattern=pat, patterns=pats)
    for key, v in pats.items():
        c[key] = np.empty(nb, v.dtype)
        c[key][segs[:, 0]] = v[pat]
    c["boxes"], c["pairs"] = _vote_models(rng)
    c["status"] = np.zeros(VOTE_MODELS, np.int32)
    c["block_spp"], c["n_spps"] = rng.permutation(nb).astype(np.int32), [nb]
    return c


def vote_start(c, seed=4):
    rng = np.random.default_rng(seed)
    return [(rng.integers(-5, 0, s).astype(np.int32), rng.integers(-9, -5, s).astype(np.int32),
             np.full(s, 2, np.float32), rng.normal(size=s).astype(np.float32) - 50, np.full(s, -100, np.float32))
            for s in c["n_spps"]]


def vote_reference(c, start, seg_limit=None, block_limit=None):
    """vote_ref.vote_block per block -> the five tables of every scene (from `start`) and block_out i32[nb, 3].
    seg_limit: only the first seg_limit segments of a block exist (the candidates below 2 * seg_limit);
    block_limit: only the first block_limit blocks are voted, the others keep SENT in block_out."""
    tabs = [[a.copy() for a in sc] for sc in start]
    block_out = np.full((len(c["blocks"]), 3), SENT, np.int32)
    for k, (r0, n, si, s0, ns) in enumerate(c["blocks"][:block_limit]):
        sg = c["segs"][s0:s0 + (ns if seg_limit is None else min(ns, seg_limit))]
        r = None
        if len(sg):
            cut = lambda arr: np.stack([arr[o:o + n] for o, _ in sg])  # noqa: E731
            r = vote_ref.vote_block(int(n), [tuple(c["boxes"][m]) for _, m in sg], [c["status"][m] == 0 for _, m in sg],
                                    cut(c["pn"]), cut(c["lab"]), cut(c["mu"]), cut(c["var"]))
        if r is None:
            block_out[k] = -1, -1, 0
            continue
        m = int(sg[r["seg"]][1])
        sp = c["block_spp"][k]
        sem, ins, prob, mu, var = tabs[si]
        sem[sp], ins[sp] = c["pairs"][m][2 if r["second"] else 0], c["pairs"][m][3 if r["second"] else 1]
        prob[sp], mu[sp], var[sp] = r["prob"], r["mu"], r["var"]
        block_out[k] = m, r["box"], r["votes"]
    return tabs, block_out


def vote_grid_reference(c, start, block_limit=None):
    """vote_reference for vote_grid_case without a loop over its blocks: vote_ref.vote_block once per (model, pattern)
    that occurs, the results dealt to the blocks that hold the pair."""
    nb = len(c["blocks"]) if block_limit is None else min(len(c["blocks"]), block_limit)
    model, pat, p = c["segs"][:nb, 1], c["pattern"][:nb], c["patterns"]
    key = model * VOTE_PATTERNS + pat
    uniq, inv = np.unique(key, return_inverse=True)
    vals = np.zeros(len(uniq), [("ok", bool), ("sem", np.int32), ("ins", np.int32), ("prob", np.float32), ("mu", np.float32),
                                ("var", np.float32), ("out", np.int32, 3)])
    for u, kk in enumerate(uniq):
        m, q = int(kk) // VOTE_PATTERNS, int(kk) % VOTE_PATTERNS
        row = [p[name][q:q + 1][None] for name in ("pn", "lab", "mu", "var")]
        r = vote_ref.vote_block(1, [tuple(c["boxes"][m])], [c["status"][m] == 0], *row)
        if r is None:
            vals["out"][u] = -1, -1, 0
            continue
        pr = c["pairs"][m]
        vals[u] = (True, pr[2 if r["second"] else 0], pr[3 if r["second"] else 1], r["prob"], r["mu"], r["var"],
                   (m, r["box"], r["votes"]))
    tabs = [[a.copy() for a in sc] for sc in start]
    block_out = np.full((len(c["blocks"]), 3), SENT, np.int32)
    v = vals[inv.reshape(-1)]
    block_out[:nb] = v["out"]
    sp = c["block_spp"][:nb][v["ok"]]
    for arr, name in zip(tabs[0], ("sem", "ins", "prob", "mu", "var")):
        arr[sp] = v[name][v["ok"]]
    return tabs, block_out
