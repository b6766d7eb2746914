"""A NumPy restatement of the superpoint pooling definition (include/gapro_hip.h "Superpoint pooling"):
plain loops in point order, a float32 value after every operation, no ``np.add.at`` and no sorting helper for the sums.
The loops run over the points; the channels of a point are one float32 vector, whose operations NumPy rounds element by
element.  ``convention=`` restates the conventions the definition rules out, for the tests that tell them apart."""
import numpy as np

F32 = np.float32
FLAG_INDEX, FLAG_MAP, BAD_ARG = 1, 2, -1  # GAPRO_SPP_FLAG_*, GAPRO_ERR_BAD_ARG


def flags_of(index, S, point_map=None, R=None):
    index = np.asarray(index).astype(np.int64)
    flags = FLAG_INDEX if ((index < 0) | (index >= S)).any() else 0
    if point_map is not None:
        m = np.asarray(point_map).astype(np.int64)
        flags |= FLAG_MAP if ((m < 0) | (m >= R)).any() else 0
    return flags


def _listed(index, S, point_map, R):
    """Per point: is it in a segment (its index, and its map value if there is a map, are in range)."""
    index = np.asarray(index).astype(np.int64)
    ok = (index >= 0) & (index < S)
    if point_map is not None:
        m = np.asarray(point_map).astype(np.int64)
        ok &= (m >= 0) & (m < R)
    return ok


def _groups(keys, n_keys, ok):
    """The points of every key in ascending point order, by one pass over the points."""
    groups = [[] for _ in range(n_keys)]
    for p in range(len(keys)):
        if ok[p]:
            groups[int(keys[p])].append(p)
    return groups


def plan_ref(index, S, point_map=None, R=None, batch_offsets=None):
    """What gapro_spp_plan_build writes: a dict of seg_off, seg_pts, counts, and with a map row_off, row_pts, seg_rows,
    with batch_offsets spp_batch_offsets; and the flags."""
    index = np.asarray(index).astype(np.int64)
    N = len(index)
    ok = _listed(index, S, point_map, R)
    left_out = [p for p in range(N) if not ok[p]]

    def csr(groups):
        off = np.zeros(len(groups) + 1, dtype=np.int32)
        pts = []
        for k, g in enumerate(groups):
            pts += g
            off[k + 1] = len(pts)
        return off, np.array(pts + left_out, dtype=np.int32).reshape(N)

    segs = _groups(index, S, ok)
    out = {"flags": flags_of(index, S, point_map, R)}
    out["seg_off"], out["seg_pts"] = csr(segs)
    out["counts"] = np.array([len(g) for g in segs], dtype=np.int32)
    if point_map is not None:
        m = np.asarray(point_map).astype(np.int64)
        out["row_off"], out["row_pts"] = csr(_groups(m, R, ok))
        listed = int(out["seg_off"][-1])
        rows = np.full(N, -1, dtype=np.int32)
        rows[:listed] = m[out["seg_pts"][:listed]]
        out["seg_rows"] = rows
    if batch_offsets is not None:
        bo = np.asarray(batch_offsets).astype(np.int64)
        per = np.zeros(len(bo) - 1, dtype=np.int64)
        for g in segs:
            if g:
                for b in range(len(bo) - 1):
                    if bo[b] <= g[0] < bo[b + 1]:
                        per[b] += 1
        out["spp_batch_offsets"] = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
    return out


def unique_loop(index, batch_offsets):
    """ISBNet's spp_pool loop (isbnet.py:736-742)."""
    out = [0]
    for b in range(len(batch_offsets) - 1):
        out.append(out[-1] + len(np.unique(np.asarray(index)[batch_offsets[b]:batch_offsets[b + 1]])))
    return np.array(out, dtype=np.int64)


def _rows2(a):
    a = np.asarray(a, dtype=F32)
    return a.reshape(a.shape[0], -1)


def _tree(vals):
    vals = list(vals)
    while len(vals) > 1:
        vals = [(vals[i] + vals[i + 1]).astype(F32) if i + 1 < len(vals) else vals[i] for i in range(0, len(vals), 2)]
    return vals[0]


def pool_forward_ref(src, index, S, reduce="mean", point_map=None, convention=None):
    """``(out f32[S, C], arg i64[S, C])`` (``arg`` None for the mean); a 1-D ``src`` gives 1-D results.
    ``convention``: None (the definition), and the wrong ones -- ``"reversed"`` (descending points), ``"tree"`` (a
    pairwise tree), ``"reciprocal"`` (``sum * (1 / n)``), ``"last_tie"`` (``>=``), ``"nan"`` (a NaN wins)."""
    x = _rows2(src)
    R, C = x.shape
    N = len(index)
    m = np.arange(N) if point_map is None else np.asarray(point_map).astype(np.int64)
    segs = _groups(np.asarray(index).astype(np.int64), S, _listed(index, S, point_map, R))
    out = np.zeros((S, C), dtype=F32)
    arg = np.full((S, C), N, dtype=np.int64) if reduce == "max" else None
    for s, pts in enumerate(segs):
        if not pts:
            continue
        if convention == "reversed":
            pts = pts[::-1]
        if reduce == "mean":
            if convention == "tree":
                acc = _tree([x[m[p]] for p in pts])
            else:
                acc = np.zeros(C, dtype=F32)
                for p in pts:
                    acc = (acc + x[m[p]]).astype(F32)
            n = F32(len(pts))
            out[s] = (acc * (F32(1) / n).astype(F32)).astype(F32) if convention == "reciprocal" else (acc / n).astype(F32)
        else:
            best, a = x[m[pts[0]]].copy(), np.full(C, pts[0], dtype=np.int64)
            for p in pts[1:]:
                v = x[m[p]]
                with np.errstate(invalid="ignore"):
                    take = v >= best if convention == "last_tie" else v > best
                if convention == "nan":
                    take = take | (np.isnan(v) & ~np.isnan(best))
                best, a = np.where(take, v, best).astype(F32), np.where(take, p, a)
            out[s], arg[s] = best, a
    if np.asarray(src).ndim == 1:
        out, arg = out[:, 0], (arg[:, 0] if arg is not None else None)
    return out, arg


def pool_backward_ref(g, index, S, reduce="mean", arg=None, point_map=None, R=None, convention=None):
    """``d_src`` (``[N, C]``, or ``[R, C]`` through a map) of the upstream ``g`` ``[S, C]``.  ``convention="by_segment"``
    is the wrong order of a mapped backward: a row's points added segment by segment (the order in which a sum per
    segment followed by a scatter would arrive) and not in ascending point order."""
    g2 = _rows2(g)
    C = g2.shape[1]
    index = np.asarray(index).astype(np.int64)
    N = len(index)
    ok = _listed(index, S, point_map, R)
    counts = [len(v) for v in _groups(index, S, ok)]
    a2 = None if arg is None else np.asarray(arg).reshape(S, -1)
    d_point = np.zeros((N, C), dtype=F32)
    for p in range(N):
        if not ok[p]:
            continue
        s = index[p]
        if reduce == "mean":
            d_point[p] = (g2[s] / F32(counts[s])).astype(F32)
        else:
            d_point[p] = np.where(a2[s] == p, g2[s], F32(0)).astype(F32)
    if point_map is None:
        d_src = d_point
    else:
        m = np.asarray(point_map).astype(np.int64)
        d_src = np.zeros((R, C), dtype=F32)
        order = range(N)
        if convention == "by_segment":
            order = [p for pts in _groups(index, S, ok) for p in pts]
        for p in order:
            if ok[p]:
                d_src[m[p]] = (d_src[m[p]] + d_point[p]).astype(F32)
    return d_src[:, 0] if np.asarray(g).ndim == 1 else d_src


def sum_bound(x, index, S, point_map=None):
    """``2 gamma_{n-1} sum|x_i| / n`` per output: the bound between two float32 sums of the same n terms in any two
    orders (each within ``gamma_{n-1} sum|x_i|`` of the exact sum; ``gamma_k = k u / (1 - k u)``, ``u = 2^-24``), carried
    through the division, plus one rounding of each quotient."""
    x = _rows2(x).astype(np.float64)
    N = len(index)
    m = np.arange(N) if point_map is None else np.asarray(point_map).astype(np.int64)
    u = 2.0 ** -24
    mass = np.zeros((S, x.shape[1]))
    cnt = np.zeros(S)
    for p in range(N):
        mass[index[p]] += np.abs(x[m[p]])
        cnt[index[p]] += 1
    k = np.maximum(cnt - 1, 0)
    gamma = k * u / (1 - k * u)
    n = np.maximum(cnt, 1)[:, None]
    return 2 * gamma[:, None] * mass / n + 2 * u * mass / n * (1 + gamma[:, None])
