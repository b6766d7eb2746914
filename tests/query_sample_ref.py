"""NumPy restatement of the query sampling (include/gapro_hip.h, "Query sampling"), written from the
definitions there: float32 with every operation cast, ``np.argmax`` for the tie rule (the lowest index of equal maxima).
It restates the SOURCE of the reference's CUDA kernels (isbnet/ops/src/sampling, isbnet/ops/src/ballquery,
isbnet/pointnet2/_ext_src/src/sampling_gpu.cu and ball_query_gpu.cu); it is not a run of them.

Two deliberately wrong variants show that the test cases discriminate:
``tournament(block)``  the reference's tie order: a strided per-thread scan and a shared-memory tournament whose
                       winner among equal distances depends on the block size its launcher picks;
``sqdist_fused``       the squared distance as a contracting compiler evaluates it, fma(dz, dz, fma(dy, dy, dx * dx)),
                       emulated with a float64 product-sum rounded to float32 once per step.
"""
import numpy as np

F = np.float32
FAR = F(1e10)
ORIGIN_BALL = F(1e-3)
FLAG_OFFSETS, FLAG_EMPTY, FLAG_NOT_FINITE = 1, 2, 4
OK, ERR_BAD_ARG, ERR_NOT_FINITE = 0, -1, -4


def status_of(flags):
    return ERR_BAD_ARG if flags & (FLAG_OFFSETS | FLAG_EMPTY) else ERR_NOT_FINITE if flags & FLAG_NOT_FINITE else OK


def sqdist(dx, dy, dz):
    """((dx*dx + dy*dy) + dz*dz), every operation rounded to float32 on its own."""
    dx, dy, dz = (np.asarray(v, F) for v in (dx, dy, dz))
    with np.errstate(all="ignore"):
        xx, yy, zz = (dx * dx).astype(F), (dy * dy).astype(F), (dz * dz).astype(F)
        return ((xx + yy).astype(F) + zz).astype(F)


def sqdist_fused(dx, dy, dz):
    """The contracted form: each multiply-add rounded once."""
    dx, dy, dz = (np.asarray(v, F) for v in (dx, dy, dz))
    with np.errstate(all="ignore"):
        acc = (dx * dx).astype(F)
        acc = (dy.astype(np.float64) * dy.astype(np.float64) + acc.astype(np.float64)).astype(F)
        return (dz.astype(np.float64) * dz.astype(np.float64) + acc.astype(np.float64)).astype(F)


def lowest_index(score):
    return int(np.argmax(score))


def tournament(block):
    """The reference's arg-max for a launch of ``block`` threads (a power of two): thread t scans t, t + block, .. with a
    strict ``>`` from (best, besti) = (-1, 0); the pairs are then folded ``dists[a] = max(v1, v2); i = v2 > v1 ? i2 :
    i1`` with strides block / 2 .. 1."""
    def pick(score):
        n = len(score)
        pad = np.full((-n) % block + n, -1.0, F)
        pad[:n] = score
        cols = pad.reshape(-1, block)
        besti = np.argmax(cols, axis=0) * block + np.arange(block)  # the first row of the column's maximum
        best = cols.max(axis=0)
        besti = np.where(best > F(-1), besti, 0)
        stride = block // 2
        while stride >= 1:
            v1, v2 = best[:stride], best[stride:2 * stride]
            besti = np.where(v2 > v1, besti[stride:2 * stride], besti[:stride])
            best = np.maximum(v1, v2)
            stride //= 2
        return int(besti[0])
    return pick


def _range(table, b, total):
    lo, hi = (int(table[b - 1]) if b > 0 else 0), int(table[b])
    return lo, hi, 0 <= lo <= hi <= total


def fps_ref(xyz, offset, new_offset, skip_origin=False, local_index=False, dist=sqdist, pick=lowest_index):
    """``(idx int32[m], minima float32[n], flags)``; entries the device does not write are -2 / NaN here."""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    n_total, m_total = len(xyz), max(int(new_offset[-1]), 0) if len(new_offset) else 0
    idx = np.full(m_total, -2, np.int32)
    minima = np.full(n_total, np.nan, F)
    flags = 0
    for b in range(len(offset)):
        n0, n1, ok_n = _range(offset, b, n_total)
        m0, m1, ok_m = _range(new_offset, b, m_total)
        if not (ok_n and ok_m):
            flags |= FLAG_OFFSETS
            continue
        n, m = n1 - n0, m1 - m0
        if m == 0:
            continue
        if n == 0:
            idx[m0:m1] = -1
            flags |= FLAG_EMPTY
            continue
        p = xyz[n0:n1]
        if not np.isfinite(p).all():
            flags |= FLAG_NOT_FINITE
        cand = np.ones(n, bool)
        if skip_origin:
            cand = ~(sqdist(p[:, 0], p[:, 1], p[:, 2]) <= ORIGIN_BALL)
        d = np.full(n, FAR, F)
        base = 0 if local_index else n0
        old = 0
        idx[m0] = base
        for s in range(1, m):
            with np.errstate(all="ignore"):
                d2 = dist((p[:, 0] - p[old, 0]).astype(F), (p[:, 1] - p[old, 1]).astype(F),
                          (p[:, 2] - p[old, 2]).astype(F))
                upd = cand & (d2 < d)  # a NaN leaves the minimum
            d[upd] = d2[upd]
            old = pick(np.where(cand, d, F(-1)))
            idx[m0 + s] = base + old
        minima[n0:n1] = d
    return idx, minima, flags


def ball_ref(radius, nsample, xyz, new_xyz, offset, new_offset, local_index=False):
    """``(idx int32[m, nsample], counts int32[m], flags)``."""
    xyz, new_xyz = np.asarray(xyz, F).reshape(-1, 3), np.asarray(new_xyz, F).reshape(-1, 3)
    n_total, m_total = len(xyz), len(new_xyz)
    r2 = F(F(radius) * F(radius))
    idx = np.zeros((m_total, nsample), np.int32)
    counts = np.zeros(m_total, np.int32)
    flags = 0
    for b in range(len(offset)):
        if not (_range(offset, b, n_total)[2] and _range(new_offset, b, m_total)[2]):
            flags |= FLAG_OFFSETS
    for q in range(m_total):
        b = 0
        while b < len(new_offset) and q >= int(new_offset[b]):
            b += 1
        if b == len(new_offset) or not _range(offset, b, n_total)[2]:
            flags |= FLAG_OFFSETS
            continue
        n0, n1, _ = _range(offset, b, n_total)
        p = xyz[n0:n1]
        with np.errstate(all="ignore"):
            d2 = sqdist((new_xyz[q, 0] - p[:, 0]).astype(F), (new_xyz[q, 1] - p[:, 1]).astype(F),
                        (new_xyz[q, 2] - p[:, 2]).astype(F))
            hits = np.nonzero(d2 < r2)[0][:nsample]
        if len(hits):
            base = 0 if local_index else n0
            idx[q, :] = base + hits[0]
            idx[q, :len(hits)] = base + hits
            counts[q] = len(hits)
    return idx, counts, flags
