"""A NumPy restatement of the reference's voxelisation source (ISBNet isbnet/ops/src/voxelize/voxelize.cpp:41-165 and
voxelize.cu:10-62; SPFormer's pointgroup_ops copy is the same): plain loops, a dict in insertion order, a float32 cast
on every operation.  It restates the source; it is not a run of it.  The wrong conventions the tests
discriminate against are the keyword arguments.
"""
import numpy as np

FLAG_BATCH, FLAG_DUPLICATE = 1, 2                    # GAPRO_VOXELIZE_FLAG_*
POOL_COUNT, POOL_INDEX, POOL_TWICE = 1, 2, 4         # GAPRO_VOXEL_POOL_FLAG_*
MAX_ACTIVE = 4096                                    # GAPRO_VOXELIZE_MAX_ACTIVE
BAD_ARG = -1


class Refused(Exception):
    """What the header arithmetic refuses (a ValueError of the public call)."""


def table_width(mode, n_voxels, max_active):
    rows = mode in (3, 4)
    if rows and max_active > MAX_ACTIVE:
        raise Refused("max_active")
    width = max_active + 1 if rows else 2
    if n_voxels * width > 2 ** 31 - 1:
        raise Refused("table")
    return width


def voxelize_idx_ref(coords, mode=4, *, sorted_numbering=False, unordered_rows=False, swap_first_last=False):
    """(output_coords, input_map, output_map, flags) by voxelize.cpp:69-165: the points in order, a voxel numbered when
    its key is first met (:88-92, :108-112), rows in the order of the points (:93, :113)."""
    coords = np.asarray(coords, dtype=np.int64)
    n, cols = coords.shape
    if n == 0:
        return np.zeros((0, cols), np.int64), np.zeros(0, np.int32), np.zeros((0, 2), np.int32), 0
    if cols == 4 and (coords[:, 0] < 0).any():
        return None, None, None, FLAG_BATCH  # SGs[batchIdx] out of range in the reference (:107)
    seen = {}  # key -> voxel, in insertion order
    rows = []
    input_map = np.zeros(n, np.int32)
    for i in range(n):
        key = tuple(int(x) for x in coords[i])
        if key not in seen:
            seen[key] = len(rows)
            rows.append([])
        rows[seen[key]].append(i)
        input_map[i] = seen[key]
    if sorted_numbering:  # the wrong convention: torch.unique's order
        order = sorted(range(len(rows)), key=lambda v: tuple(int(x) for x in coords[rows[v][0]]))
        new = np.empty(len(rows), np.int64)
        new[order] = np.arange(len(rows))
        rows = [rows[v] for v in order]
        input_map = new[input_map].astype(np.int32)
    if unordered_rows:  # the wrong convention: rows as some schedule's atomics left them
        rows = [r[::-1] for r in rows]
    M = len(rows)
    max_active = max(len(r) for r in rows)
    if mode == 0 and max_active > 1:
        return None, None, None, FLAG_DUPLICATE  # the assert of :135
    width = table_width(mode, M, max_active)
    output_map = np.zeros((M, width), np.int32)
    for v, r in enumerate(rows):
        if mode in (0, 1):
            output_map[v] = (1, r[-1] if swap_first_last else r[0])  # :142 front
        elif mode == 2:
            output_map[v] = (1, r[0] if swap_first_last else r[-1])  # :148 back
        else:
            output_map[v, 0] = len(r)
            output_map[v, 1:1 + len(r)] = r
    output_coords = np.stack([coords[(sorted(r) if unordered_rows else r)[0]] for r in rows])  # :47, rule[1]
    return output_coords, input_map, output_map, 0


def pool_flags(map_rule, n_points):
    """The status flags of the pooling calls for a table: a count outside [0, A], an index outside [0, n_points), a
    point listed twice."""
    flags, seen = 0, set()
    A = map_rule.shape[1] - 1
    for r in map_rule:
        n = int(r[0])
        if n < 0 or n > A:
            flags |= POOL_COUNT
            continue
        for p in r[1:1 + n]:
            if p < 0 or p >= n_points:
                flags |= POOL_INDEX
            elif int(p) in seen:
                flags |= POOL_TWICE
            else:
                seen.add(int(p))
    return flags


def _mult(n, mode):
    return np.float32(1.0) / np.float32(n) if (mode == 4 and n > 0) else np.float32(1.0)


def pool_forward_ref(feats, map_rule, mode=4, *, convention="unfused"):
    """voxelize.cu:10-25: per row and channel, from a zeroed float32, ``out += mult * x`` in the row's order, the product
    and the sum each rounded to float32.  ``convention``: "fused" rounds ``mult * x + out`` once, "divide" sums and then
    divides -- the two wrong ones.  A flagged row is zeros and a flagged entry is skipped (this project's rule)."""
    feats = np.asarray(feats, np.float32)
    N, C = feats.shape
    M, A = map_rule.shape[0], map_rule.shape[1] - 1
    out = np.zeros((M, C), np.float32)
    for v in range(M):
        n = int(map_rule[v, 0])
        if n < 0 or n > A:
            continue
        mult = _mult(n, mode)
        for c in range(C):
            acc = np.float32(0.0)
            for k in range(1, n + 1):
                p = int(map_rule[v, k])
                if p < 0 or p >= N:
                    continue
                x = feats[p, c]
                if convention == "unfused":
                    acc = np.float32(acc + np.float32(mult * x))
                elif convention == "fused":
                    acc = np.float32(np.float64(mult) * np.float64(x) + np.float64(acc))  # exact product, one rounding
                else:
                    acc = np.float32(acc + x)
            if convention == "divide" and mode == 4 and n > 0:
                acc = np.float32(acc / np.float32(n))
            out[v, c] = acc
    return out


def pool_backward_ref(d_out, map_rule, n_points, mode=4):
    """voxelize.cu:39-54 for a table that lists a point at most once: ``d_feats[p] = mult * d_out[v]``, zeros elsewhere.
    A flagged row gives nothing and a flagged entry is skipped."""
    d_out = np.asarray(d_out, np.float32)
    M, C = d_out.shape
    A = map_rule.shape[1] - 1
    d_feats = np.zeros((n_points, C), np.float32)
    for v in range(M):
        n = int(map_rule[v, 0])
        if n < 0 or n > A:
            continue
        mult = _mult(n, mode)
        for k in range(1, n + 1):
            p = int(map_rule[v, k])
            if 0 <= p < n_points:
                d_feats[p] = (mult * d_out[v]).astype(np.float32)
    return d_feats
