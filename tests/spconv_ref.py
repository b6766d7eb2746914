"""NumPy restatement of the sparse convolutions (include/gapro_hip.h, "Sparse convolutions"): a
dictionary rulebook, float64 einsums for the three forwards and the hand-derived backwards.  Every sum also returns,
per output element, T (the number of its terms) and A (the same sum over |x| and |w|): a float64 accumulation of T
terms is within T 2^-52 A of the exact sum, which is what the device tests allow on top of the float32 rounding.

``wrong=`` switches on ONE wrong convention (tests/test_spconv_cpu.py shows that each is caught):
    "convolution"   the kernel flipped (a convolution instead of a cross-correlation)
    "xz"            the offsets applied as (x, y, z)
    "weight_layout" the weight's memory read as [k, k, k, C_in, C_out]
    "keep_odd"      the last slice of an odd extent kept by the strided layer
    "no_batch"      the batch column ignored
    "sorted"        coarse rows numbered in sorted rather than first-child order
"""
import numpy as np

OFFSETS = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]  # k = (dz+1) 9 + (dy+1) 3 + dx+1


def out_shape(shape):
    return tuple((d - 2) // 2 + 1 if d >= 2 else 0 for d in shape)


def subm_table(coords, shape, wrong=None):
    """neighbours int32[27, V]: the row at p + d_k in the same sample and inside the grid, or -1."""
    coords = np.asarray(coords, dtype=np.int64)
    key = (lambda b, p: tuple(p)) if wrong == "no_batch" else (lambda b, p: (b,) + tuple(p))
    rows = {key(int(r[0]), [int(v) for v in r[1:]]): i for i, r in enumerate(coords)}
    nbr = np.full((27, len(coords)), -1, dtype=np.int32)
    for k, d in enumerate(OFFSETS):
        if wrong == "xz":
            d = d[::-1]
        if wrong == "convolution":
            d = tuple(-v for v in d)
        for i, r in enumerate(coords):
            p = [int(r[1 + a]) + d[a] for a in range(3)]
            if all(0 <= p[a] < shape[a] for a in range(3)):
                nbr[k, i] = rows.get(key(int(r[0]), p), -1)
    return nbr


def down_tables(coords, shape, wrong=None):
    """(coarse_coords int32[V_c, 4], children int32[8, V_c], parent int32[V], child_slot int32[V]) of the strided
    layer: coarse rows numbered by their first child in ascending input row."""
    coords = np.asarray(coords, dtype=np.int64)
    Do = out_shape(shape)
    number, coarse, parent = {}, [], np.full(len(coords), -1, dtype=np.int32)
    slot = ((coords[:, 1] & 1) * 4 + (coords[:, 2] & 1) * 2 + (coords[:, 3] & 1)).astype(np.int32)
    for i, r in enumerate(coords):
        q = (0 if wrong == "no_batch" else int(r[0]),) + tuple(int(v) >> 1 for v in r[1:])
        if wrong != "keep_odd" and any(q[1 + a] >= Do[a] for a in range(3)):
            continue
        if q not in number:
            number[q] = len(coarse)
            coarse.append(q)
        parent[i] = number[q]
    coarse = np.array(coarse, dtype=np.int32).reshape(-1, 4)
    if wrong == "sorted" and len(coarse):
        order = np.lexsort(coarse.T[::-1])
        rank = np.empty(len(coarse), dtype=np.int32)
        rank[order] = np.arange(len(coarse), dtype=np.int32)
        coarse, parent = coarse[order], np.where(parent >= 0, rank[np.maximum(parent, 0)], -1).astype(np.int32)
    children = np.full((8, len(coarse)), -1, dtype=np.int32)
    for i in range(len(coords)):
        if parent[i] >= 0:
            children[slot[i], parent[i]] = i
    return coarse, children, parent, slot


def one_of_table(index, k_of, K=8):
    """The dense [K, R] form of a "one of K" table."""
    tab = np.full((K, len(index)), -1, dtype=np.int32)
    ok = np.asarray(index) >= 0
    tab[np.asarray(k_of)[ok], np.nonzero(ok)[0]] = np.asarray(index)[ok]
    return tab


def weights_by_offset(w, wrong=None):
    """f64[K, C_out, C_in] of a weight [C_out, kz, ky, kx, C_in]."""
    w = np.asarray(w, dtype=np.float64)
    Co, Ci = w.shape[0], w.shape[-1]
    if wrong == "weight_layout":
        return np.ascontiguousarray(w).reshape(-1, Ci, Co).transpose(0, 2, 1)
    return w.reshape(Co, -1, Ci).transpose(1, 0, 2)


def forward(tab, x, w, bias=None, wrong=None):
    """y[r] = bias + sum_k W_k x[tab[k, r]]; returns (y, T, A), each f64[R_out, C_out]."""
    W = weights_by_offset(w, wrong)
    x = np.asarray(x, dtype=np.float64)
    R, Co, Ci = tab.shape[1], W.shape[1], W.shape[2]
    y, T, A = np.zeros((R, Co)), np.zeros((R, Co)), np.zeros((R, Co))
    for k in range(tab.shape[0]):
        ok = tab[k] >= 0
        if ok.any():
            y[ok] += x[tab[k][ok]] @ W[k].T
            A[ok] += np.abs(x[tab[k][ok]]) @ np.abs(W[k]).T
            T[ok] += Ci
    if bias is not None:
        b = np.asarray(bias, dtype=np.float64)
        y, A, T = y + b, A + np.abs(b), T + 1
    return y, T, A


def backward_input(tab, n_in, g, w):
    """dx[j] = sum over the pairs (k, r) with tab[k, r] = j of W_k^T g[r]; (dx, T, A), each f64[n_in, C_in]."""
    W = weights_by_offset(w)
    g = np.asarray(g, dtype=np.float64)
    Co, Ci = W.shape[1], W.shape[2]
    dx, T, A = np.zeros((n_in, Ci)), np.zeros((n_in, Ci)), np.zeros((n_in, Ci))
    for k in range(tab.shape[0]):
        ok = tab[k] >= 0
        if ok.any():  # an input row is the pair of at most one output row per offset
            dx[tab[k][ok]] += g[ok] @ W[k]
            A[tab[k][ok]] += np.abs(g[ok]) @ np.abs(W[k])
            T[tab[k][ok]] += Co
    return dx, T, A


def backward_weight(tab, x, g, w_shape):
    """dW[:, k, :] = sum_r g[r] (x) x[tab[k, r]] in the weight's own shape, dbias = sum_r g[r]; each with T and A."""
    x, g = np.asarray(x, dtype=np.float64), np.asarray(g, dtype=np.float64)
    K, Co, Ci = tab.shape[0], g.shape[1], x.shape[1]
    dW, T, A = np.zeros((Co, K, Ci)), np.zeros((Co, K, Ci)), np.zeros((Co, K, Ci))
    for k in range(K):
        ok = tab[k] >= 0
        if ok.any():
            dW[:, k, :] = g[ok].T @ x[tab[k][ok]]
            A[:, k, :] = np.abs(g[ok]).T @ np.abs(x[tab[k][ok]])
            T[:, k, :] = ok.sum()
    db = (g.sum(0), np.full(Co, float(len(g))), np.abs(g).sum(0))
    return (dW.reshape(w_shape), T.reshape(w_shape), A.reshape(w_shape)), db


def tolerance(ref, T, A):
    """ulp32(ref) + T 2^-52 A: the float32 rounding of the result and the float64 accumulation of T terms."""
    ulp = np.spacing(np.abs(np.asarray(ref)).astype(np.float32)).astype(np.float64)
    return ulp + np.asarray(T) * 2.0 ** -52 * np.asarray(A)


def layer_tables(layer, coords, shape, wrong=None):
    """(forward table [K, rows_out], rows_in) of "subm", "down" or "inverse" on ``coords``."""
    if layer == "subm":
        return subm_table(coords, shape, wrong), len(coords)
    coarse, children, parent, slot = down_tables(coords, shape, wrong)
    if layer == "down":
        return children, len(coords)
    return one_of_table(parent, slot), len(coarse)
