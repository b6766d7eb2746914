"""NumPy float64 restatement of the matcher's cost (ISBNet/isbnet/model/matcher.py:156-197) as gapro_match_cost defines
it (include/gapro_hip.h, "Cost matrices"): every term in float64 from the float32 inputs, one rounding to float32, then
NaN / +-inf -> 100000.  Also a brute-force assignment for small problems, the fixtures' loader and the comparison the
tests share.  Nothing here is used by the product.
"""
import itertools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ["two", "wide", "sixty_four"]
WEIGHTS = (0.5, 1.0, 1.0, 0.2, 0.2)  # class, dice, bce, conf, giou (matcher.py:192)
DUP_GT = 4                           # the fixtures' aux assignment
BIG = np.float32(100000.0)


def giou_cross(b1, b2):
    """model_utils.py:385-413 in float64: [N, 6] x [M, 6] -> [N, M].  minimum / maximum / clip hand a NaN on, as torch's."""
    b1 = np.asarray(b1, dtype=np.float64)[:, None, :]
    b2 = np.asarray(b2, dtype=np.float64)[None, :, :]
    with np.errstate(all="ignore"):
        inter = np.prod(np.clip(np.minimum(b1[..., 3:], b2[..., 3:]) - np.maximum(b1[..., :3], b2[..., :3]), 0.0, None), -1)
        v1 = np.prod(np.clip(b1[..., 3:] - b1[..., :3], 0.0, None), -1)
        v2 = np.prod(np.clip(b2[..., 3:] - b2[..., :3], 0.0, None), -1)
        union = v1 + v2 - inter
        bound = np.prod(np.clip(np.maximum(b1[..., 3:], b2[..., 3:]) - np.minimum(b1[..., :3], b2[..., :3]), 0.0, None), -1)
        return inter / (union + 1e-6) - (bound - union) / (bound + 1e-6)


def cost64(cls_logits, mask_logits, conf_logits, box_preds, mask, cls, box, weights=WEIGHTS):
    """One sample: cls_logits [Q, C], mask_logits [Q, S], conf_logits [Q], box_preds [Q, 6]; mask [I, S], cls [I],
    box [I, 6].  The cost in float64, before the rounding."""
    x = np.asarray(mask_logits, dtype=np.float64)
    t = np.asarray(mask, dtype=np.float64)
    z = np.asarray(cls_logits, dtype=np.float64)
    w_class, w_dice, w_bce, w_conf, w_giou = (float(v) for v in weights)
    with np.errstate(all="ignore"):
        e = np.exp(-np.abs(x))
        sig = np.where(x >= 0.0, 1.0, e) / (1.0 + e)
        sp = np.maximum(x, 0.0) + np.log1p(e)
        dot_sig, dot_x = sig @ t.T, x @ t.T
        lost = ~np.isfinite(x).all(axis=1)  # a NaN or infinite logit takes its whole row, whatever the product skips
        dot_sig[lost] = np.nan
        dot_x[lost] = np.nan
        dice = 1.0 - (2.0 * dot_sig + 1.0) / (sig.sum(1)[:, None] + t.sum(1)[None, :] + 1.0)
        bce = (sp.sum(1)[:, None] - dot_x) / x.shape[1]
        p = np.exp(z - z.max(axis=1, keepdims=True))
        p = p / p.sum(axis=1, keepdims=True)
        cls_cost = -p[:, np.asarray(cls, dtype=np.int64)]
        conf = -np.asarray(conf_logits, dtype=np.float64)[:, None]
        giou = -giou_cross(box_preds, box)
        return w_class * cls_cost + w_dice * dice + w_bce * bce + w_conf * conf + w_giou * giou


def cost(*args, **kw):
    """cost64 rounded to float32 once, then the 100000 rule of matcher.py:196-197."""
    with np.errstate(all="ignore"):
        out = cost64(*args, **kw).astype(np.float32)
    out[~np.isfinite(out)] = BIG
    return out


def ulp32(a):
    """The spacing of float32 at |a| (at least the smallest normal's)."""
    return np.spacing(np.maximum(np.abs(np.asarray(a, dtype=np.float32)), np.float32(1.1754944e-38))).astype(np.float64)


def close(got, want):
    """Device against the restatement: 1 float32 ulp of the value plus 1e-9.  The float64 sums of the two differ by their
    order alone, ~4096 2^-52 100 = 9e-11 at S <= 4096 and |x| <= 100, so the rounded results differ only where a value
    sits on a float32 rounding boundary."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    bound = ulp32(want) + 1e-9
    assert (err <= bound).all(), "max error %.3g at a bound of %.3g" % (err.max(), bound[np.unravel_index(err.argmax(), err.shape)])
    return True


def pairs(rows, cols, n_inst):
    """An assignment as the tests compare it: sorted (row, original column) pairs."""
    return sorted(zip(np.asarray(rows).tolist(), (np.asarray(cols) % n_inst).tolist()))


def brute_force(cost_matrix, dup=1):
    """The optimal total of the rectangular assignment on np.tile(cost, (1, dup)) by enumeration (small problems): every
    injective map of the smaller side into the larger one."""
    c = np.tile(np.asarray(cost_matrix, dtype=np.float64), (1, dup))
    if c.shape[0] > c.shape[1]:
        c = c.T
    n, m = c.shape
    assert n <= 6 and m <= 12
    c = c.tolist()
    return min(sum(c[i][j] for i, j in enumerate(perm)) for perm in itertools.permutations(range(m), n))


def total(cost_matrix, rows, cols):
    return float(np.asarray(cost_matrix, dtype=np.float64)[np.asarray(rows), np.asarray(cols)].sum())


def check_assignment(cost_matrix, rows, cols, dup=1):
    """rows ascending and distinct, every original column used at most dup times, as many pairs as the smaller side."""
    n_rows, n_cols = np.asarray(cost_matrix).shape
    rows, cols = np.asarray(rows), np.asarray(cols)
    assert rows.dtype == np.int64 and cols.dtype == np.int64 and len(rows) == len(cols) == min(n_rows, dup * n_cols)
    assert (np.diff(rows) > 0).all() and (rows >= 0).all() and (rows < n_rows).all()
    assert (cols >= 0).all() and (cols < n_cols).all() and np.bincount(cols, minlength=n_cols).max() <= dup
    return True


def fixture(name):
    """A fixture of tests/golden/make_golden_match.py: the npz and its samples as dicts (None: no instance)."""
    z = np.load(os.path.join(GOLDEN, "match_%s.npz" % name))
    samples = []
    for b in range(int(z["batch_size"])):
        if bool(z["is_none"][b]):
            samples.append(None)
            continue
        samples.append({k: z["%s_%d" % (k, b)] for k in ("mask_logits", "mask", "cls", "box", "ref_cost", "row", "col",
                                                         "aux_row", "aux_col")})
    return z, samples
