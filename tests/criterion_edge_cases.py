"""Inputs of the edge tests of the criterion kernels (gapro_amd/csrc/match_cost.hip, match_loss.hip, point_loss.hip;
DESIGN.md 4.7): named, seeded cases that put matched_losses, match_cost / hungarian_match and point_wise_losses on the
kinks of their expressions (ties of min / max, clamps at exactly 0, L1 differences of 0, x = 0, a sigmoid sum of exactly
0, the float32 faces of the level-set membership), on non-finite inputs, and on the second rounds of the loops over
classes, samples, rows and queries.

tests/test_criterion_edges_cpu.py asserts that every case is what its name says, holds the restatements
(tests/loss_ref.py, match_ref.py, point_loss_ref.py) to torch's float64 autograd on them and shows that each kink case
tells the right convention from the wrong one a kernel could have; tests/test_criterion_edges_gpu.py runs the cases on
the device.  NumPy only; a case is built once per process (the builders are cached): nobody may write into what they
return.
"""
import functools

import numpy as np

from gapro_amd import _lib

UP = np.array([0.7, 1.3, 0.9, 1.1, 0.6, 1.7, 2.3], dtype=np.float32)  # tests/test_losses_gpu.py's upstream weights
MAX_SAMPLES = _lib.SPP_GT_MAX_SAMPLES
PAD = np.float32(0.005)  # criterion.py:196-198
FACES = ("lo_x", "lo_y", "lo_z", "hi_x", "hi_y", "hi_z")


# ------------------------------------------------------------------------------------------------------ matched_losses
def _loss_problem(rng, Q, C, F, shapes, sigma=2.0, spread=1.5):
    """shapes: per sample (n_gt, S), "no_logits" or "no_rows" (tests/test_losses_gpu.py's generator).  Label boxes around
    the origin hold about half of the columns (all of them at ``spread`` <= 0.4); predicted faces differ from the labels'
    by 0.11 to 0.5; 0.1 <= |x| <= 5."""
    B = len(shapes)
    sizes = [s[1] if isinstance(s, tuple) else 2 for s in shapes]
    off = np.cumsum([0] + sizes)
    N = int(off[-1])
    lo = rng.uniform(-2, 0, (B, Q, 3))
    args = {"cls_logits": rng.normal(0, 2, (B, Q, C)).astype(np.float32), "mask_logits": [],
            "conf_logits": rng.normal(0, 1, (B, Q)).astype(np.float32),
            "box_preds": np.concatenate([lo, lo + rng.uniform(0.5, 3, (B, Q, 3))], 2).astype(np.float32),
            "prob_labels": rng.uniform(0.05, 1, N).astype(np.float32), "batch_offsets": off,
            "levelset_feats": rng.uniform(0, 1, (N, F)).astype(np.float32),
            "levelset_coords": rng.uniform(-spread, spread, (N, 3)).astype(np.float32)}
    gt = {k: [] for k in ("row_indices", "inst_labels", "cls_labels", "box_labels")}
    for b, (s, S) in enumerate(zip(shapes, sizes)):
        n = s[0] if isinstance(s, tuple) else 1
        x = np.clip(rng.normal(0, sigma, (Q, S)), -5, 5)
        x = np.where(np.abs(x) < 0.1, x + np.where(x < 0, -0.2, 0.2), x)
        args["mask_logits"].append(None if s == "no_logits" else x.astype(np.float32))
        glo = rng.uniform(-1.6, -0.4, (n, 3))
        rows = rng.permutation(Q)[:n].astype(np.int64)
        gt["row_indices"].append(None if s == "no_rows" else rows)
        gt["inst_labels"].append((rng.random((n, S)) < 0.4).astype(np.float32))
        gt["cls_labels"].append(rng.integers(0, C, n).astype(np.int64))
        label = np.concatenate([glo, glo + rng.uniform(1.2, 2.6, (n, 3))], 1).astype(np.float32)
        gt["box_labels"].append(label)
        pred = label + (rng.choice([-1.0, 1.0], (n, 6)) * rng.uniform(0.11, 0.5, (n, 6))).astype(np.float32)
        args["box_preds"][b, rows] = pred
    return args, gt


def _case(args, gt, **more):
    return dict(args=args, gt=gt, empty_weight=more.pop("empty_weight", None), cls_dtype=more.pop("cls_dtype", "int64"),
                **more)


KINK_ROWS = ("tie_lo_x", "tie_lo_y", "tie_lo_z", "tie_hi_x", "tie_hi_y", "tie_hi_z", "touching", "identical",
             "zero_volume", "inverted", "disjoint", "x_zero", "x_minus_1000", "x_plus_1000")


@functools.lru_cache(maxsize=None)
def kinks():
    """One sample, 16 queries, 16 columns, one kink per matched row (KINK_ROWS, in the order of gt's rows):
      tie_<face>    exactly that predicted face equals the label's in float32, the other five differ by >= 0.1
      touching      predicted lo_x == label hi_x: an intersection width of exactly 0, which clamp(min=0) passes
      identical     box_preds == box_labels: every min / max pair tied, every L1 difference 0 (the L1 gradient is exact
                    zeros; the GIoU gradient is the two 1e-6's share, about 1e-8 per face, in torch too)
      zero_volume   predicted hi_x == lo_x inside the label: the predicted and the intersection width both exactly 0
      inverted      predicted hi_x below lo_x: an active clamp
      disjoint      the prediction 10 to the side of its label
      x_zero        every logit of the row 0 (each column counts for the IoU)
      x_minus_1000  the columns inside the row's box at -1000: a sigmoid sum of exactly 0.0 under the 1e-5 clamp
      x_plus_1000   every logit of the row +1000
    ``row_of`` maps a name to its row of gt, ``query_of`` to its query."""
    rng = np.random.default_rng(4701)
    n, Q, S = len(KINK_ROWS), 16, 16
    args, gt = _loss_problem(rng, Q, 4, 2, [(n, S)])
    row_of = {name: r for r, name in enumerate(KINK_ROWS)}
    rows, label = gt["row_indices"][0], gt["box_labels"][0]
    pred = args["box_preds"][0, rows].copy()
    for k in range(6):
        pred[k, k] = label[k, k]
    r = row_of["touching"]
    pred[r, 0], pred[r, 3] = label[r, 3], label[r, 3] + np.float32(1.0)
    pred[row_of["identical"]] = label[row_of["identical"]]
    r = row_of["zero_volume"]
    pred[r, 0] = pred[r, 3] = label[r, 0] + np.float32(0.3)
    r = row_of["inverted"]
    pred[r, 3] = pred[r, 0] - np.float32(0.5)
    pred[row_of["disjoint"], [0, 3]] += np.float32(10.0)
    args["box_preds"][0, rows] = pred
    x = args["mask_logits"][0]
    x[rows[row_of["x_zero"]], :] = 0.0
    r = row_of["x_minus_1000"]
    inside = members32(args["levelset_coords"], label[r:r + 1])[0]
    x[rows[r], inside] = -1000.0
    x[rows[row_of["x_plus_1000"]], :] = 1000.0
    return _case(args, gt, row_of=row_of, query_of={name: int(rows[r]) for name, r in row_of.items()})


def members32(coords, box_label):
    """criterion.py:196-198 as the reference evaluates it, in float32: [n, S] bool; a NaN coordinate is outside."""
    c = np.asarray(coords, dtype=np.float32)[None, :, :]
    b = np.asarray(box_label, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.all(c >= (b[:, None, :3] - PAD), axis=-1) & np.all(c <= (b[:, None, 3:] + PAD), axis=-1)


def members64(coords, box_label):
    """The membership a kernel would find that compared in float64: (double)c >= (double)g - 0.005."""
    c = np.asarray(coords, dtype=np.float32).astype(np.float64)[None, :, :]
    b = np.asarray(box_label, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.all(c >= b[:, None, :3] - 0.005, axis=-1) & np.all(c <= b[:, None, 3:] + 0.005, axis=-1)


def _separating(start, upper):
    """The first float32 of start, start + 0.0073, .. whose padded face, as a float32 coordinate, lies OUTSIDE the
    float64 box: which way ``g -/+ 0.005f`` rounds depends on g's binade, so most values do not separate the two."""
    for j in range(2000):
        g = np.float32(start + 0.0073 * j)
        face = np.float32(g + PAD) if upper else np.float32(g - PAD)
        if (float(face) > float(g) + 0.005) if upper else (float(face) < float(g) - 0.005):
            return g
    raise AssertionError("no separating value from %r" % start)


FACE_COLUMNS = 18  # 6 on a face, 6 one step outside, a NaN and an infinite coordinate, 2 inside, 2 outside


@functools.lru_cache(maxsize=None)
def faces():
    """One sample, 4 queries, two matched rows; row 0's label box has, for each face k, column 2 k exactly on the padded
    float32 face and column 2 k + 1 one float32 step outside it (the other two coordinates well inside); column 12 has
    a NaN and column 13 an infinite coordinate; 14 and 15 lie well inside, 16 and 17 well outside.  The six face values
    are ones where a float64 comparison puts the on-face column outside (`_separating`)."""
    rng = np.random.default_rng(4702)
    S = FACE_COLUMNS
    args, gt = _loss_problem(rng, 4, 4, 2, [(2, S)])
    box = np.array([_separating(-0.5, False), _separating(-0.12, False), _separating(-0.1, False),
                    _separating(2.0, True), _separating(2.1, True), _separating(2.2, True)], dtype=np.float32)
    gt["box_labels"][0][0] = box
    rows = gt["row_indices"][0]
    args["box_preds"][0, rows[0]] = box + np.array([0.2, -0.3, 0.15, -0.25, 0.3, 0.12], dtype=np.float32)
    lo, hi = (box[:3] - PAD).astype(np.float32), (box[3:] + PAD).astype(np.float32)
    coords = rng.uniform(0.4, 1.6, (S, 3)).astype(np.float32)  # well inside
    for k in range(3):
        coords[2 * k, k], coords[2 * k + 1, k] = lo[k], np.nextafter(lo[k], np.float32(-np.inf))
        coords[6 + 2 * k, k], coords[7 + 2 * k, k] = hi[k], np.nextafter(hi[k], np.float32(np.inf))
    coords[12, 1], coords[13, 2] = np.nan, np.inf
    coords[16], coords[17, 0] = np.float32(7.0), np.float32(-3.0)
    args["levelset_coords"] = coords
    return _case(args, gt, on_face=[0, 2, 4, 6, 8, 10], off_face=[1, 3, 5, 7, 9, 11])


CLASS_COUNTS = (1, 64, 65, 257)


@functools.lru_cache(maxsize=None)
def classes(C):
    """Q = 3, S = 5: the matched targets are class 0 and class C - 1 (the first element of the second round at C = 65 and
    C = 257), query 1 is unmatched (target C - 1), the class weights are distinct; int32 and int64 labels alternate."""
    k = CLASS_COUNTS.index(C)
    rng = np.random.default_rng(4710 + C)
    args, gt = _loss_problem(rng, 3, C, 2, [(2, 5)])
    gt["row_indices"][0] = np.array([2, 0], dtype=np.int64)
    gt["cls_labels"][0] = np.array([0, C - 1], dtype=np.int64)
    return _case(args, gt, empty_weight=rng.permutation(np.linspace(0.2, 2.0, C)).astype(np.float32),
                 cls_dtype=("int32", "int64")[k % 2])


BATCHES = ("B5_last_kept", "B9_wave0_skipped", "Bmax_every_third_skipped")


@functools.lru_cache(maxsize=None)
def batches(name):
    """Q = 2, S in 1 .. 3 per sample; the finishing kernel's wave w takes the samples w, w + 4, ..:
      B5_last_kept              only sample 4 is kept: wave 0's second round
      B9_wave0_skipped          samples 0, 4 and 8 are skipped: all of wave 0's
      Bmax_every_third_skipped  B = SPP_GT_MAX_SAMPLES, samples 0, 3, 6, .. skipped
    A skipped sample has no logits or no rows, in turn; every column lies inside every label box."""
    B, skipped = {"B5_last_kept": (5, lambda b: b != 4), "B9_wave0_skipped": (9, lambda b: b % 4 == 0),
                  "Bmax_every_third_skipped": (MAX_SAMPLES, lambda b: b % 3 == 0)}[name]
    rng = np.random.default_rng(4720 + B)
    shapes, n_skipped = [], 0
    for b in range(B):
        shapes.append(("no_logits", "no_rows")[n_skipped % 2] if skipped(b) else (1 + b % 2, 1 + (b // 2) % 3))
        n_skipped += skipped(b)
    return _case(*_loss_problem(rng, 2, 4, 2, shapes, spread=0.4))


@functools.lru_cache(maxsize=None)
def rows():
    """Q = 130, S = 3, n_gt = 129: three rounds of the finishing kernel's lanes over the rows and over the queries."""
    return _case(*_loss_problem(np.random.default_rng(4730), 130, 4, 2, [(129, 3)]))


NAN_BACKWARD = ("zero_weight_sum", "nan_box")


@functools.lru_cache(maxsize=None)
def nan_backward(name):
    """A forward with NaN losses whose backward runs: every prob_labels 0 (the weighted BCE is 0 / 0), or a NaN in one
    matched row of box_preds (the L1 and the GIoU loss are NaN)."""
    args, gt = _loss_problem(np.random.default_rng(4740), 5, 4, 2, [(3, 16)])
    if name == "zero_weight_sum":
        args["prob_labels"][:] = 0.0
    else:
        args["box_preds"][0, gt["row_indices"][0][1], 4] = np.nan
    return _case(args, gt)


LOSS_CASES = ([("kinks", kinks, ()), ("faces", faces, ())] + [("classes-C%d" % c, classes, (c,)) for c in CLASS_COUNTS]
              + [("batches-" + n, batches, (n,)) for n in BATCHES] + [("rows", rows, ())]
              + [("nan_backward-" + n, nan_backward, (n,)) for n in NAN_BACKWARD])


# ------------------------------------------------------------------------------------------ match_cost / hungarian_match
def _match_batch(rng, Q, C, shapes):
    """shapes: per sample (I, S) or None (tests/test_match_gpu.py's generator, with the class count free)."""
    B = len(shapes)
    lo = rng.uniform(-3, 3, (B, Q, 3))
    d = {"cls_logits": rng.normal(0, 2, (B, Q, C)).astype(np.float32),
         "conf_logits": rng.normal(0, 1, (B, Q)).astype(np.float32),
         "box_preds": np.concatenate([lo, lo + rng.uniform(0.2, 3, (B, Q, 3))], 2).astype(np.float32), "samples": []}
    for s in shapes:
        if s is None:
            d["samples"].append(None)
            continue
        n_inst, S = s
        ilo = rng.uniform(-3, 3, (n_inst, 3))
        d["samples"].append({"mask_logits": rng.normal(0, 3, (Q, S)).astype(np.float32),
                             "mask": (rng.random((n_inst, S)) < 0.4).astype(np.float32),
                             "cls": rng.integers(0, C, n_inst).astype(np.int64),
                             "box": np.concatenate([ilo, ilo + rng.uniform(0.2, 3, (n_inst, 3))], 1).astype(np.float32)})
    return d


@functools.lru_cache(maxsize=None)
def match_classes(C):
    """(Q, I, S) = (17, 17, 5) at one class and at 200."""
    return _match_batch(np.random.default_rng(4750 + C), 17, C, [(17, 5)])


@functools.lru_cache(maxsize=None)
def match_class_logits():
    """Q = 8, I = 4, S = 8, C = 4, the instances' classes 0, 1, 2, 0: query 0 has -inf on class 3, which no instance has
    (its row stays finite); query 1 has -inf on class 0 (finite, a class term of exactly 0 against instances 0 and 3);
    query 2 has a +inf logit and every logit of query 3 is -inf (whole rows of 100000)."""
    d = _match_batch(np.random.default_rng(4760), 8, 4, [(4, 8)])
    d["samples"][0]["cls"] = np.array([0, 1, 2, 0], dtype=np.int64)
    z = d["cls_logits"][0]
    z[0, 3], z[1, 0], z[2, 1], z[3, :] = -np.inf, -np.inf, np.inf, -np.inf
    d["big_rows"] = [[2, 3]]
    return d


@functools.lru_cache(maxsize=None)
def match_mask_logits():
    """Q = 8, I = 4, S = 8: one +inf mask logit in query 2 and one -inf in query 5; the kernel meets both as inf * 0 (or
    inf * 1) inside the contraction x . t^T."""
    d = _match_batch(np.random.default_rng(4761), 8, 4, [(4, 8)])
    x = d["samples"][0]["mask_logits"]
    x[2, 3], x[5, 6] = np.inf, -np.inf
    d["big_rows"] = [[2, 5]]
    return d


MATCH_BOX_PAIRS = KINK_ROWS[:8] + ("disjoint",)


@functools.lru_cache(maxsize=None)
def match_boxes():
    """Q = I = 9: query k and instance k are the tie, touching, identical and disjoint pairs of `kinks`."""
    case = kinks()
    pick = [case["row_of"][name] for name in MATCH_BOX_PAIRS]
    d = _match_batch(np.random.default_rng(4762), len(pick), 4, [(len(pick), 8)])
    d["box_preds"][0] = case["args"]["box_preds"][0, case["gt"]["row_indices"][0][pick]]
    d["samples"][0]["box"] = case["gt"]["box_labels"][0][pick].copy()
    return d


MATCH_BATCHES = ("B40_every_other_none", "Bmax", "Q65_I65_S3")


@functools.lru_cache(maxsize=None)
def match_batches(name):
    """B40_every_other_none: B = 40, one instance per kept sample, every other sample None (the bisection of the checking
    kernel over samples that share a row offset, the `+ B` of the tile capacity); Bmax: B = SPP_GT_MAX_SAMPLES at Q = 17,
    I = 1, S = 1; Q65_I65_S3: five tiles each way."""
    if name == "B40_every_other_none":
        return _match_batch(np.random.default_rng(4770), 5, 4, [None if b % 2 else (1, 2 + b % 3) for b in range(40)])
    if name == "Bmax":
        return _match_batch(np.random.default_rng(4771), 17, 4, [(1, 1)] * MAX_SAMPLES)
    return _match_batch(np.random.default_rng(4772), 65, 4, [(65, 3)])


@functools.lru_cache(maxsize=None)
def match_ties():
    """Q = 4, I = 3: queries 0 and 1 are identical and so are instances 0 and 1, so rows 0 and 1 and columns 0 and 1 of
    the cost are equal bit for bit and the assignment has equal-cost optima."""
    d = _match_batch(np.random.default_rng(4780), 4, 4, [(3, 8)])
    s = d["samples"][0]
    for a in (d["cls_logits"][0], d["conf_logits"][0], d["box_preds"][0], s["mask_logits"]):
        a[1] = a[0]
    for a in (s["mask"], s["cls"], s["box"]):
        a[1] = a[0]
    return d


MATCH_CASES = ([("classes-C%d" % c, match_classes, (c,)) for c in (1, 200)]
               + [("class_logits", match_class_logits, ()), ("mask_logits", match_mask_logits, ()),
                  ("boxes", match_boxes, ())] + [("batches-" + n, match_batches, (n,)) for n in MATCH_BATCHES]
               + [("ties", match_ties, ())])


# ---------------------------------------------------------------------------------------------------- point_wise_losses
POINT_PAIRS = ("touching", "identical", "disjoint")


@functools.lru_cache(maxsize=None)
def point_pairs():
    """Eight points with an instance, four classes; points 0, 1 and 2 are the touching (predicted lo_x == label hi_x),
    identical and disjoint pairs.  Their coordinates are small dyadic numbers, so the float64 additions c + x and l + x
    are exact and the ties survive them."""
    rng = np.random.default_rng(4790)
    N, C = 8, 4
    lab = np.concatenate([-rng.uniform(0.2, 2.5, (N, 3)), rng.uniform(0.2, 2.5, (N, 3))], 1).astype(np.float32)
    pred = lab + (rng.choice([-1.0, 1.0], (N, 6)) * rng.uniform(0.11, 0.19, (N, 6))).astype(np.float32)
    pred[0, 0], pred[0, 3] = lab[0, 3], lab[0, 3] + np.float32(1.0)
    pred[1] = lab[1]
    pred[2, [0, 3]] += np.float32(10.0)
    coords = rng.uniform(-6, 6, (N, 3)).astype(np.float32)
    coords[:3] = np.array([[0.5, -1.25, 2.0], [4.0, 0.0, -8.0], [-0.75, 2.5, 1.0]], dtype=np.float32)
    return {"semantic_scores": rng.normal(0, 2, (N, C)).astype(np.float32), "corners_offset": pred,
            "box_conf": rng.uniform(0, 1, N).astype(np.float32), "semantic_labels": rng.integers(0, C, N).astype(np.int64),
            "instance_labels": rng.integers(0, 9, N).astype(np.int64), "corners_offset_labels": lab,
            "coords_float": coords}
