"""Inputs of the heuristic-labeler and getInstanceInfo edge tests (test_labeler_edges_cpu.py / test_labeler_edges_gpu.py),
and a plain reference of the labelers to tie them to.

``Literal`` is a deliberately literal per-point, per-superpoint Python loop for gen_pseudo_label ("volume", "dist",
"none") and gen_pseudo_label_box2mask, written from the reference's lines gen_ps_utils.py:242-290, 485-569 and 99-123; it
shares no code with oracle/labeler_oracle.py.  Its three choices: the float32 margin ``box -+ 0.005f`` is widened to
float64 before the compare; float32 centres are ``(lo + hi) / 2``; the squared distance is the sum of three separately
rounded float64 squares in x, y, z order.  For "dist" it reads the coordinates of scene point k for the k-th multi-box
point (the reference's indexing, :525-526) or, on request, the point's own: test_labeler_edges_cpu.py uses the switch to
show that a case can tell the two apart.

Every case is a named entry of LABELER_CASES / INSTANCE_CASES; test_labeler_edges_cpu.py proves on the CPU that each is
what its builder's comment claims, so that nothing in the GPU file passes vacuously.

Superpoint ids: the labelers rank them with the partition's table, which holds a range of max(4 n, 2^20) ids; ids that are
negative AND ids above 2^31 therefore cannot meet in one scene, and the occupancy-mask case comes in two variants.
"""
from collections import OrderedDict, namedtuple
from fractions import Fraction
from functools import lru_cache

import numpy as np

import partition_cases as pc

LABELERS = ("volume", "dist", "none", "box2mask")
DATASETS = ("scannetv2", "other")  # superpoint alignment on / off
F32 = np.float32
MARGIN = F32(0.005)

# structural constants of gapro_amd/csrc/labels.hip that the cases are built around
LAB_CHUNK = 2048            # points per workgroup of the "dist" rank scan
LAB_MAX_BOXES = 256
LAB_GRID_POINTS = 2048 * 256   # k_lab_points / k_lab_tally / k_lab_final wrap above this many points
CORNER_GRID_POINTS = 1024 * 256  # k_inst_corners wraps above this many
INST_LDS_IDS = 512          # k_inst_minmax: ids below go through the LDS table
INST_FIRST_CAP = 1024       # getInstanceInfo_device's first table

LabCase = namedtuple("LabCase", "name coords spp cls box vol labelers meta")


def _case(name, coords, spp, cls, box, vol=None, labelers=LABELERS, **meta):
    box = np.ascontiguousarray(np.asarray(box, F32).reshape(-1, 6))
    if vol is None:
        vol = np.prod(box[:, 3:] - box[:, :3], axis=1).astype(F32)
    arrays = (np.ascontiguousarray(coords, np.float64), np.ascontiguousarray(spp, np.int64),
              np.ascontiguousarray(cls, np.int64), box, np.ascontiguousarray(vol, F32))
    for a in arrays:
        a.setflags(write=False)
    return LabCase(name, *arrays, tuple(labelers), meta)


def args_of(case):
    """Positional arguments of gen_pseudo_label / gen_pseudo_label_box2mask (the library's and the oracle's)."""
    return case.coords, case.spp, case.cls, case.box, case.vol


# ------------------------------------------------------------------------------------------ the literal reference
def sqdist_reference(p, c):
    """torch.sum((p - c) ** 2, -1) in float64: every square rounded, then summed in x, y, z order."""
    dx, dy, dz = p[0] - c[0], p[1] - c[1], p[2] - c[2]
    sx, sy, sz = dx * dx, dy * dy, dz * dz
    return (sx + sy) + sz


def _rn(q):
    """A rational rounded to the nearest float64 (int / int true division is correctly rounded)."""
    return float(Fraction(q))


def sqdist_fused(p, c, order):
    """The squared distance as a compiler may contract it: one rounded product, then two fused multiply-adds, each
    rounded once (exact rational arithmetic in between).  order = the axes from the innermost product outwards, e.g.
    (0, 1, 2) = fma(dz, dz, fma(dy, dy, RN(dx dx)))."""
    d = [Fraction(p[k] - c[k]) for k in range(3)]  # the subtraction is a rounded operation of its own
    acc = Fraction(_rn(d[order[0]] * d[order[0]]))
    for k in order[1:]:
        acc = Fraction(_rn(d[k] * d[k] + acc))
    return float(acc)


class Literal:
    """The four labelers of one case, point by point.  Labels: box index, -1 = no box, -2 = rule "none" on a multi-box
    point."""

    def __init__(self, case, instance_classes=18):
        self.case = case
        self.instance_classes = instance_classes
        box = case.box
        self.n, self.n_boxes = len(case.coords), len(box)
        # :502-504 / :248-250: float32 box -+ 0.005 in float32, compared with float64 coordinates in float64
        self.lo = [[float(box[b, k] - MARGIN) for k in range(3)] for b in range(self.n_boxes)]
        self.hi = [[float(box[b, 3 + k] + MARGIN) for k in range(3)] for b in range(self.n_boxes)]
        self.centre = [[float((box[b, k] + box[b, 3 + k]) / F32(2.0)) for k in range(3)] for b in range(self.n_boxes)]
        self.vol = [float(v) for v in case.vol]  # float32 values, compared exactly
        self.points = case.coords.tolist()
        self.spp = case.spp.tolist()
        lo, hi = self.lo, self.hi
        self.inside = []  # per point the boxes that hold it, ascending
        for x, y, z in self.points:
            self.inside.append([b for b in range(self.n_boxes)
                                if lo[b][0] <= x <= hi[b][0] and lo[b][1] <= y <= hi[b][1] and lo[b][2] <= z <= hi[b][2]])
        self.multi = [i for i in range(self.n) if len(self.inside[i]) > 1]
        self._mask = self._members = None

    # ---- the rule for every point
    def raw(self, labeler, own_coords=False):
        rule = "volume" if labeler == "box2mask" else labeler
        out = [-100] * self.n
        rank = 0  # among the multi-box points
        for i, boxes in enumerate(self.inside):
            if not boxes:
                out[i] = -1
            elif len(boxes) == 1:
                out[i] = boxes[0]
            else:
                if rule == "none":
                    out[i] = -2
                elif rule == "volume":
                    best = boxes[0]
                    for b in boxes[1:]:
                        if self.vol[b] < self.vol[best]:  # scatter_min: the first minimum wins
                            best = b
                    out[i] = best
                elif rule == "dist":
                    p = self.points[i if own_coords else rank]  # :526 indexes the scene by the rank
                    best, best_d = boxes[0], sqdist_reference(p, self.centre[boxes[0]])
                    for b in boxes[1:]:
                        d = sqdist_reference(p, self.centre[b])
                        if d < best_d:
                            best, best_d = b, d
                    out[i] = best
                else:
                    raise ValueError(rule)
                rank += 1
        return out

    # ---- the superpoint vote
    def members(self):
        if self._members is None:
            self._members = OrderedDict()
            for i, s in enumerate(self.spp):
                self._members.setdefault(s, []).append(i)
        return self._members

    def label_counts(self, raw):
        """{superpoint id: [count of class 0 = no box, count of box 0, ...]} (:552, :104-111)."""
        out = {}
        for s, idx in self.members().items():
            c = [0] * (self.n_boxes + 1)
            for i in idx:
                c[raw[i] + 1 if raw[i] >= 0 else 0] += 1
            out[s] = c
        return out

    def occupancy_mask(self):
        """{superpoint id: [mean occupancy of box b >= 0.7, in float32]} (:542-546)."""
        if self._mask is None:
            self._mask = {}
            for s, idx in self.members().items():
                c = [0] * self.n_boxes
                for i in idx:
                    for b in self.inside[i]:
                        c[b] += 1
                n = F32(len(idx))
                self._mask[s] = [bool(F32(k) / n >= F32(0.7)) for k in c]
        return self._mask

    def aligned(self, raw, masked):
        counts = self.label_counts(raw)
        mask = self.occupancy_mask() if masked else None
        vote = {}
        for s, c in counts.items():
            best, best_c = 0, c[0]
            for l in range(1, self.n_boxes + 1):
                v = c[l] if (mask is None or mask[s][l - 1]) else 0  # :117
                if v > best_c:  # argmax: the first maximum wins
                    best, best_c = l, v
            vote[s] = best - 1 if best > 0 else -1  # :556
        return [vote[s] for s in self.spp]

    # ---- the whole labeler
    def labels(self, labeler, dataset_name, own_coords=False):
        lab = self.raw(labeler, own_coords)
        if dataset_name == "scannetv2":
            lab = self.aligned(lab, masked=labeler != "box2mask")
        cls = self.case.cls.astype(np.int32).tolist()  # .int() of the int64 classes (:561)
        background = self.instance_classes
        sem = [cls[v] if v >= 0 else (background if v == -1 else -100) for v in lab]
        inst = [v if v >= 0 else -100 for v in lab]
        return np.array(sem, np.int32), np.array(inst, np.int32)


@lru_cache(maxsize=None)
def literal(name):
    return Literal(labeler_case(name))


@lru_cache(maxsize=None)
def oracle_labels(name):
    """{(labeler, dataset_name): (sem, inst)} of oracle/labeler_oracle.py, computed once per case and read-only."""
    from oracle import labeler_oracle as L

    case = labeler_case(name)
    out = {}
    for labeler in case.labelers:
        for ds in DATASETS:
            if labeler == "box2mask":
                sem, inst = L.gen_pseudo_label_box2mask(*args_of(case), dataset_name=ds)
            else:
                sem, inst = L.gen_pseudo_label(*args_of(case), dataset_name=ds, heuristic_rule=labeler)
            sem.setflags(write=False)
            inst.setflags(write=False)
            out[labeler, ds] = (sem, inst)
    return out


# ------------------------------------------------------------------------------------------ many boxes
MANY_BOXES = (63, 64, 65, 128, 129, 255, 256)
# seeds at which the smallest box of many points is box 64 (65 boxes) and "none" still labels some points (65, 129)
MANY_BOX_SEEDS = {65: 11065, 129: 10129}


def _many_boxes(n_boxes):
    """Cell-aligned boxes of a 4 x 4 x 2 grid scene: a handful of distinct float32 volumes among them, so the "first
    minimum wins" rule decides most multi-box points; from 65 boxes on labels beyond the first occupancy word."""
    kw = pc.grid_scene(MANY_BOX_SEEDS.get(n_boxes, 9000 + n_boxes), 3000, n_boxes, 6, 0.5, "shuffled")
    return _case("boxes_%d" % n_boxes, kw["coords_float"], kw["spp"], kw["instance_cls"], kw["instance_box"],
                 kw["instance_box_volume"], n_boxes=n_boxes)


# ------------------------------------------------------------------------------------------ the rank scan of "dist"
RANK_FORCED = (0, 63, 64, 255, 256, 2047, 2048, 2049, 4095, 4096)
RANK_N = 2 * LAB_CHUNK + 300
# box 1 (A) and box 3 (B) overlap in x in [1, 2] with centres at x = 1 and x = 2; box 2 lies inside the overlap (a third
# bit on some points); boxes 0 and 4 are apart
RANK_BOXES = ((5, 0, 0, 6, 1, 1), (0, 0, 0, 2, 1, 1), (1.25, 0, 0, 1.75, 1, 0.5), (1, 0, 0, 3, 1, 1), (8, 0, 0, 9, 1, 1))


def _rank_scan(name, n, single_head=0, seed=0):
    """Whether a point is multi-box is chosen per index: RANK_FORCED and n - 1 are, the rest at random (about half);
    the first single_head points are single-box, so that no rank equals its index.  A multi-box point lies in the
    overlap of A and B, whichever centre is nearer to it; the others in A only, B only, box 0 or in no box, so the point
    whose coordinates the k-th multi-box point is measured from may decide differently."""
    rng = np.random.default_rng(400 + seed + n)
    multi = rng.random(n) < 0.5
    for i in RANK_FORCED + (n - 1,):
        if i < n:
            multi[i] = True
    multi[:single_head] = False
    coords = rng.uniform([0.0, 0.05, 0.05], [1.0, 0.95, 0.95], size=(n, 3))
    where = rng.integers(0, 4, size=n)
    x0 = np.array([0.05, 2.05, 5.05, 6.5])[where]  # A only, B only, box 0, nowhere
    coords[:, 0] = np.where(multi, 1.05 + 0.9 * coords[:, 0], x0 + 0.9 * coords[:, 0])
    spp = rng.integers(0, max(n // 12, 1), size=n) * 7 - 50
    forced = tuple(sorted(set(i for i in RANK_FORCED + (n - 1,) if single_head <= i < n)))
    return _case(name, coords, spp, [3, 0, 17, 5, 9], RANK_BOXES, forced=forced, multi=multi, single_head=single_head)


# ------------------------------------------------------------------------------------------ mirrored centres
MIRROR_POINTS = 200
MIRROR_AXES = ((0, 1), (1, 2), (0, 2))  # pairs mirrored about x = y, y = z, x = z


def _mirrored():
    """Three pairs of boxes, each pair mirrored about a coordinate plane through the origin (corners are multiples of
    1/8: exact in float32, and so are the centres), and per pair MIRROR_POINTS points ON the mirror plane inside both
    boxes of the pair and no other: the two squared distances are the same three squares in another order.  About x = y
    the reference's (x^2 + y^2) + z^2 commutes; about y = z and x = z it does only when the third square adds exactly, so
    those points stand at the centres' third coordinate (that square is 0).  The distances are then equal in the
    reference's arithmetic and the first box wins, while a contracted evaluation rounds the two squares at different
    places.  The points stand at the start of the array (rank k = index k: each is
    measured from its own coordinates); single-box and no-box filler follows."""
    rng = np.random.default_rng(77)
    boxes, coords, pair_of_point = [], [], []
    base = np.array([1.0, 1.5, 0.0, 2.75, 3.25, 1.0])  # the pair's first box in (u, v, w) = (mirrored axes, the third)
    for pair, (u, v) in enumerate(MIRROR_AXES):
        w = 3 - u - v
        shift = 16.0 * pair  # pairs far apart, along the mirror plane
        first, second = np.zeros(6), np.zeros(6)
        for half in (0, 3):
            first[half + u], first[half + v], first[half + w] = base[half] + shift, base[half + 1] + shift, base[half + 2]
            second[half + u], second[half + v], second[half + w] = base[half + 1] + shift, base[half] + shift, base[half + 2]
        boxes += [first, second]
        t = rng.uniform(1.5 + shift, 2.75 + shift, size=MIRROR_POINTS)
        p = np.zeros((MIRROR_POINTS, 3))
        p[:, u], p[:, v], p[:, w] = t, t, (rng.uniform(0.0, 1.0, size=MIRROR_POINTS) if pair == 0 else 0.5)
        coords.append(p)
        pair_of_point += [pair] * MIRROR_POINTS
    boxes = np.array(boxes)
    assert np.array_equal(boxes.astype(F32).astype(np.float64), boxes)
    filler = []
    for b in boxes:  # 40 points in the part of each box that its mirror image does not cover
        f = rng.uniform(b[:3] + 0.01, b[3:] - 0.01, size=(400, 3))
        other = boxes[[j for j in range(6) if not np.array_equal(boxes[j], b)]]
        alone = ~np.any(np.all((f[:, None, :] >= other[None, :, :3] - 0.01) & (f[:, None, :] <= other[None, :, 3:] + 0.01),
                               axis=2), axis=1)
        filler.append(f[alone][:40])
    filler.append(rng.uniform([100, 100, 100], [101, 101, 101], size=(30, 3)))
    coords = np.concatenate(coords + filler)
    spp = np.arange(len(coords)) // 4 + (1 << 31) + 11
    return _case("mirrored_centres", coords, spp, [1, 2, 3, 4, 5, 6], boxes, pair_of_point=np.array(pair_of_point))


# ------------------------------------------------------------------------------------------ the occupancy mask
MASK_SPPS = ((10, 6), (10, 7), (10, 8), (100, 69), (100, 70), (1, 1), (1, 0))  # (points, inside box A)
MASK_IDS = {"neg": (-900001, -65537, -17, -3, 0, 5, 40000), "big": tuple((1 << 31) + v for v in (1, 2, 700, 701, 4096,
                                                                                                 65536, 1000000))}


def _mask(variant):
    """Hand-built superpoints of 10 points with 6, 7 and 8 inside box A (box 2 of 3) and the rest in no box, of 100 with 69
    and 70 inside, and two of a single point: the float32 occupancy is below, exactly at and above 0.7.  Shuffled."""
    rng = np.random.default_rng(len(variant))
    ids = MASK_IDS[variant]
    coords, spp = [], []
    for sid, (n, k) in zip(ids, MASK_SPPS):
        coords += [rng.uniform([0.1, 0.1, 0.1], [0.9, 0.9, 0.9], size=(k, 3)),
                   rng.uniform([3.1, 0.1, 0.1], [3.9, 0.9, 0.9], size=(n - k, 3))]
        spp += [sid] * n
    coords, spp = np.concatenate(coords), np.array(spp, np.int64)
    perm = rng.permutation(len(spp))
    box = [[10, 0, 0, 11, 1, 1], [20, 0, 0, 21, 1, 1], [0, 0, 0, 1, 1, 1]]
    return _case("mask_%s_ids" % variant, coords[perm], spp[perm], [4, 5, 6], box, ids=ids)


# ------------------------------------------------------------------------------------------ vote ties
TIE_BOXES = 72
TIE_A, TIE_B = 5, 6  # overlapping, equal volumes


def _vote_ties():
    """72 unit boxes in a row (box j at x = 10 j), box 6 = box 5 moved by 0.5.  Superpoint 100: the first 10 points of the
    scene, inside both box 5 and box 6 (both occupancies 1.0), 5 nearer each centre -- under "dist" with the mask the
    vote is 5 : 5 and the lower box wins.  Superpoint 200: 5 points in no box and 5 in box 9 -- "no box" wins.
    Superpoint 300: 5 points only in box 3 and 5 only in box 70 -- box 3 wins.  Superpoint 400: the same vote with box 70
    first in the array."""
    rng = np.random.default_rng(12)
    box = np.zeros((TIE_BOXES, 6))
    box[:, 0], box[:, 3:] = 10.0 * np.arange(TIE_BOXES), 1.0
    box[:, 3] += box[:, 0]
    box[TIE_B, 0], box[TIE_B, 3] = box[TIE_A, 0] + 0.5, box[TIE_A, 3] + 0.5

    def inside(b, n, x_lo=0.05, x_hi=0.95):
        p = rng.uniform([x_lo, 0.05, 0.05], [x_hi, 0.95, 0.95], size=(n, 3))
        p[:, 0] += box[b, 0]
        return p

    near_a, near_b = inside(TIE_A, 5, 0.55, 0.7), inside(TIE_A, 5, 0.8, 0.95)  # centres at x = 50.5 and 51
    head = np.empty((10, 3))
    head[0::2], head[1::2] = near_b, near_a
    nobox = inside(9, 5, 2.0, 3.0)
    parts = [(head, 100), (nobox, 200), (inside(9, 5), 200), (inside(3, 5), 300), (inside(70, 5), 300),
             (inside(70, 5), 400), (inside(3, 5), 400), (inside(20, 7), 500), (inside(TIE_B, 3, 0.55, 0.95), 500)]
    coords = np.concatenate([p for p, _ in parts])
    spp = np.concatenate([np.full(len(p), s) for p, s in parts])
    return _case("vote_ties", coords, spp, np.arange(TIE_BOXES) % 18, box,
                 ties={"dist": {100: (TIE_A, TIE_B, TIE_A)}, "box2mask": {200: (-1, 9, -1), 300: (3, 70, 3),
                                                                           400: (3, 70, 3)}})


# ------------------------------------------------------------------------------------------ faces
FACE_BOX = 2
FACE_CLS = (3, 17, -100, 2 ** 31 - 1, 7, 0)


def _faces():
    """Box 2 (corners that are not exact in float32) probed on its six faces, the other two coordinates at its centre:
    the float64 value of the float32 sum box -+ 0.005f (inside), one np.nextafter beyond it (outside), and box -+ 0.005
    computed in float64 (whichever side of the float32 face it falls on).  Box 0 has lo > hi on the y axis and holds
    nothing, although a point stands in its middle; box 1 has zero volume (a plate at z = 0.5 inside box 4: points on it
    are in both, "volume" takes the plate); box 3 is ordinary.  The classes are 0, 17, -100 and 2^31 - 1."""
    rng = np.random.default_rng(2)
    box = np.zeros((6, 6), F32)
    box[0] = [30, 1.5, 0, 31, 0.5, 1]
    box[1] = [40.25, 0.25, 0.5, 40.75, 0.75, 0.5]
    box[FACE_BOX] = np.array([1.1, 2.3, 0.7, 2.2, 3.1, 1.9], F32) + rng.uniform(0, 0.01, 6).astype(F32)
    box[3] = [50, 0, 0, 51, 1, 1]
    box[4] = [40, 0, 0, 41, 1, 1]
    box[5] = [60, 0, 0, 61, 1, 1]
    c32 = box[FACE_BOX]
    c = c32.astype(np.float64)
    centre = 0.5 * (c[:3] + c[3:])
    pts, kind = [], []
    for axis in range(3):
        for side in (0, 1):
            face32 = np.float64(c32[axis] - MARGIN) if side == 0 else np.float64(c32[3 + axis] + MARGIN)
            face64 = c[axis] - 0.005 if side == 0 else c[3 + axis] + 0.005
            outward = -np.inf if side == 0 else np.inf
            for v, k in ((face32, "on"), (np.nextafter(face32, outward), "beyond"), (face64, "f64")):
                p = centre.copy()
                p[axis] = v
                pts.append(p)
                kind.append(k)
    n_probe = len(pts)
    pts.append([30.5, 1.0, 0.5])  # the middle of the inverted box
    plate = rng.uniform([40.3, 0.3, 0.5], [40.7, 0.7, 0.5], size=(6, 3))
    plate[3:, 2] = [0.504, 0.496, 0.506]  # inside the plate's margin twice, beyond it once
    rest = np.concatenate([rng.uniform([50.1, 0.1, 0.1], [50.9, 0.9, 0.9], size=(3, 3)),
                           rng.uniform([60.1, 0.1, 0.1], [60.9, 0.9, 0.9], size=(3, 3)),
                           rng.uniform([40.1, 0.1, 0.8], [40.9, 0.9, 0.9], size=(3, 3))])
    coords = np.concatenate([np.array(pts), plate, rest])
    spp = np.arange(len(coords)) // 2 - 6
    return _case("faces", coords, spp, FACE_CLS, box, kind=tuple(kind), n_probe=n_probe, inverted_point=n_probe,
                 plate_points=tuple(range(n_probe + 1, n_probe + 7)))


# ------------------------------------------------------------------------------------------ grid-stride loops
def _grid_stride():
    """More points than one sweep of the point kernels' grids (2048 x 256 + 300): three overlapping boxes, 2048 grid-cell
    superpoints, and 257 chunks for the rank scan of "dist"."""
    rng = np.random.default_rng(3)
    n = LAB_GRID_POINTS + 300
    coords = rng.uniform(0.0, 1.0, size=(n, 3)) * np.array([4.0, 4.0, 2.0])
    ijk = np.minimum((coords / 0.25).astype(np.int64), [15, 15, 7])
    spp = (ijk[:, 0] * 16 + ijk[:, 1]) * 8 + ijk[:, 2]
    box = [[0, 0, 0, 2.5, 3.5, 2], [1.5, 0.5, 0, 4, 4, 2], [1, 1, 0.5, 3, 3, 1.5]]
    return _case("grid_stride", coords, spp, [2, 11, 6], box, labelers=("volume", "dist"))


LABELER_CASES = OrderedDict()
for _b in MANY_BOXES:
    LABELER_CASES["boxes_%d" % _b] = (_many_boxes, (_b,))
LABELER_CASES["rank_scan"] = (_rank_scan, ("rank_scan", RANK_N))
LABELER_CASES["rank_scan_single_head"] = (_rank_scan, ("rank_scan_single_head", RANK_N, 300, 1))
for _n in (1, 63, 257):
    LABELER_CASES["rank_scan_n%d" % _n] = (_rank_scan, ("rank_scan_n%d" % _n, _n))
LABELER_CASES["mirrored_centres"] = (_mirrored, ())
LABELER_CASES["mask_neg_ids"] = (_mask, ("neg",))
LABELER_CASES["mask_big_ids"] = (_mask, ("big",))
LABELER_CASES["vote_ties"] = (_vote_ties, ())
LABELER_CASES["faces"] = (_faces, ())
LABELER_CASES["grid_stride"] = (_grid_stride, ())
LABELER_CASE_NAMES = tuple(LABELER_CASES)


@lru_cache(maxsize=None)
def labeler_case(name):
    fn, args = LABELER_CASES[name]
    case = fn(*args)
    assert case.name == name
    return case


# ------------------------------------------------------------------------------------------ getInstanceInfo
InstCase = namedtuple("InstCase", "name xyz inst sem")
ID_EDGES = (0, 1, 510, 511, 512, 513, 1022, 1023)


def _inst_case(name, xyz, inst, sem):
    arrays = (np.ascontiguousarray(xyz, np.float64), np.ascontiguousarray(inst, np.float64),
              np.ascontiguousarray(sem, np.float64))
    for a in arrays:
        a.setflags(write=False)
    return InstCase(name, *arrays)


def _shuffled_ids(name, ids, n, seed):
    """n points shuffled over the ids (every id at least once), semantic labels among -100 and a few classes."""
    rng = np.random.default_rng(seed)
    ids = np.asarray(ids, np.float64)
    inst = np.concatenate([ids, rng.choice(ids, size=n - len(ids))])
    rng.shuffle(inst)
    return _inst_case(name, rng.uniform(-5, 5, size=(n, 3)), inst, rng.choice([-100.0, 2.0, 5.0, 19.0, 3.0], size=n))


def _singletons():
    rng = np.random.default_rng(21)
    inst = np.concatenate([np.full(2000, 0.0), [1.0], np.full(1500, 2.0), [7.0], [600.0], np.full(500, 601.0), [-100.0] * 50])
    rng.shuffle(inst)
    return _inst_case("singletons", rng.normal(0, 3, size=(len(inst), 3)), inst, rng.integers(2, 20, size=len(inst)))


def _signs():
    """Instance 0 all negative, 1 mixed, 2 with -0.0, +0.0 and other values on every axis, 3 with nothing but the two
    zeros (its extent is 0; which zero is the minimum is not compared: the zeros are equal)."""
    rng = np.random.default_rng(22)
    a = -rng.uniform(0.5, 9, size=(300, 3))
    b = rng.uniform(-4, 4, size=(300, 3))
    c = rng.choice([-0.0, 0.0, -1.5, 2.5, -1e-3], size=(300, 3))
    d = rng.choice([-0.0, 0.0], size=(40, 3))
    xyz = np.concatenate([a, b, c, d])
    inst = np.concatenate([np.full(300, 0.0), np.full(300, 1.0), np.full(300, 2.0), np.full(40, 3.0)])
    perm = rng.permutation(len(inst))
    return _inst_case("signs", xyz[perm], inst[perm], rng.integers(2, 20, size=len(inst)))


def _magnitudes():
    """Subnormals and magnitudes from 1e-300 to 1e100, either sign, finite values only.  Instance 0 mixes them all;
    instances 1 .. 4 hold one band each (subnormal float64, float32-subnormal range, 1e-300 .. 1e-200, 1e90 .. 1e100)."""
    rng = np.random.default_rng(23)

    def band(n, lo_exp, hi_exp):
        return rng.choice([-1.0, 1.0], size=(n, 3)) * 10.0 ** rng.uniform(lo_exp, hi_exp, size=(n, 3))

    sub = rng.integers(1, 1 << 40, size=(60, 3)).astype(np.float64) * 5e-324 * rng.choice([-1.0, 1.0], size=(60, 3))
    bands = [np.concatenate([sub[:20], band(20, -300, -200), band(20, -45, -37), band(20, -3, 3), band(20, 90, 100),
                             [[5e-324, -5e-324, 2.2250738585072014e-308]]]),
             sub[20:], band(50, -45, -37), band(50, -300, -200), band(50, 90, 100)]
    xyz = np.concatenate(bands)
    inst = np.concatenate([np.full(len(b), float(i)) for i, b in enumerate(bands)])
    perm = rng.permutation(len(inst))
    return _inst_case("magnitudes", xyz[perm], inst[perm], rng.integers(2, 20, size=len(inst)))


def _class_shift():
    """The first point of instance 0 and of instance 5 carries the semantic label -100 (kept as is under the ScanNet
    shift); instance 2's first point carries 2 (shifted to 0) and a later one -100."""
    rng = np.random.default_rng(24)
    inst = np.array([0.0, 2.0, 5.0, 2.0, 0.0, -100.0, 5.0, 9.0] + list(rng.choice([0.0, 2.0, 5.0, 9.0], size=200)))
    sem = np.array([-100.0, 2.0, -100.0, -100.0, 7.0, 3.0, 4.0, 1.0] + list(rng.choice([-100.0, 2.0, 19.0], size=200)))
    return _inst_case("class_shift", rng.uniform(-2, 2, size=(len(inst), 3)), inst, sem)


def _corner_grid_stride():
    return _shuffled_ids("corner_grid_stride", list(range(30)) + [-100.0], CORNER_GRID_POINTS + 77, 25)


INSTANCE_CASES = OrderedDict([
    ("id_edges", (_shuffled_ids, ("id_edges", ID_EDGES + (-100, -1), 6000, 26))),
    ("id_edges_regrow", (_shuffled_ids, ("id_edges_regrow", ID_EDGES + (-100, -1, 1024, 1025, 3001), 6000, 27))),
    ("dense_1101", (_shuffled_ids, ("dense_1101", tuple(range(1101)), 3500, 28))),
    ("singletons", (_singletons, ())),
    ("signs", (_signs, ())),
    ("magnitudes", (_magnitudes, ())),
    ("class_shift", (_class_shift, ())),
    ("corner_grid_stride", (_corner_grid_stride, ())),
])
INSTANCE_CASE_NAMES = tuple(INSTANCE_CASES)


@lru_cache(maxsize=None)
def instance_case(name):
    fn, args = INSTANCE_CASES[name]
    case = fn(*args)
    assert case.name == name
    return case


@lru_cache(maxsize=None)
def oracle_instance_info(name, scannet):
    """oracle.eval_oracle.get_instance_info of a case, computed once and read-only."""
    from oracle.eval_oracle import get_instance_info

    case = instance_case(name)
    with np.errstate(over="ignore", under="ignore"):  # float64 -> float32 corners of the magnitudes case
        out = get_instance_info(case.xyz, case.inst, case.sem, scannet=scannet)
    for a in out[1:]:
        a.setflags(write=False)
    return out
