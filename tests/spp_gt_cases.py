"""Edge cases of the per-sample ground-truth masks (gapro_amd/csrc/spp_gt.hip), shared by the CPU and the GPU test.

A case is a name, a builder of its inputs and the condition it is there for; the condition is asserted wherever the
case is used, so a case that no longer meets it fails on the CPU as well.  What a case must give -- results or a
refusal -- comes from the restatement tests/spp_gt_ref.py, never from the device.
"""
from collections import namedtuple

import numpy as np

from gapro_amd import _lib

import spp_gt_ref as ref

THREADS = 256
WAVE = 64
GRID_CAP = _lib.SPP_GT_GRID_CAP  # workgroups of a pass over the points

Case = namedtuple("Case", ["name", "build", "holds"])
# spps is None in subsample mode, idxs is None in superpoint mode
Inputs = namedtuple("Inputs", ["labels", "spps", "idxs", "cls", "box", "offsets", "batch_size", "ignore", "n_spps"])


def _tables(rng, n_cls, negative=()):
    cls = rng.integers(0, 18, n_cls).astype(np.int64)
    for i in negative:
        cls[i] = -100
    box = rng.uniform(-8, 8, (n_cls, 6)).astype(np.float32)
    box[0, 0] = -0.0  # bit copies: the sign of a zero and a NaN's payload survive
    box[-1, 5] = np.float32(np.nan)
    return cls, box


def sample(rng, n, inst_ids, spp_ids, p_ignore=0.2, ignore=-100):
    """n points in runs of one superpoint each (every id of spp_ids owns a run), most of a run in one instance."""
    spp_ids, inst_ids = np.asarray(spp_ids), np.asarray(inst_ids)
    k = len(spp_ids)
    assert n >= k
    cuts = np.sort(rng.permutation(np.arange(1, n))[:k - 1])
    run = np.repeat(np.arange(k), np.diff(np.r_[0, cuts, n]))
    spp = spp_ids[rng.permutation(k)][run]
    if len(inst_ids) == 0:
        return np.full(n, ignore, dtype=np.int64), spp.astype(np.int64)
    owner = inst_ids[np.r_[np.arange(len(inst_ids)), rng.integers(0, len(inst_ids), k)][:k] % len(inst_ids)]
    lab = owner[run]
    noise = rng.random(n) < 0.15
    lab[noise] = inst_ids[rng.integers(0, len(inst_ids), int(noise.sum()))]
    lab[rng.random(n) < p_ignore] = ignore
    own = rng.permutation(n)[:len(inst_ids)]  # every instance id owns a point
    lab[own] = inst_ids[:len(own)]
    return lab.astype(np.int64), spp.astype(np.int64)


def batch(seed, parts, n_cls, n_spps, negative=(), ignore=-100, lead=0, trail=0):
    """parts: per sample (n, inst_ids, spp_ids), n == 0 for a sample without points; `lead` / `trail` points before the
    first and after the last offset carry labels and superpoint ids no sample could (they must not be read)."""
    rng = np.random.default_rng(seed)
    labels, spps, off = [np.full(lead, 10 ** 7, dtype=np.int64)], [np.full(lead, -5, dtype=np.int64)], [lead]
    for n, inst_ids, spp_ids in parts:
        if n:
            lab, spp = sample(rng, n, inst_ids, spp_ids, ignore=ignore)
            labels.append(lab)
            spps.append(spp)
        off.append(off[-1] + n)
    labels.append(np.full(trail, -7, dtype=np.int64))
    spps.append(np.full(trail, n_spps + 3, dtype=np.int64))
    cls, box = _tables(rng, n_cls, negative)
    return Inputs(np.concatenate(labels), np.concatenate(spps), None, cls, box, np.asarray(off, dtype=np.int64),
                  len(parts), ignore, n_spps)


def explicit(rows, cls, n_spps=None, offsets=None, ignore=-100):
    """rows: (superpoint id, [labels of its points]) in point order."""
    labels = np.concatenate([np.asarray(r[1], dtype=np.int64) for r in rows])
    spps = np.concatenate([np.full(len(r[1]), r[0], dtype=np.int64) for r in rows])
    cls = np.asarray(cls, dtype=np.int64)
    box = np.arange(6 * len(cls), dtype=np.float32).reshape(-1, 6)
    off = np.asarray([0, len(labels)] if offsets is None else offsets, dtype=np.int64)
    return Inputs(labels, spps, None, cls, box, off, len(off) - 1, ignore,
                  int(spps.max()) + 1 if n_spps is None else n_spps)


def expected(d, strict=False):
    """The restatement's result, or the Refused it raises (as a value)."""
    try:
        if d.spps is None:
            return ref.get_subsample_gt(d.labels, d.idxs, d.cls, d.box, d.offsets, d.batch_size, d.ignore)
        return ref.get_spp_gt(d.labels, d.spps, d.cls, d.box, d.offsets, d.batch_size, d.ignore, strict, d.n_spps)
    except ref.Refused as e:
        return e


def _ids_of(d, b):
    lab = d.labels[d.offsets[b]:d.offsets[b + 1]]
    return set(np.unique(lab[lab != d.ignore]).tolist())


def _spps_of(d, b):
    return set(np.unique(d.spps[d.offsets[b]:d.offsets[b + 1]]).tolist())


def _nones(d, strict=False):
    return [e is None for e in expected(d, strict)]


# ---- bit-word edges ------------------------------------------------------------------------------------------------
EDGE_IDS = [0, 31, 32, 33, 63, 64, 65]
OFF_EDGE_IDS = [1, 30, 34, 62]


def _bit_words():
    return batch(1, [(400, EDGE_IDS, EDGE_IDS), (300, OFF_EDGE_IDS, OFF_EDGE_IDS), (200, range(7, 13), range(7, 13))],
                 n_cls=66, n_spps=66)


# ---- rule edges ----------------------------------------------------------------------------------------------------
def _rule_edges():
    #          2 of 4 | 2 of 4      1 of 3, 2 of 3   half ignored   majority ignored   negative class owns one
    rows = [(0, [0, 0, 1, 1]), (1, [1, 2, 2]), (2, [2, -100]), (3, [-100, -100, 0]), (4, [3, 3, 3, 0]),
            (5, [4, 4, 4, 5, 5, 5]), (6, [1])]
    return explicit(rows, cls=[2, 5, 0, -100, 7, 9])


# ---- wave and grid edges of the tally ------------------------------------------------------------------------------
def _tally_layout(seed, pattern, total=0):
    """`pattern` (run lengths, one superpoint each) placed twice: at a wave's first lane, and so that a sample boundary
    falls in its middle, a wave's lane 32; ignored labels at a fifth of the lanes; ordinary points follow up to `total`."""
    rng = np.random.default_rng(seed)
    plen = int(np.sum(pattern))
    gap = (WAVE // 2 - plen - plen // 2) % WAVE
    tail = max(0, total - (2 * plen + gap))
    runs = list(pattern) + [gap] + list(pattern) + ([tail] if tail else [])
    runs = [r for r in runs if r > 0]
    spp = np.repeat(rng.permutation(len(runs)), runs).astype(np.int64)
    n = len(spp)
    boundary = plen + gap + plen // 2
    assert boundary % WAVE == WAVE // 2
    lab = np.where(np.arange(n) < boundary, 0, 2) + (np.repeat(np.arange(len(runs)), runs) % 2)
    lab = lab.astype(np.int64)
    if tail:  # the tail is ordinary data: short runs of superpoints
        t0 = n - tail
        spp[t0:] = len(runs) + np.arange(tail) // 7
        lab[t0:] = 2 + rng.integers(0, 2, tail)
    lab[rng.random(n) < 0.2] = -100
    lab[[0, boundary]] = [0, 2]
    if tail:
        lab[-1] = 3
    cls = np.asarray([3, 4, 5, 6], dtype=np.int64)
    box = rng.uniform(-4, 4, (4, 6)).astype(np.float32)
    return Inputs(lab, spp, None, cls, box, np.asarray([0, boundary, n], dtype=np.int64), 2, -100, int(spp.max()) + 1)


def _tally_case(name, pattern, seed):
    plen = int(np.sum(pattern))

    def holds(d):
        lanes = d.labels[:plen]
        return (d.offsets[1] % WAVE == WAVE // 2 and (lanes == -100).any() and (lanes != -100).any()
                and len(np.unique(d.spps[:plen])) == len(pattern))

    return Case(name, lambda: _tally_layout(seed, pattern), holds)


def _sized(n):
    return Case("%d points" % n, lambda: _tally_layout(50 + n % 7, [64], total=n),
                lambda d: len(d.labels) == n and d.offsets[1] % WAVE == WAVE // 2 and d.labels[-1] == 3)


# ---- subsample mode ------------------------------------------------------------------------------------------------
def _subsample(permuted, past_the_end=False):
    d = batch(21, [(300, [0, 1, 2, 5], [0]), (200, [6, 7, 9], [0]), (250, [10, 11], [0])], n_cls=12, n_spps=1,
              negative=(1, 9))
    rng = np.random.default_rng(22)
    if permuted:
        idxs = np.concatenate([rng.integers(0, 300, 170), 300 + rng.integers(0, 200, 90), 500 + rng.integers(0, 250, 130)])
        off = [0, 170, 260, 390]
    else:
        idxs, off = np.arange(750), [0, 300, 500, 750]
    idxs = idxs.astype(np.int64)
    if past_the_end:
        idxs[off[1] + 5] = 750
    return d._replace(spps=None, idxs=idxs, offsets=np.asarray(off, dtype=np.int64), n_spps=0)


# ---- refusals: each on sample 1 of three ---------------------------------------------------------------------------
def _three():
    return batch(31, [(200, [0, 1, 2], range(0, 20)), (180, [3, 4, 5], range(20, 40)), (160, [6, 7], range(40, 50))],
                 n_cls=8, n_spps=50)


def _refused(kind):
    d = _three()
    labels, spps, off = d.labels.copy(), d.spps.copy(), d.offsets.copy()
    at = int(off[1]) + 11
    if kind == "negative label":
        labels[at] = -1
    elif kind == "label beyond instance_cls":
        labels[at] = 8
    elif kind == "fractional label":
        labels = labels.astype(np.float64)
        labels[at] = 3.5
    elif kind == "NaN label":
        labels = labels.astype(np.float64)
        labels[at] = np.nan
    elif kind == "negative superpoint id":
        spps[at] = -1
    elif kind == "superpoint id beyond n_spps":
        spps[at] = 50
    elif kind == "offsets that decrease":
        off[2] = off[1] - 1
    elif kind == "offsets beyond the points":
        off[3] = len(labels) + 1
    elif kind == "label and superpoint id, the label wins":
        labels[at] = 8
        spps[int(off[0]) + 3] = 50
    return d._replace(labels=labels, spps=spps, offsets=off)


REFUSALS = {  # kind -> (status, flag, sample)
    "negative label": (ref.BAD_ARG, ref.FLAG_LABEL, 1),
    "label beyond instance_cls": (ref.BAD_ARG, ref.FLAG_LABEL, 1),
    "fractional label": (ref.BAD_ARG, ref.FLAG_LABEL, 1),
    "NaN label": (ref.BAD_ARG, ref.FLAG_LABEL, 1),
    "negative superpoint id": (ref.SPP_RANGE, ref.FLAG_SPP, 1),
    "superpoint id beyond n_spps": (ref.SPP_RANGE, ref.FLAG_SPP, 1),
    "offsets that decrease": (ref.BAD_ARG, ref.FLAG_OFFSETS, 1),
    "offsets beyond the points": (ref.BAD_ARG, ref.FLAG_OFFSETS, 2),
    "label and superpoint id, the label wins": (ref.BAD_ARG, ref.FLAG_LABEL, 1),
    "subsample index one past the end": (ref.BAD_ARG, ref.FLAG_GATHER, 1),
}


def _is_refused(kind):
    def holds(d):
        e = expected(d)
        return isinstance(e, ref.Refused) and (e.code, e.flag, e.sample) == REFUSALS[kind]
    return holds


CASES = [
    Case("bit-word edges", _bit_words,
         lambda d: _ids_of(d, 0) == set(EDGE_IDS) == _spps_of(d, 0) and _ids_of(d, 1) == set(OFF_EDGE_IDS) == _spps_of(d, 1)
         and _ids_of(d, 2) == set(range(7, 13)) == _spps_of(d, 2) and len(d.cls) == 66 == d.n_spps),
    Case("rule edges", _rule_edges,
         lambda d: expected(d)[0]["mask"].tolist() == [[1, 0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0, 1],
                                                       [0, 1, 1, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1, 0],
                                                       [0, 0, 0, 0, 0, 1, 0]]
         and expected(d, True)[0]["mask"].tolist() == [[0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 1],
                                                       [0, 1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0],
                                                       [0, 0, 0, 0, 0, 0, 0]]
         and expected(d)[0]["ids"].tolist() == [0, 1, 2, 4, 5]),
    Case("batch of one", lambda: batch(2, [(300, [0, 2, 3], range(5, 25))], n_cls=4, n_spps=25),
         lambda d: d.batch_size == 1 and _nones(d) == [False]),
    Case("samples without points first, in the middle and last",
         lambda: batch(3, [(0, [], []), (200, [0, 1], range(10)), (0, [], []), (150, [2, 3], range(10, 18)), (0, [], [])],
                       n_cls=4, n_spps=18),
         lambda d: _nones(d) == [True, False, True, False, True]
         and d.offsets[0] == d.offsets[1] and d.offsets[2] == d.offsets[3] and d.offsets[4] == d.offsets[5]),
    Case("a sample with points but no kept instance",
         lambda: batch(4, [(200, [0, 1], range(10)), (150, [2], range(10, 18)), (100, [], range(18, 22)),
                           (120, [3, 4], range(22, 30))], n_cls=5, n_spps=30, negative=(2,)),
         lambda d: _nones(d) == [False, True, True, False] and _ids_of(d, 1) == {2} and d.cls[2] < 0),
    Case("every sample None",
         lambda: batch(5, [(100, [], range(5)), (0, [], []), (90, [1], range(5, 9))], n_cls=3, n_spps=9, negative=(1,)),
         lambda d: _nones(d) == [True, True, True]),
    Case("points before the first and after the last offset",
         lambda: batch(6, [(200, [0, 1, 2], range(12)), (170, [3, 4], range(12, 20))], n_cls=5, n_spps=20, lead=50,
                       trail=70),
         lambda d: d.offsets[0] == 50 and d.offsets[-1] == len(d.labels) - 70 and d.labels[0] >= len(d.cls)
         and d.spps[-1] >= d.n_spps and d.labels[-1] < 0 and d.labels[-1] != d.ignore and _nones(d) == [False, False]),
    Case("a superpoint id shared by two samples",
         lambda: batch(7, [(200, [0, 1, 2], range(0, 12)), (170, [3, 4], range(8, 20))], n_cls=5, n_spps=20),
         lambda d: _spps_of(d, 0) & _spps_of(d, 1) == {8, 9, 10, 11}),
    Case("ignore_label -1", lambda: batch(8, [(200, [0, 1, 2], range(12)), (170, [3, 4], range(12, 20))], n_cls=5,
                                          n_spps=20, ignore=-1),
         lambda d: d.ignore == -1 and (d.labels == -1).any() and not (d.labels == -100).any()),
    _tally_case("64 points in one cell", [64], 41),
    _tally_case("64 points in two cells", [32, 32], 42),
    _tally_case("64 points in 64 cells", [1] * 64, 43),
    _tally_case("runs of 63, 64 and 65 points", [63, 64, 65], 44),
    _sized(THREADS - 1), _sized(THREADS), _sized(THREADS + 1),
    Case("one point past a full grid", lambda: _tally_layout(45, [64], total=GRID_CAP * THREADS + 1),
         lambda d: len(d.labels) == GRID_CAP * THREADS + 1 and d.labels[-1] == 3),
    Case("subsample: identity", lambda: _subsample(False),
         lambda d: d.spps is None and np.array_equal(d.idxs, np.arange(len(d.labels))) and _nones(d) == [False] * 3),
    Case("subsample: permuted with repeats", lambda: _subsample(True),
         lambda d: d.spps is None and len(np.unique(d.idxs)) < len(d.idxs) and (np.diff(d.idxs) < 0).any()),
]
CASES += [Case("refused: " + k, (lambda k=k: _refused(k)), _is_refused(k)) for k in REFUSALS if "subsample" not in k]
CASES.append(Case("refused: subsample index one past the end", lambda: _subsample(True, past_the_end=True),
                  _is_refused("subsample index one past the end")))
CASE_NAMES = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
REFUSED_NAMES = [n for n in CASE_NAMES if n.startswith("refused: ")]
GOOD_NAMES = [n for n in CASE_NAMES if not n.startswith("refused: ")]


def build(name):
    c = BY_NAME[name]
    d = c.build()
    assert c.holds(d), "case %r no longer meets its condition" % name
    return d
