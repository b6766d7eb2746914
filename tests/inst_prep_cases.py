"""Edge cases of the instance-label preparation (gapro_amd/csrc/inst_prep.hip), shared by the CPU and the GPU test.

A case is a name, a builder of its inputs and the condition it is there for; the condition is asserted wherever the
case is used, so a case that no longer meets it fails on the CPU as well.  What a case must give -- results or a
refusal -- comes from the restatement tests/inst_prep_ref.py, never from the device.
"""
from collections import namedtuple

import numpy as np

from gapro_amd import _lib, consumer_ops

import inst_prep_ref as ref

THREADS = 256
GRID_CAP = _lib.INST_PREP_GRID_CAP   # workgroups of a pass over the points
LDS_IDS = _lib.INST_PREP_LDS_IDS     # new ids tallied in LDS
ID_TABLE = consumer_ops.ID_TABLE     # ids the first launch of a call has room for
MAX_IDS = _lib.INST_PREP_MAX_IDS     # an id at or beyond it is refused

Case = namedtuple("Case", ["name", "build", "holds"])
Inputs = namedtuple("Inputs", ["coords", "inst", "sem", "shift"])


def _grid_coords(rng, n, scale=8.0):
    return (rng.integers(-int(scale * 512), int(scale * 512), (n, 3)) / 512.0).astype(np.float32)


def scene(seed, n, ids, p_neg=0.2, neg=(-100,), shift=0, coords=None):
    """n points labelled with `ids` (every id owns a point where n allows it) and with `neg` at a share p_neg."""
    rng = np.random.default_rng(seed)
    ids = np.asarray(ids, dtype=np.int64)
    inst = ids[rng.integers(0, len(ids), n)] if len(ids) else np.full(n, neg[0], dtype=np.int64)
    off = rng.random(n) < p_neg
    if len(neg):
        inst[off] = np.asarray(neg, dtype=np.int64)[rng.integers(0, len(neg), int(off.sum()))]
    own = rng.permutation(n)[:len(ids)]
    inst[own] = ids[:len(own)]
    sem = rng.integers(0, 20, n).astype(np.int64)
    sem[rng.random(n) < 0.1] = -100
    xyz = _grid_coords(rng, n) if coords is None else coords(rng, n)
    return Inputs(np.ascontiguousarray(xyz, dtype=np.float32), inst, sem, shift)


def present(d):
    return np.unique(d.inst[d.inst >= 0])


def holes(d):
    p = present(d)
    return np.setdiff1d(np.arange(len(p)), p)


def _sized(n):
    ids = [0, 1, 3, 4, 9]  # holes at 2 and, where all five own a point, K - 1 = 4 is in use
    return Case("V=%d" % n, lambda: scene(100 + n, n, ids, p_neg=0.25 if n > 1 else 0.0, shift=2),
                lambda d: len(d.inst) == n and d.inst.max() >= 0)


def _past_the_grid():
    """The last point is the one the capped grid reaches only on its second sweep; it alone carries id 10."""
    d = scene(1, GRID_CAP * THREADS + 1, [0, 1, 2, 3, 8, 9], p_neg=0.2)
    inst = d.inst.copy()
    inst[-1] = 10
    return d._replace(inst=inst)


def _first_class():
    d = scene(31, 400, [0, 1, 2], p_neg=0.1)
    sem = d.sem.copy()
    sem[d.inst == 1] = 3
    sem[np.nonzero(d.inst == 1)[0][0]] = 7
    return d._replace(sem=sem)


def _ignored_class():
    d = scene(32, 400, [0, 1, 2], p_neg=0.1, shift=2)
    sem = d.sem.copy()
    sem[np.nonzero(d.inst == 0)[0][0]] = -100
    sem[np.nonzero(d.inst == 2)[0][0]] = 2
    return d._replace(sem=sem)


def _one_point():
    d = scene(33, 300, [0, 1, 2, 5], p_neg=0.1)
    inst = d.inst.copy()
    inst[inst == 5] = 1
    inst[17] = 5
    return d._replace(inst=inst)


def _signed_zeros(rng, n):
    xyz = np.where(rng.random((n, 3)) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    xyz[::3] = -0.0
    return xyz


def _signed_zero_case():
    d = scene(35, 300, [0, 1, 2, 4], p_neg=0.1, coords=_signed_zeros)
    xyz = d.coords.copy()
    xyz[d.inst == 2] = -0.0  # an instance of -0.0 alone
    xyz[d.inst == 1] = 0.0   # and one of +0.0 alone
    return d._replace(coords=xyz)


def _scales(rng, n):
    return (np.sign(rng.random((n, 3)) - 0.5) * 10.0 ** rng.uniform(-30, 30, (n, 3))).astype(np.float32)


def _non_finite(labelled):
    d = scene(38, 500, [0, 1, 2, 4], p_neg=0.3)
    xyz = d.coords.copy()
    rows = np.nonzero(d.inst >= 0 if labelled else d.inst < 0)[0]
    xyz[rows[0], 1] = np.inf
    xyz[rows[1], 2] = np.nan
    if not labelled:
        xyz[rows[2], 0] = -np.inf
    return d._replace(coords=xyz)


def _is_subnormal(x):
    x = np.abs(x)
    return (x > 0) & (x < np.finfo(np.float32).tiny)


CASES = [_sized(n) for n in (1, 63, 64, 65, 255, 256, 257)] + [
    Case("one point past a full grid", _past_the_grid,
         lambda d: len(d.inst) == GRID_CAP * THREADS + 1 and d.inst[-1] == 10 and np.sum(d.inst == 10) == 1),
    Case("single id 0", lambda: scene(2, 300, [0], p_neg=0.3),
         lambda d: list(present(d)) == [0]),
    Case("single id 7", lambda: scene(3, 300, [7], p_neg=0.3),
         lambda d: list(present(d)) == [7]),
    Case("hole at 0", lambda: scene(4, 300, [1, 2, 3], p_neg=0.2),
         lambda d: list(holes(d)) == [0]),
    Case("consecutive holes", lambda: scene(5, 400, [0, 1, 5, 6, 7, 11, 12], p_neg=0.2),
         lambda d: list(holes(d)) == [2, 3, 4]),
    Case("hole at K - 1", lambda: scene(6, 300, [0, 1, 2, 9], p_neg=0.2),
         lambda d: list(holes(d)) == [len(present(d)) - 1]),
    Case("no hole", lambda: scene(7, 300, list(range(12)), p_neg=0.2),
         lambda d: len(holes(d)) == 0 and len(present(d)) == 12),
    Case("only negative labels", lambda: scene(8, 300, [], neg=(-100, -1)),
         lambda d: d.inst.max() < 0),
    Case("-1 and -100 mixed", lambda: scene(9, 400, [0, 2, 3], p_neg=0.5, neg=(-1, -100)),
         lambda d: {-1, -100} <= set(d.inst.tolist()) and d.inst.max() == 3),
    Case("ids on both sides of the LDS table's edge",
         lambda: scene(10, 4000, [i for i in range(LDS_IDS + 18) if i not in (5, 100, 101, 102, 103)], p_neg=0.1),
         lambda d: len(present(d)) > LDS_IDS + 1 and len(holes(d)) == 5 and present(d).max() >= LDS_IDS),
    Case("largest id at the id table's last entry", lambda: scene(11, 300, [0, 1, 2, ID_TABLE - 1], p_neg=0.2),
         lambda d: d.inst.max() == ID_TABLE - 1),
    Case("ids on both sides of the id table's capacity",
         lambda: scene(12, 300, [0, 1, 2, ID_TABLE - 1, ID_TABLE, ID_TABLE + 5], p_neg=0.2),
         lambda d: {ID_TABLE - 1, ID_TABLE} <= set(d.inst.tolist())),
    Case("an id just below the refusal bound", lambda: scene(13, 200, [0, 1, MAX_IDS - 1], p_neg=0.2),
         lambda d: d.inst.max() == MAX_IDS - 1),
    Case("an id at the refusal bound", lambda: scene(14, 200, [0, 1, MAX_IDS], p_neg=0.2),
         lambda d: d.inst.max() == MAX_IDS),
    Case("first point of another class than the majority", _first_class,
         lambda d: d.sem[np.nonzero(d.inst == 1)[0][0]] == 7 and np.sum(d.sem[d.inst == 1] == 3) > 1),
    Case("class -100 with a label shift", _ignored_class,
         lambda d: d.shift == 2 and d.sem[np.nonzero(d.inst == 0)[0][0]] == -100
         and d.sem[np.nonzero(d.inst == 2)[0][0]] == 2),
    Case("an instance of one point", _one_point,
         lambda d: np.sum(d.inst == 5) == 1),
    Case("equal coordinates",
         lambda: scene(34, 300, [0, 1, 3], coords=lambda rng, n: np.tile(np.float32([1.25, -3.5, 0.1]), (n, 1))),
         lambda d: len(np.unique(d.coords, axis=0)) == 1),
    Case("signed zeros", _signed_zero_case,
         lambda d: np.all(d.coords == 0) and np.signbit(d.coords).any() and not np.signbit(d.coords).all()
         and np.signbit(d.coords[d.inst == 2]).all() and not np.signbit(d.coords[d.inst == 1]).any()),
    Case("denormals",
         lambda: scene(36, 300, [0, 1, 3],
                       coords=lambda rng, n: (rng.integers(-4000, 4000, (n, 3)) * np.float32(1e-45)).astype(np.float32)),
         lambda d: _is_subnormal(d.coords).sum() > 0.9 * d.coords.size),
    Case("scales from 1e-30 to 1e30", lambda: scene(37, 600, [0, 1, 2, 4], coords=_scales),
         lambda d: np.abs(d.coords).min() < 1e-28 and np.abs(d.coords).max() > 1e28 and np.isfinite(d.coords).all()),
    Case("non-finite coordinate on a labelled point", lambda: _non_finite(True),
         lambda d: not np.isfinite(d.coords[d.inst >= 0]).all()),
    Case("non-finite coordinate on an unlabelled point", lambda: _non_finite(False),
         lambda d: np.isfinite(d.coords[d.inst >= 0]).all() and not np.isfinite(d.coords[d.inst < 0]).all()),
]
CASE_NAMES = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}


def build(name):
    c = BY_NAME[name]
    d = c.build()
    assert c.holds(d), "case %r no longer meets its condition" % name
    return d


def expected(fn, *args):
    """The restatement's result, or the Refused it raises (as a value)."""
    try:
        return fn(*args)
    except ref.Refused as e:
        return e
