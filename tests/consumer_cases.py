"""Inputs of the consumer-op edge tests (test_consumer_edges_cpu.py / test_consumer_edges_gpu.py) and plain NumPy float64
references of the three ops to hold gapro_amd/consumer_ops.py to.

The references are written from the reference's lines (cited in oracle/consumer_oracle.py) and share no code with that
module or with the package:
* ``pool_reference``  -- custom_scatter_mean, ISBNet/isbnet/model/model_utils.py:600-613: the sum per index over the count
  clamped at 1.  ``pool_exact`` does the sum in integers for the cases whose values are k 2^-16.
* ``bce_reference``   -- criterion.py:287-288.  The gradient is the closed form w[p] (sigmoid(x) - y) / (sum w (G + 1e-6))
  with sigmoid(x) - y in the two-sided form that does not cancel: autograd through the value's expression does (in float64
  it loses digits from |x| = 24 on and returns 0 from 37 on).
* ``kl_reference``    -- criterion.py:435-463, value and both gradients per entry, every mask explicit.
Each reference takes switches that restate ONE mistake (``sigmoid="one_sided"``, ``strict_eps``, ``half_labelled``,
``count_eps`` / ``row_eps``, ``pool_float32_running``); test_consumer_edges_cpu.py uses them to show that the case built
for that mistake fails with it at the tolerance of the GPU file.

Every case is a named entry of POOL_CASES / BCE_CASES / KL_CASES; test_consumer_edges_cpu.py proves on the CPU that each
is what its builder's comment claims, so that nothing in the GPU file passes vacuously.
"""
from collections import OrderedDict, namedtuple
from functools import lru_cache

import numpy as np

F32, F64 = np.float32, np.float64

# structural constants of gapro_amd/csrc/consumer.hip that the cases are built around
THREADS = 256                    # per workgroup: 4 waves of 64 lanes
WAVE = 64
LOSS_SWEEP = 1024 * THREADS      # elements one sweep of the BCE and KL grids covers
POOL_SWEEP = 2048 * THREADS      # points one sweep of the pool's grid covers

# the project's tolerances (tests/test_consumer_gpu.py)
BCE_VALUE_RTOL = 2e-6
GRAD_RTOL = 2e-6
GRAD_ATOL = 1e-30                # 0 on the saturated case
KL_VALUE_RTOL = 1e-5
# the gradient is one float64 evaluation rounded once to float32 (relative error <= 2^-24): two float32 ulps hold it, and
# only at that resolution can a one-row case see the 1e-6 of the row count (rtol 2e-6 cannot: 1 / (1 + 1e-6) = 1 - 1e-6)
SHORT_GRAD_RTOL = 2.0 ** -22
SENTINEL = -100.0


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def ordered(a):
    """float32 values as integers in the order of the floats: the difference of two is their distance in ulps."""
    i = np.ascontiguousarray(a, F32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def ulp_distance(a, b):
    return np.abs(ordered(a) - ordered(b))


def is_normal_f32(v):
    v = np.abs(np.asarray(v, F64))
    return (v >= float(np.finfo(F32).tiny)) & (v <= float(np.finfo(F32).max))


# ========================================================================================== pool
PoolCase = namedtuple("PoolCase", "name idx chans n_out kind meta")
SCALE = 65536  # exact values are k / SCALE


def as_float32(chan):
    """What the wrapper feeds the kernel: the channel converted to float32."""
    return np.asarray(chan).astype(F32)


def pool_reference(case, n_out=None, pool_float32_running=False):
    """Float64 sum per index over max(count, 1), rounded to float32.  pool_float32_running: the mistake of summing in
    float32, point by point."""
    n_out = pool_n_out(case) if n_out is None else n_out
    count = np.zeros(n_out, np.int64)
    np.add.at(count, case.idx, 1)
    out = []
    for chan in case.chans:
        v = as_float32(chan)
        if pool_float32_running:
            s = np.zeros(n_out, F32)
            np.add.at(s, case.idx, v)
            out.append((s / np.maximum(count, 1).astype(F32)).astype(F32))
        else:
            s = np.zeros(n_out, F64)
            np.add.at(s, case.idx, v.astype(F64))
            out.append((s / np.maximum(count, 1).astype(F64)).astype(F32))
    return tuple(out), count


def pool_exact(case):
    """The same in integers: values k / 65536 summed as k (int64, exact), the one division done in float64 and rounded to
    float32 once, as the kernel rounds."""
    n_out = pool_n_out(case)
    count = np.zeros(n_out, np.int64)
    np.add.at(count, case.idx, 1)
    out = []
    for chan in case.chans:
        k = np.rint(as_float32(chan).astype(F64) * SCALE).astype(np.int64)
        s = np.zeros(n_out, np.int64)
        np.add.at(s, case.idx, k)
        out.append(((s.astype(F64) / SCALE) / np.maximum(count, 1).astype(F64)).astype(F32))
    return tuple(out), count


def pool_expected(case):
    return pool_exact(case) if case.kind == "exact" else pool_reference(case)


def pool_n_out(case):
    return int(case.idx.max()) + 1 if case.n_out is None else case.n_out


def _exact_channels(rng, n, step=1, dtype=F32):
    """prob in [0, 1], mu and var in [-100, 100] with the -100 sentinel on a fifth of the points, all k step / 65536."""
    top = SCALE // step
    prob = rng.integers(0, top + 1, size=n) * step
    mu = rng.integers(-100 * top, 100 * top + 1, size=n) * step
    var = rng.integers(0, 100 * top + 1, size=n) * step
    unl = rng.random(n) < 0.2
    mu[unl] = -100 * SCALE
    var[unl] = -100 * SCALE
    chans = tuple((c.astype(F64) / SCALE).astype(dtype) for c in (prob, mu, var))
    for c, k in zip(chans, (prob, mu, var)):
        assert np.array_equal(c.astype(F64) * SCALE, k.astype(F64))
    return chans


def _random_channels(rng, n, dtype=F32):
    """Ordinary values: nothing about their sums is exact."""
    prob = rng.random(n)
    mu = np.where(rng.random(n) < 0.3, SENTINEL, rng.normal(size=n))
    var = np.where(mu == SENTINEL, SENTINEL, rng.random(n) * 0.5)
    return tuple(c.astype(dtype) for c in (prob, mu, var))


def _covering_idx(rng, n, n_idx, empty=()):
    """n indices over [0, n_idx), every one but `empty` at least once, shuffled."""
    live = np.array([s for s in range(n_idx) if s not in empty], np.int64)
    idx = np.concatenate([live, rng.choice(live, size=n - len(live))])
    rng.shuffle(idx)
    return idx


def _pool(name, idx, chans, n_out=None, kind="exact", **meta):
    idx = np.ascontiguousarray(idx, np.int64)
    _freeze(idx, *chans)
    return PoolCase(name, idx, tuple(chans), n_out, kind, meta)


def _pool_n1():
    return _pool("n1", [0], _exact_channels(np.random.default_rng(1), 1))


def _pool_one_address():
    """n_out = 1 and more points than one sweep of the grid: every atomic of the launch lands on the same four words."""
    n = 600000
    return _pool("one_address", np.zeros(n, np.int64), _exact_channels(np.random.default_rng(2), n), n_out=1)


def _pool_n_out(n_out):
    rng = np.random.default_rng(100 + n_out)
    return _pool("n_out_%d" % n_out, _covering_idx(rng, 3000, n_out), _exact_channels(rng, 3000), n_out=n_out)


def _pool_empties():
    """Superpoints 0, 4 and 8 of 9 hold no point: their means are 0 (the count is clamped at 1)."""
    rng = np.random.default_rng(3)
    return _pool("empties", _covering_idx(rng, 700, 9, empty=(0, 4, 8)), _exact_channels(rng, 700), n_out=9,
                 empty=(0, 4, 8))


def _pool_trailing():
    """n_out = max + 1 + 300: more than a workgroup of trailing superpoints whose means are exactly 0."""
    rng = np.random.default_rng(4)
    return _pool("trailing", _covering_idx(rng, 500, 40), _exact_channels(rng, 500), n_out=340, used=40)


def _pool_derived_n_out():
    """n_out left to the wrapper (max + 1)."""
    rng = np.random.default_rng(5)
    return _pool("derived_n_out", _covering_idx(rng, 1000, 257), _exact_channels(rng, 1000))


def _pool_int32():
    rng = np.random.default_rng(6)
    return _pool("idx_int32", _covering_idx(rng, 1000, 77), _exact_channels(rng, 1000), n_out=77, idx_dtype="int32")


def _pool_cpu_idx():
    rng = np.random.default_rng(7)
    return _pool("idx_on_cpu", _covering_idx(rng, 1000, 77), _exact_channels(rng, 1000), n_out=77, idx_on_cpu=True)


def _pool_columns():
    """The three channels are the columns of one [n, 3] tensor: stride 3."""
    rng = np.random.default_rng(8)
    return _pool("columns", _covering_idx(rng, 1000, 77), _exact_channels(rng, 1000), n_out=77, columns=True)


def _pool_f16():
    """float16 channels: multiples of 1/16 up to 100 in magnitude are float16 values."""
    rng = np.random.default_rng(9)
    return _pool("chan_float16", _covering_idx(rng, 1000, 77), _exact_channels(rng, 1000, step=SCALE // 16, dtype=np.float16),
                 n_out=77)


def _pool_f64():
    """float64 channels whose conversion to float32 rounds: the expected means are those of the converted values."""
    rng = np.random.default_rng(10)
    return _pool("chan_float64", _covering_idx(rng, 1000, 77), _random_channels(rng, 1000, F64), n_out=77, kind="ulp")


def _pool_random(name, n, n_idx, seed):
    rng = np.random.default_rng(seed)
    return _pool(name, _covering_idx(rng, n, n_idx), _random_channels(rng, n), n_out=n_idx, kind="ulp")


POOL_CASES = OrderedDict([("n1", (_pool_n1, ())), ("one_address", (_pool_one_address, ()))])
for _s in (255, 256, 257):
    POOL_CASES["n_out_%d" % _s] = (_pool_n_out, (_s,))
POOL_CASES.update([
    ("empties", (_pool_empties, ())), ("trailing", (_pool_trailing, ())), ("derived_n_out", (_pool_derived_n_out, ())),
    ("idx_int32", (_pool_int32, ())), ("idx_on_cpu", (_pool_cpu_idx, ())), ("columns", (_pool_columns, ())),
    ("chan_float16", (_pool_f16, ())), ("chan_float64", (_pool_f64, ())),
    ("random_small", (_pool_random, ("random_small", 5000, 257, 11))),
    ("random_sweep", (_pool_random, ("random_sweep", POOL_SWEEP + 77, 1000, 12))),
])
POOL_CASE_NAMES = tuple(POOL_CASES)

# the guard of k_pool3_sum: the only out-of-range indices the canary test uses
CANARY_PAD = 64


def bad_indices(n_out):
    return (-2, -1, n_out, n_out + 1)


@lru_cache(maxsize=None)
def pool_guard_case():
    """77 superpoints, 1000 points of which every 25th carries one of the four out-of-range indices.  `clean` is the
    same case without those points: what the guarded kernel must compute."""
    rng = np.random.default_rng(13)
    n, n_out = 1000, 77
    idx = _covering_idx(rng, n, n_out)
    chans = _exact_channels(rng, n)
    bad = np.zeros(n, bool)
    bad[::25] = True
    dirty = idx.copy()
    dirty[bad] = np.resize(np.array(bad_indices(n_out), np.int64), int(bad.sum()))
    clean = _pool("guard_clean", idx[~bad], tuple(c[~bad] for c in chans), n_out=n_out)
    return _pool("guard_dirty", dirty, chans, n_out=n_out, bad=bad), clean


@lru_cache(maxsize=None)
def pool_case(name):
    fn, args = POOL_CASES[name]
    case = fn(*args)
    assert case.name == name
    return case


# ========================================================================================== weighted BCE
BceCase = namedtuple("BceCase", "name x y w meta")
SATURATED = (24.0, 30.0, 37.0, 40.0, 60.0)
EXTREME = (100.0, 1e4)


def sigmoid_minus_target(x, y, sigmoid="two_sided"):
    """sigmoid(x) - y in float64.  two_sided: with t = exp(-|x|), s = t / (1 + t) it is (1 - y) - s for x >= 0 and s - y
    for x < 0, exact for y in {0, 1}.  one_sided: 1 / (1 + exp(-x)) - y, the form that cancels."""
    x, y = np.asarray(x, F64), np.asarray(y, F64)
    if sigmoid == "one_sided":
        with np.errstate(over="ignore"):
            return 1.0 / (1.0 + np.exp(-x)) - y
    t = np.exp(-np.abs(x))
    s = t / (1.0 + t)
    return np.where(x >= 0, (1.0 - y) - s, s - y)


def bce_reference(case, sigmoid="two_sided", row_eps=1e-6):
    """(value, gradient) in float64 of criterion.py:287-288 at the case's values as the kernel sees them (float32)."""
    x, y, w = (np.asarray(a).astype(F32).astype(F64) for a in (case.x, case.y, case.w))
    rows = x.shape[0]
    per = np.maximum(x, 0.0) - x * y + np.log1p(np.exp(-np.abs(x)))
    with np.errstate(invalid="ignore", divide="ignore"):
        value = (per * w[None, :]).sum() / w.sum() / (rows + row_eps)
        grad = w[None, :] * sigmoid_minus_target(x, y, sigmoid) / (w.sum() * (rows + row_eps))
    return float(value), grad


def _bce(name, x, y, w, **meta):
    x, y, w = np.ascontiguousarray(x), np.ascontiguousarray(y), np.ascontiguousarray(w, F32)
    _freeze(x, y, w)
    return BceCase(name, x, y, w, meta)


def _moderate_logits(rng, G, P):
    """|x| <= 10: the oracle's float64 autograd still has nine digits of sigmoid(x) - y there."""
    return np.clip(3.0 * rng.normal(size=(G, P)), -10.0, 10.0).astype(F32)


def _bce_shape(G, P):
    rng = np.random.default_rng(1000 * G + P)
    x = _moderate_logits(rng, G, P)
    return _bce("shape_%dx%d" % (G, P), x, (rng.random((G, P)) < 0.3).astype(F32), (0.5 + 0.5 * rng.random(P)).astype(F32),
                moderate=True)


def _bce_zero_columns():
    """A third of the columns weigh nothing: their gradient is exactly 0."""
    rng = np.random.default_rng(20)
    G, P = 3, 301
    w = (0.5 + 0.5 * rng.random(P)).astype(F32)
    w[::3] = 0.0
    return _bce("zero_columns", _moderate_logits(rng, G, P), (rng.random((G, P)) < 0.5).astype(F32), w, moderate=True)


def _bce_soft():
    """Targets in [0.05, 0.95]."""
    rng = np.random.default_rng(21)
    G, P = 4, 263
    return _bce("soft_targets", _moderate_logits(rng, G, P), (0.05 + 0.9 * rng.random((G, P))).astype(F32),
                (0.5 + 0.5 * rng.random(P)).astype(F32), moderate=True)


def _bce_bool():
    rng = np.random.default_rng(22)
    G, P = 2, 300
    return _bce("bool_targets", _moderate_logits(rng, G, P), rng.random((G, P)) < 0.4, (0.5 + 0.5 * rng.random(P)).astype(F32),
                moderate=True)


def _confident(magnitudes, rng, G, P):
    """Every (magnitude, sign, target) combination, tiled over [G, P] in a shuffled order: confident and right
    (sign agrees with the target) as often as confident and wrong."""
    combos = np.array([(m * s, t) for m in magnitudes for s in (1.0, -1.0) for t in (0.0, 1.0)])
    pick = np.resize(rng.permutation(len(combos)), G * P)
    rng.shuffle(pick)
    return combos[pick, 0].reshape(G, P).astype(F32), combos[pick, 1].reshape(G, P).astype(F32)


def _bce_saturated():
    """Hard targets, |x| in {24, 30, 37, 40, 60}.  sum w (G + 1e-6) <= 4 * 320, so that the smallest expected gradient,
    0.5 exp(-60) / 1280 = 3.4e-30, is a normal float32: all are compared with atol 0."""
    rng = np.random.default_rng(23)
    G, P = 4, 320
    x, y = _confident(SATURATED, rng, G, P)
    return _bce("saturated", x, y, (0.5 + 0.5 * rng.random(P)).astype(F32))


def _bce_extreme():
    """|x| in {100, 1e4}: exp(-|x|) is below every float32.  Checked apart: the value, the confident-and-wrong gradients,
    and that the confident-and-right ones are at most 1e-37 in magnitude."""
    rng = np.random.default_rng(24)
    G, P = 2, 64
    x, y = _confident(EXTREME, rng, G, P)
    return _bce("extreme", x, y, (0.5 + 0.5 * rng.random(P)).astype(F32))


def _bce_zero_weights():
    """sum w = 0: the reference's lines divide 0 by 0."""
    rng = np.random.default_rng(25)
    G, P = 2, 70
    return _bce("zero_weights", _moderate_logits(rng, G, P), (rng.random((G, P)) < 0.5).astype(F32), np.zeros(P, F32))


def _bce_transposed():
    """The logits reach the op as the transpose of a [P, G] tensor (meta: the test builds that tensor from x.T)."""
    rng = np.random.default_rng(26)
    G, P = 5, 259
    return _bce("transposed", _moderate_logits(rng, G, P), (rng.random((G, P)) < 0.3).astype(F32),
                (0.5 + 0.5 * rng.random(P)).astype(F32), moderate=True, transposed=True)


def _to_bfloat16_values(x):
    """float32 values with the low 16 bits cleared: exactly the bfloat16 numbers."""
    return (np.ascontiguousarray(x, F32).view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)


def _bce_low_precision(dtype):
    rng = np.random.default_rng(27 + len(dtype))
    G, P = 3, 257
    x = _moderate_logits(rng, G, P)
    x = x.astype(np.float16).astype(F32) if dtype == "float16" else _to_bfloat16_values(x)
    return _bce("logits_" + dtype, x, (rng.random((G, P)) < 0.3).astype(F32), (0.5 + 0.5 * rng.random(P)).astype(F32),
                moderate=True, dtype=dtype)


def _bce_no_grad():
    """requires_grad=False: one workgroup, a null gradient pointer.  More than one sweep of the reduction's grid."""
    rng = np.random.default_rng(29)
    G, P = 3, 87382
    return _bce("no_grad", _moderate_logits(rng, G, P), (rng.random((G, P)) < 0.3).astype(F32),
                (0.5 + 0.5 * rng.random(P)).astype(F32), moderate=True, no_grad=True)


BCE_SHAPES = ((1, 1), (1, 255), (1, 256), (1, 257), (3, 87382), (5, 52429))
BCE_CASES = OrderedDict(("shape_%dx%d" % gp, (_bce_shape, gp)) for gp in BCE_SHAPES)
BCE_CASES.update([
    ("zero_columns", (_bce_zero_columns, ())), ("soft_targets", (_bce_soft, ())), ("bool_targets", (_bce_bool, ())),
    ("saturated", (_bce_saturated, ())), ("extreme", (_bce_extreme, ())), ("zero_weights", (_bce_zero_weights, ())),
    ("transposed", (_bce_transposed, ())), ("logits_float16", (_bce_low_precision, ("float16",))),
    ("logits_bfloat16", (_bce_low_precision, ("bfloat16",))), ("no_grad", (_bce_no_grad, ())),
])
BCE_CASE_NAMES = tuple(BCE_CASES)
# the cases test_bce_value_and_gradient runs as they are; the others have a test of their own
BCE_PLAIN = tuple(n for n in BCE_CASE_NAMES if n not in ("extreme", "zero_weights", "logits_float16", "logits_bfloat16",
                                                         "no_grad"))


@lru_cache(maxsize=None)
def bce_case(name):
    fn, args = BCE_CASES[name]
    case = fn(*args)
    assert case.name == name
    return case


@lru_cache(maxsize=None)
def bce_expected(name):
    value, grad = bce_reference(bce_case(name))
    grad.setflags(write=False)
    return value, grad


# ========================================================================================== KL to GP
KlCase = namedtuple("KlCase", "name mu_l var_l mu_p lv_p weight eps meta")
EPS = 1e-4
UNLABELLED, TINY, REST = 0, 1, 2


def kl_branches(case, strict_eps=False, half_labelled=False):
    """Per entry: UNLABELLED if either label is -100, TINY if var <= eps, REST otherwise.  The compare is the
    reference's: a float32 tensor against the Python float, which torch rounds to float32 first.
    strict_eps: the mistake var < eps.  half_labelled: the mistake of ignoring an entry only if BOTH labels are -100."""
    mu_l, var_l = case.mu_l, case.var_l
    if half_labelled:
        labelled = ~((mu_l == F32(SENTINEL)) & (var_l == F32(SENTINEL)))
    else:
        labelled = (mu_l != F32(SENTINEL)) & (var_l != F32(SENTINEL))
    tiny = (var_l < F32(case.eps)) if strict_eps else (var_l <= F32(case.eps))
    return np.where(labelled, np.where(tiny, TINY, REST), UNLABELLED)


def kl_reference(case, strict_eps=False, half_labelled=False, count_eps=1e-4):
    """(value, d value / d mu_pred, d value / d logvar_pred) in float64, flat.  ``mask.sum() + 1e-4`` of the reference's lines
    is an integer tensor plus a Python float, which torch evaluates in float32: the group sizes are rounded so here."""
    br = kl_branches(case, strict_eps, half_labelled).reshape(-1)
    mu_l, var_l, mu_p, lv = (np.asarray(a, F32).astype(F64).reshape(-1) for a in (case.mu_l, case.var_l, case.mu_p, case.lv_p))
    value, g_mu, g_lv = 0.0, np.zeros(len(br)), np.zeros(len(br))
    tiny, rest = br == TINY, br == REST
    if tiny.sum() > 0:  # :446-452
        scale = case.weight / float(F32(int(tiny.sum()) + count_eps))
        e, d = np.exp(lv[tiny]), mu_p[tiny] - mu_l[tiny]
        value += scale * ((e - 1.0) ** 2 + d ** 2).sum()
        g_mu[tiny] = scale * 2.0 * d
        g_lv[tiny] = scale * 2.0 * (e - 1.0) * e
    if rest.sum() > 0:  # :454-463
        scale = case.weight / float(F32(int(rest.sum()) + count_eps))
        v, d, l = var_l[rest], mu_p[rest] - mu_l[rest], lv[rest]
        with np.errstate(invalid="ignore", divide="ignore"):  # only a restated mistake brings a variance <= 0 here
            e2 = np.exp(-2.0 * l)
            value += scale * ((l - np.log(v)) + (d ** 2 + v ** 2) * e2 - 0.5).sum()
        g_mu[rest] = scale * 2.0 * d * e2
        g_lv[rest] = scale * (1.0 - 2.0 * (d ** 2 + v ** 2) * e2)
    return float(value), g_mu, g_lv


def _kl(name, mu_l, var_l, mu_p, lv_p, weight=1.0, eps=EPS, **meta):
    arrays = tuple(np.ascontiguousarray(a, F32) for a in (mu_l, var_l, mu_p, lv_p))
    _freeze(*arrays)
    return KlCase(name, *arrays, float(weight), float(eps), meta)


def _kl_labels(rng, n, p_tiny=0.3, p_unlabelled=0.3):
    """Labels of the three kinds at random: tiny variances of 5e-5, unlabelled entries -100 in both."""
    r = rng.random(n)
    mu_l = rng.normal(size=n)
    var_l = 0.01 + 0.5 * rng.random(n)
    var_l[r < p_tiny] = 5e-5
    unl = (r >= p_tiny) & (r < p_tiny + p_unlabelled)
    mu_l[unl] = SENTINEL
    var_l[unl] = SENTINEL
    return mu_l, var_l


def _kl_preds(rng, n, lv_scale=0.5):
    return rng.normal(size=n), lv_scale * rng.normal(size=n)


def _kl_n1(branch):
    rng = np.random.default_rng(30 + branch)
    mu_l, var_l = {UNLABELLED: (SENTINEL, SENTINEL), TINY: (0.3, 5e-5), REST: (0.3, 0.2)}[branch]
    mu_p, lv = _kl_preds(rng, 1)
    return _kl("n1_" + ("unlabelled", "tiny", "rest")[branch], [mu_l], [var_l], mu_p, lv, branch=branch)


def _kl_mixed(n):
    rng = np.random.default_rng(40 + n % 1000)
    return _kl("mixed_%d" % n, *_kl_labels(rng, n), *_kl_preds(rng, n), weight=0.7)


def _kl_only(branch):
    rng = np.random.default_rng(50 + branch)
    n = 300
    p = {TINY: (1.0, 0.0), REST: (0.0, 0.0), UNLABELLED: (0.0, 1.0)}[branch]
    return _kl("only_" + ("unlabelled", "tiny", "rest")[branch], *_kl_labels(rng, n, *p), *_kl_preds(rng, n), branch=branch)


def _kl_half_labelled():
    """A third of the entries have mu = -100 and a valid variance (half of them a tiny one), a third a valid mu and
    var = -100, a third both valid: only the last third counts."""
    rng = np.random.default_rng(60)
    n = 300
    mu_l, var_l = _kl_labels(rng, n, p_tiny=0.5, p_unlabelled=0.0)
    kind = np.arange(n) % 3
    mu_l[kind == 0] = SENTINEL
    var_l[kind == 1] = SENTINEL
    return _kl("half_labelled", mu_l, var_l, *_kl_preds(rng, n), kind=kind)


def _kl_eps_boundary(eps=EPS, weight=1.0, name="eps_boundary"):
    """100 entries each with var = float32(eps), the float32 below it and the float32 above it."""
    rng = np.random.default_rng(61)
    n = 300
    e = F32(eps)
    around = np.array([np.nextafter(e, F32(0)), e, np.nextafter(e, F32(1))], F32)
    return _kl(name, rng.normal(size=n), around[np.arange(n) % 3], *_kl_preds(rng, n), weight=weight, eps=eps,
               around=around)


def _kl_zero_variance():
    rng = np.random.default_rng(62)
    n = 260
    mu_l, var_l = _kl_labels(rng, n, p_tiny=0.0, p_unlabelled=0.2)
    var_l[::2] = np.where(var_l[::2] == SENTINEL, SENTINEL, 0.0)
    return _kl("zero_variance", mu_l, var_l, *_kl_preds(rng, n))


def _kl_negative_variance():
    """Variances of -0.25, -1e-6 and -99.5 (not the sentinel): var <= eps holds, the reference puts them in the tiny
    branch, and the logarithm of the other branch never sees them."""
    rng = np.random.default_rng(63)
    n = 260
    mu_l, var_l = _kl_labels(rng, n, p_tiny=0.0, p_unlabelled=0.2)
    neg = np.resize(np.array([-0.25, -1e-6, -99.5]), len(var_l[::2]))
    var_l[::2] = np.where(var_l[::2] == SENTINEL, SENTINEL, neg)
    return _kl("negative_variance", mu_l, var_l, *_kl_preds(rng, n))


def _kl_options():
    """epsilon = 2^-6 (the 5e-5 .. 0.5 labels fall on both sides of it) and weight = 2.5."""
    rng = np.random.default_rng(64)
    n = 400
    mu_l, var_l = _kl_labels(rng, n)
    live = var_l > 1e-3
    var_l[live] = 0.001 + 0.04 * rng.random(int(live.sum()))
    return _kl("options", mu_l, var_l, *_kl_preds(rng, n), weight=2.5, eps=2.0 ** -6)


def _kl_batched():
    """Predictions and labels shaped [3, 173]."""
    rng = np.random.default_rng(65)
    n = 3 * 173
    arrays = _kl_labels(rng, n) + _kl_preds(rng, n)
    return _kl("batched", *(a.reshape(3, 173) for a in arrays), shape=(3, 173))


def _kl_grad_of(which):
    rng = np.random.default_rng(66 + len(which))
    n = 300
    return _kl("grad_" + which, *_kl_labels(rng, n), *_kl_preds(rng, n), requires={"logvar_only": (False, True),
                                                                                    "none": (False, False)}[which])


def _kl_near_converged():
    """mu_pred - mu_label and logvar_pred of order 1e-3: next to the optimum of the tiny branch (logvar = 0, mu = label),
    where exp(logvar) - 1 cancels in float32."""
    rng = np.random.default_rng(68)
    n = 20000
    mu_l, var_l = _kl_labels(rng, n, p_tiny=0.5, p_unlabelled=0.1)
    mu_p = np.where(mu_l == SENTINEL, 0.0, mu_l) + 1e-3 * rng.normal(size=n)
    lv = 1e-3 * rng.normal(size=n)
    return _kl("near_converged", mu_l, var_l, mu_p, lv)


def _kl_wide_logvar():
    rng = np.random.default_rng(69)
    n = 3000
    return _kl("wide_logvar", *_kl_labels(rng, n), rng.normal(size=n), rng.uniform(-10.0, 10.0, size=n))


KL_CASES = OrderedDict(("n1_" + ("unlabelled", "tiny", "rest")[b], (_kl_n1, (b,))) for b in (UNLABELLED, TINY, REST))
for _n in (255, 256, 257, LOSS_SWEEP + 1):
    KL_CASES["mixed_%d" % _n] = (_kl_mixed, (_n,))
KL_CASES.update([
    ("only_tiny", (_kl_only, (TINY,))), ("only_rest", (_kl_only, (REST,))), ("only_unlabelled", (_kl_only, (UNLABELLED,))),
    ("half_labelled", (_kl_half_labelled, ())), ("eps_boundary", (_kl_eps_boundary, ())),
    ("eps_boundary_options", (_kl_eps_boundary, (2.0 ** -6, 2.5, "eps_boundary_options"))),
    ("zero_variance", (_kl_zero_variance, ())), ("negative_variance", (_kl_negative_variance, ())),
    ("options", (_kl_options, ())), ("batched", (_kl_batched, ())), ("grad_logvar_only", (_kl_grad_of, ("logvar_only",))),
    ("grad_none", (_kl_grad_of, ("none",))), ("near_converged", (_kl_near_converged, ())),
    ("wide_logvar", (_kl_wide_logvar, ())),
])
KL_CASE_NAMES = tuple(KL_CASES)


@lru_cache(maxsize=None)
def kl_case(name):
    fn, args = KL_CASES[name]
    case = fn(*args)
    assert case.name == name
    return case


@lru_cache(maxsize=None)
def kl_expected(name):
    value, g_mu, g_lv = kl_reference(kl_case(name))
    _freeze(g_mu, g_lv)
    return value, g_mu, g_lv
