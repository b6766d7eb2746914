"""Case tables, generators and float64 references of the prediction-edge tests (test_predict_edges_cpu.py /
test_predict_edges_gpu.py), and the comparison that test_predict_gpu.py shares with them.

Reference of every comparison: oracle.svgp_oracle.svgp_predict, the float64 posterior of a STATE (no training), at the
float32 feature rows the kernel reads.  Tolerance (``_check``): two correct float64 evaluations of one state agree far
inside a float32 half-ulp, so both round to float32 values at most one unit in the last place apart -- var rtol 2^-23,
mu rtol 2^-23 + atol 1e-10, probs atol 1.2e-7, labels equal wherever the reference's |p - 0.5| > 1e-6 (at most 0.1 % of
a model's rows may be left out), probs_new == where(labels, probs, 1 - probs) exactly.  ``reference_gap`` is the
precondition of that argument: the same state evaluated with an explicit inv(L) and matrix products instead of
triangular solves must give the same var to 1e-9 relative and the same mu to 1e-9 (under 2 % of 2^-24).

Part 1, hand-made states (``hand_model``): dense K_ZZ (length scale = the typical distance of two points), a dense
L_S, so that every 16-block of L^-1 and L_S carries weight in the result.
Part 2, the fit kernels' own prediction tails (``FIT_SHAPES``): one launch per shape whose problems share a training
set and differ in T only, T at the edges of the tail's column chunk.
Part 3, one-point sides (``SIDE_CASES``) against the trained float64 oracle.
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

ULP = 2.0 ** -23
GAP_BOUND = 1e-9  # reference_gap: var relative, mu absolute


def _check(out, ref, what="", untrained=False):
    """out: the 5-tuple of the library; ref: (mu, var, p) in float64.  untrained: a model at zero Adam steps predicts
    the prior, p = 0.5 exactly at every row; there the labels must agree on ALL rows (no row is left out as a tie)."""
    probs, probs_new, labels, mu, var = out
    mu_r, var_r, p_r = ref
    assert probs.dtype == np.float32 and mu.dtype == np.float32 and var.dtype == np.float32 and labels.dtype == bool
    dv = np.max(np.abs(var.astype(np.float64) - var_r.astype(np.float32)) / var_r) if len(var) else 0.0
    dm = np.max(np.abs(mu.astype(np.float64) - mu_r.astype(np.float32))) if len(mu) else 0.0
    dp = np.max(np.abs(probs.astype(np.float64) - p_r.astype(np.float32))) if len(mu) else 0.0
    print("%s rows %d: var rel %.3e  mu abs %.3e  p abs %.3e" % (what, len(mu), dv, dm, dp))
    np.testing.assert_allclose(var, var_r.astype(np.float32), rtol=ULP, atol=0, err_msg=what)
    np.testing.assert_allclose(mu, mu_r.astype(np.float32), rtol=ULP, atol=1e-10, err_msg=what)
    np.testing.assert_allclose(probs, p_r.astype(np.float32), rtol=0, atol=1.2e-7, err_msg=what)
    safe = np.abs(p_r - 0.5) > 1e-6
    if untrained:
        assert (p_r == 0.5).all() and (probs == np.float32(0.5)).all()
        safe[:] = True
    assert (~safe).mean() <= 1e-3 if len(safe) else True
    np.testing.assert_array_equal(labels[safe], (p_r.astype(np.float32) >= np.float32(0.5))[safe])
    np.testing.assert_array_equal(probs_new, np.where(labels, probs, np.float32(1) - probs))


def _as_ref(out):
    """A fit's own five outputs as a (mu, var, p) reference (float32 values held in float64)."""
    return out[3].astype(np.float64), out[4].astype(np.float64), out[0].astype(np.float64)


def _oracle(model, X, chunk=2000):
    from oracle import svgp_oracle as so

    s, ell = model.outputscale, model.lengthscale
    d2 = ((model.Z[:, None, :] - model.Z[None, :, :]) ** 2).sum(-1)
    L = np.linalg.cholesky(s * np.exp(-0.5 * d2 / (ell * ell)) + model.jitter * np.eye(model.m))
    outs = [so.svgp_predict(X[a:a + chunk].astype(np.float64), model.Z, model.mean, model.LS, model.c, model.rho_s,
                            model.rho_l, jitter=model.jitter, L=L) for a in range(0, len(X), chunk)]
    return tuple(np.concatenate([o[k] for o in outs]) for k in range(3))


def deviations(out, ref):
    """(var relative, mu absolute, p absolute) of a 5-tuple against a float64 reference, as ``_check`` prints them."""
    if not len(out[0]):
        return 0.0, 0.0, 0.0
    mu_r, var_r, p_r = ref
    return (float(np.max(np.abs(out[4].astype(np.float64) - var_r.astype(np.float32)) / var_r)),
            float(np.max(np.abs(out[3].astype(np.float64) - mu_r.astype(np.float32)))),
            float(np.max(np.abs(out[0].astype(np.float64) - p_r.astype(np.float32)))))


# ---------------------------------------------------------------------------------------------------------------------
# part 0: the reference against itself
def inv_l(model):
    """L^-1 of the model's K_ZZ + jitter I as an explicit matrix (float64)."""
    from scipy.linalg import solve_triangular

    s, ell = model.outputscale, model.lengthscale
    d2 = ((model.Z[:, None, :] - model.Z[None, :, :]) ** 2).sum(-1)
    L = np.linalg.cholesky(s * np.exp(-0.5 * d2 / (ell * ell)) + model.jitter * np.eye(model.m))
    return solve_triangular(L, np.eye(model.m), lower=True)


def oracle_by_inverse(model, X, min_variance=1e-6):
    """The posterior of ``_oracle`` evaluated another way: A = inv(L) K_ZX by a matrix product."""
    from scipy.special import ndtr

    s, ell = model.outputscale, model.lengthscale
    X = np.asarray(X, dtype=np.float64)
    d2 = ((model.Z[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    A = inv_l(model) @ (s * np.exp(-0.5 * d2 / (ell * ell)))
    mu = A.T @ model.mean + model.c
    B = np.tril(model.LS).T @ A
    var = np.maximum(s + model.jitter + (B * B - A * A).sum(0), min_variance)
    return mu, var, ndtr(mu / np.sqrt(1.0 + var))


def reference_gap(ref, model, X):
    """(max |dvar| / var, max |dmu|) between ``ref`` = _oracle(model, X) and the evaluation by an explicit inverse."""
    if not len(X):
        return 0.0, 0.0
    mu2, var2, _ = oracle_by_inverse(model, X)
    return float(np.max(np.abs(var2 - ref[1]) / ref[1])), float(np.max(np.abs(mu2 - ref[0])))


def offdiag_share(Li, b=16):
    """Share of the Frobenius norm of a square matrix that lies outside its diagonal b x b blocks."""
    M = len(Li)
    blk = np.arange(M) // b
    off = blk[:, None] != blk[None, :]
    return float(np.sqrt((Li[off] ** 2).sum() / (Li ** 2).sum()))


# ---------------------------------------------------------------------------------------------------------------------
# part 1: hand-made states for gapro_svgp_predict_batch
HAND_M = (1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 272, 530, 1040)
HAND_D = (1, 6, 7, 32, 40)
HAND_T = (1, 15, 16, 17, 31, 32, 33, 63, 65, 390)
CLASS_CAPS = (64, 128, 256)  # padded sizes up to which a model's column block lives in LDS, by launch class
N_ORDINARY, N_NEAR, N_FAR, FAR_SCALE = 300, 50, 40, 6.0
RESEED = {(2, 7): 1}  # (M, D) -> seed offset of a case that missed a precondition of test_predict_edges_cpu.py


def std_of(d):
    return 1.0 if d <= 8 else 0.3


def hand_sizes(d):
    """M >= 530 at D = 40 adds nothing to D = 32 (one any-width build) and is left out."""
    return tuple(m for m in HAND_M if m < 530 or d in (6, 7, 32))


def launch_class(m):
    """0, 1, 2: column block in LDS with M_p <= 64 / 128 / 256; 3: a workspace slice under a grid-stride loop."""
    mp = (m + 15) // 16 * 16
    return sum(mp > c for c in CLASS_CAPS)


def _inv_softplus(v):
    return float(np.log(np.expm1(v)))


@lru_cache(maxsize=None)
def hand_model(m, d):
    from gapro_amd.gp_model import GPModel

    rng = np.random.default_rng(100000 * RESEED.get((m, d), 0) + 100 * m + d)
    std = std_of(d)
    Z = std * rng.standard_normal((m, d))
    mean = 0.5 * rng.standard_normal(m)
    LS = np.diag(rng.uniform(0.3, 1.0, m)) + 0.2 * np.tril(rng.standard_normal((m, m)), -1) / np.sqrt(m)
    return GPModel(Z, mean, LS, 0.1, 0.3, _inv_softplus(np.sqrt(d) * std), 1e-4, 0)


@lru_cache(maxsize=None)
def hand_table(m, d):
    """(rows f32[R, D], kind i8[R]: 0 ordinary, 1 an inducing point shifted by 0.01, 2 at six times the scale, where
    k(Z, x) vanishes), R = 340 + min(M, 50), shuffled."""
    rng = np.random.default_rng(7000000 + 100 * m + d)
    std = std_of(d)
    near = hand_model(m, d).Z[:min(m, N_NEAR)] + 0.01
    rows = np.concatenate([std * rng.standard_normal((N_ORDINARY, d)), near,
                           FAR_SCALE * std * rng.standard_normal((N_FAR, d))]).astype(np.float32)
    kind = np.r_[np.zeros(N_ORDINARY, np.int8), np.ones(len(near), np.int8), np.full(N_FAR, 2, np.int8)]
    perm = rng.permutation(len(rows))
    rows, kind = rows[perm], kind[perm]
    rows.setflags(write=False)
    kind.setflags(write=False)
    return rows, kind


@lru_cache(maxsize=None)
def hand_reference(m, d):
    """_oracle of the model at every row of its table, computed once and shared (read-only)."""
    ref = _oracle(hand_model(m, d), hand_table(m, d)[0])
    for a in ref:
        a.setflags(write=False)
    return ref


def hand_row_vector(m, d, n=max(HAND_T)):
    """Row indices into hand_table(m, d): every row once in shuffled order, then repeats up to n entries."""
    r = len(hand_table(m, d)[0])
    rng = np.random.default_rng(9000000 + 100 * m + d)
    return np.concatenate([rng.permutation(r), rng.integers(0, r, size=max(n - r, 0))])[:max(n, r)].astype(np.int64)


Entry = namedtuple("Entry", "m t start")  # one model of a mixed launch: rows hand_row_vector(m, d)[start:start + t]


@lru_cache(maxsize=None)
def mixed_launch(d):
    """The entries of the mixed launch of feature width d: every size of hand_sizes(d), a launch class's models taken
    in turn (a model may occur more than once) until every T of HAND_T has occurred in the class."""
    rng = np.random.default_rng(31 + d)
    entries = []
    for cls in range(4):
        ms = [m for m in hand_sizes(d) if launch_class(m) == cls]
        n = max(len(ms), len(HAND_T))
        ts = list(rng.permutation(HAND_T)) + list(rng.choice(HAND_T, size=n - len(HAND_T)))
        for k in range(n):
            t = int(ts[k])
            entries.append(Entry(ms[k % len(ms)], t, int(rng.integers(0, max(HAND_T) - t + 1))))
    order = rng.permutation(len(entries))  # sizes interleaved: the library sorts them into its classes itself
    return tuple(entries[i] for i in order)


def launch_arrays(d, entries):
    """(models, feats f32[R, D], rows per entry, table rows per entry) of a launch: the tables of the sizes that occur,
    back to back."""
    sizes = sorted({e.m for e in entries})
    base, tables = {}, []
    off = 0
    for m in sizes:
        base[m] = off
        tables.append(hand_table(m, d)[0])
        off += len(tables[-1])
    local = [hand_row_vector(e.m, d)[e.start:e.start + e.t] for e in entries]
    return ([hand_model(e.m, d) for e in entries], np.concatenate(tables),
            [loc + base[e.m] for e, loc in zip(entries, local)], local)


def sliced(ref, idx):
    return tuple(a[idx] for a in ref)


# ---------------------------------------------------------------------------------------------------------------------
# part 2: the fit kernels' prediction tails
FitShape = namedtuple("FitShape", "d m route mp note")
FIT_SHAPES = (
    FitShape(6, 16, 5, 16, ""), FitShape(6, 17, 5, 32, ""), FitShape(6, 48, 5, 48, ""),
    FitShape(6, 49, 3, 64, ""), FitShape(6, 64, 3, 64, ""),
    FitShape(6, 65, 0, 80, ""), FitShape(6, 128, 0, 128, ""),
    FitShape(6, 129, 1, 144, ""), FitShape(6, 256, 1, 256, "workgroup-tiled, KMIN"),
    FitShape(6, 257, 1, 272, "beyond KMIN"), FitShape(6, 320, 1, 320, "TU 4"),
    FitShape(6, 384, 1, 384, "workgroup-tiled"), FitShape(6, 480, 1, 480, ""),
    FitShape(6, 512, 4, 512, "4 workgroups"), FitShape(6, 640, 4, 640, "8 workgroups"),
    FitShape(32, 32, 5, 32, ""), FitShape(32, 48, 3, 48, ""), FitShape(32, 96, 0, 96, ""),
    FitShape(32, 208, 1, 208, ""), FitShape(32, 224, 4, 224, "one workgroup"),
    FitShape(20, 320, 4, 320, ""),
    FitShape(40, 50, 2, 64, ""), FitShape(40, 130, 2, 160, ""),
)
FIT_IDS = ["d%d_m%d_route%d" % (s.d, s.m, s.route) for s in FIT_SHAPES]
FIT_ITERS = {}  # (d, m) -> Adam steps where 50 take too long for a test; never below 10
LS_TRAINED = 0.01  # max |tril(L_S) - I| a trained model must reach for the L_S product to matter


def fit_iters(shape):
    return FIT_ITERS.get((shape.d, shape.m), 50)


def chunk_width(shape):
    """Test columns per trip of the tail's loop: 16 in the wave-per-fit kernel, M_p elsewhere."""
    return 16 if shape.route == 5 else shape.mp


def fit_ts(shape):
    """The T of a launch's problems, in launch order.  The outputs of a launch are packed back to back, so a tail that
    writes past its last column shows in the next problem: the order is descending, every problem is followed by one
    that finishes no later, and the last one has T = W, a whole chunk -- a tail that rounds its last chunk up to W
    columns still stays inside the launch's buffers."""
    w = chunk_width(shape)
    ts = {0, 1, w - 1, w + 1, 2 * w + 17}
    if shape.route == 4:
        ts |= {31, 32, 33}  # the cluster tail reads Xt with leading dimension round_up(T, 32)
    return tuple(sorted(ts - {w}, reverse=True)) + (w,)


@lru_cache(maxsize=None)
def fit_problem(shape):
    """(feats f32[S, D], b1, b2, test index vector per T of fit_ts(shape)).  The feature table is the training set
    of make_gp_problem, its 300 ordinary test rows and 40 rows at six times the scale; a problem's test vector is a
    slice of one vector drawn with repeats from the ordinary rows, (at most 50) training rows and the far rows."""
    from gapro_amd.synth import make_gp_problem

    m1 = shape.m // 2 - 3
    m2 = shape.m - m1
    std = std_of(shape.d)
    feats, b1, b2, it = make_gp_problem(500 + shape.m + shape.d, m1, m2, N_ORDINARY, shape.d, std=std)
    rng = np.random.default_rng(40000 + 100 * shape.m + shape.d)
    far = (FAR_SCALE * std * rng.standard_normal((N_FAR, shape.d))).astype(np.float32)
    feats = np.concatenate([feats, far])
    pool = np.concatenate([it, rng.choice(shape.m, size=min(shape.m, N_NEAR), replace=False),
                           np.arange(len(feats) - N_FAR, len(feats))])
    n = max(fit_ts(shape))
    vec = rng.choice(pool, size=max(n, len(pool)) + 64).astype(np.int64)
    tests = tuple(vec[s:s + t] for t, s in ((t, int(rng.integers(0, len(vec) - t + 1))) for t in fit_ts(shape)))
    feats.setflags(write=False)
    return feats, b1, b2, tests


# ---------------------------------------------------------------------------------------------------------------------
# part 3: one-point sides on every route.  gap = (var relative, mu absolute, p absolute) between the two float64
# oracles (torch autograd, NumPy with the hand-derived backward) at the case's test rows, measured by
# test_predict_edges_cpu.py::test_one_point_sides_have_a_reproducible_reference
SideCase = namedtuple("SideCase", "m1 m2 d route seed gap")
SIDE_T = 33
SIDE_CASES = (
    SideCase(1, 63, 6, 3, 0, (6.2e-14, 3.5e-14, 1.8e-15)),
    SideCase(63, 1, 6, 3, 0, (1.3e-13, 8.0e-14, 3.3e-15)),
    SideCase(1, 127, 6, 0, 0, (7.9e-14, 8.4e-14, 7.7e-15)),
    SideCase(127, 1, 6, 0, 0, (1.3e-13, 1.7e-13, 9.9e-15)),
    SideCase(1, 128, 6, 1, 0, (1.1e-12, 3.8e-13, 3.2e-14)),
    SideCase(128, 1, 6, 1, 0, (2.8e-12, 2.3e-12, 1.0e-13)),
    SideCase(15, 114, 6, 1, 0, (1.6e-12, 2.0e-12, 3.1e-13)),
    SideCase(17, 112, 6, 1, 0, (6.9e-13, 8.7e-13, 2.8e-13)),
    SideCase(1, 223, 32, 4, 0, (2.1e-13, 1.3e-13, 3.9e-15)),
)
SIDE_IDS = ["%d_%d_d%d" % (c.m1, c.m2, c.d) for c in SIDE_CASES]
# test_fit_gpu.py::_compare: var rtol, mu rtol, mu atol, p atol; the two oracles must agree within a hundredth
COMPARE_TOL = dict(var_rtol=1e-5, mu_rtol=1e-5, mu_atol=1e-7, p_atol=2e-7)


@lru_cache(maxsize=None)
def side_problem(case):
    from gapro_amd.synth import make_gp_problem

    return make_gp_problem(900 + 7 * case.m1 + case.m2 + 1000 * case.seed, case.m1, case.m2, SIDE_T, case.d,
                           std=std_of(case.d))


@lru_cache(maxsize=None)
def side_reference(case, impl="autograd"):
    from fit_option_cases import few_threads
    from oracle import svgp_oracle as so

    feats, b1, b2, it = side_problem(case)
    X = np.concatenate([feats[b1], feats[b2]]).astype(np.float64)
    y = np.r_[-np.ones(len(b1)), np.ones(len(b2))]
    Xt = feats[it].astype(np.float64)
    with few_threads():
        if impl == "autograd":
            out = so.svgp_fit_predict_autograd(X, y, Xt, 50, "f64")
        else:
            out = so.svgp_fit_predict_manual(X, y, Xt, 50)
    for a in out:
        a.setflags(write=False)
    return out
