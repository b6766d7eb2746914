"""The case table of the fit-option tests (test_fit_options_cpu.py / test_fit_options_gpu.py) and what both share: one
problem per kernel route and feature width, the float64 references at given options (computed once per process), and
the NumPy figures the per-fit outputs are compared with.

A case is the smallest shape of its route (gapro_fit_route): 5 wave-per-fit, 3 small-fit strip, 0 512-thread strip,
1 LDS-staged, 2 generic (debug bit 8 of gapro_fit_options.reserved), 4 cluster on one workgroup and on four.  The seed
and the clamp value ``v`` of a case are chosen so that test_fit_options_cpu.py's preconditions hold: at min_variance = v
the clamp is active during training and at prediction, and no variance of the float64 trajectory comes so close to v
that two correct implementations could decide the branch differently.

``D_REF`` is the largest absolute difference between the two oracle implementations (torch autograd and the NumPy
restatement with the hand-derived backward) in every field of the trained state at the default options, measured by
test_fit_options_cpu.py::test_d_ref_table_is_what_the_two_oracles_give; the GPU test allows a route
max(1e-8, 100 x d_ref) in that field.
"""
import contextlib
from collections import namedtuple
from functools import lru_cache

import numpy as np

ITERS = 50
FLAG_NO_CLUSTER = 8
STATE_FIELDS = ("Z", "mean", "LS", "c", "rho_s", "rho_l")
LR_JITTER = ((0.03, 1e-4), (0.1, 1e-6), (0.1, 1e-2))  # (lr, jitter): a slower Adam; gpytorch's float64 jitter; a large one

Case = namedtuple("Case", "name route flags m1 m2 t d seed v")

CASES = (
    Case("wave_d6", 5, 0, 20, 28, 33, 6, 27, 0.5),
    Case("small_d6", 3, 0, 31, 33, 40, 6, 38, 0.5),
    Case("strip_d6", 0, 0, 40, 50, 33, 6, 47, 0.5),
    Case("staged_d6", 1, 0, 70, 80, 40, 6, 77, 0.5),
    Case("cluster4_d6", 4, 0, 250, 262, 30, 6, 290, 0.5),
    Case("wave_d32", 5, 0, 10, 12, 20, 32, 132, 0.6),
    Case("small_d32", 3, 0, 20, 28, 12, 32, 90, 0.5),
    Case("strip_d32", 0, 0, 40, 50, 33, 32, 110, 0.5),
    Case("staged_d32", 1, 0, 90, 100, 40, 32, 160, 0.5),
    Case("generic_d32", 2, FLAG_NO_CLUSTER, 120, 136, 25, 32, 190, 0.5),
    Case("cluster1_d32", 4, 0, 120, 136, 25, 32, 190, 0.5),
)
BY_NAME = {c.name: c for c in CASES}
IDS = [c.name for c in CASES]

# name -> field -> max |autograd - manual| of the trained state, default options, 50 steps (see the module docstring)
D_REF = {
    "wave_d6": dict(Z=8.1e-12, mean=7.3e-13, LS=6.1e-13, c=3.7e-14, rho_s=1.9e-13, rho_l=1.8e-14),
    "small_d6": dict(Z=1.2e-11, mean=3.7e-13, LS=2.3e-13, c=1.8e-13, rho_s=4.0e-14, rho_l=2.9e-14),
    "strip_d6": dict(Z=1.9e-12, mean=7.9e-14, LS=9.9e-14, c=1.3e-15, rho_s=2.1e-15, rho_l=6.7e-15),
    "staged_d6": dict(Z=1.4e-10, mean=1.9e-12, LS=7.1e-13, c=1.0e-13, rho_s=1.2e-14, rho_l=7.3e-14),
    "cluster4_d6": dict(Z=3.5e-10, mean=2.4e-11, LS=2.4e-11, c=1.0e-12, rho_s=1.7e-13, rho_l=2.6e-13),
    "wave_d32": dict(Z=4.6e-13, mean=6.0e-14, LS=2.3e-14, c=3.9e-15, rho_s=5.3e-14, rho_l=2.0e-14),
    "small_d32": dict(Z=9.7e-13, mean=1.2e-13, LS=1.4e-13, c=8.4e-15, rho_s=3.0e-14, rho_l=3.3e-14),
    "strip_d32": dict(Z=1.2e-12, mean=3.0e-13, LS=1.7e-13, c=7.0e-15, rho_s=4.2e-15, rho_l=6.4e-15),
    "staged_d32": dict(Z=3.9e-12, mean=3.2e-13, LS=3.6e-13, c=2.6e-15, rho_s=2.7e-15, rho_l=2.6e-14),
    "generic_d32": dict(Z=3.5e-12, mean=4.1e-13, LS=1.8e-13, c=4.7e-14, rho_s=3.1e-15, rho_l=4.4e-16),
    "cluster1_d32": dict(Z=3.5e-12, mean=4.1e-13, LS=1.8e-13, c=4.7e-14, rho_s=3.1e-15, rho_l=4.4e-16),
}


def std_of(d):
    return 0.3 if d > 8 else 1.0  # d = 32 at unit std is driven by rounding noise (synth.make_gp_problem)


@lru_cache(maxsize=None)
def problem(case):
    """(feats f32[S, D], b1, b2, it) of a case.  At D = 32 the blobs' own test rows are rarely clamped, so the first
    eight training rows of each side are tested as well."""
    from gapro_amd.synth import make_gp_problem

    feats, b1, b2, it = make_gp_problem(case.seed, case.m1, case.m2, case.t, case.d, std=std_of(case.d))
    if case.d > 8:
        it = np.concatenate([it, b1[:8], b2[:8]])
    return feats, b1, b2, it


def xy(case):
    feats, b1, b2, it = problem(case)
    X = np.concatenate([feats[b1], feats[b2]]).astype(np.float64)
    y = np.r_[-np.ones(len(b1)), np.ones(len(b2))]
    return X, y, feats[it].astype(np.float64)


@contextlib.contextmanager
def few_threads(n=4):
    """The oracle's matrices are small (M <= 512): with one BLAS thread per core of a large machine a fit spends its
    time waking threads, ten times what four threads need.  Speed only; without threadpoolctl nothing is limited."""
    import torch

    old = torch.get_num_threads()
    torch.set_num_threads(min(n, old))
    try:
        try:
            from threadpoolctl import threadpool_limits
        except ImportError:
            yield
        else:
            with threadpool_limits(limits=n):
                yield
    finally:
        torch.set_num_threads(old)


def _problem_key(case):
    return (case.m1, case.m2, case.t, case.d, case.seed)


@lru_cache(maxsize=None)
def _reference(key, lr, jitter, min_variance, impl, iters):
    from oracle import svgp_oracle as so

    case = next(c for c in CASES if _problem_key(c) == key)
    X, y, Xt = xy(case)
    if impl == "autograd":
        with few_threads():
            out, st = so.svgp_fit_predict_autograd(X, y, Xt, iters, "f64", jitter=jitter, lr=lr, return_trace=True,
                                                   min_variance=min_variance)
        st = dict(st, mean=st["m"])
    else:
        with few_threads():
            out, st = so.svgp_fit_predict_manual(X, y, Xt, iters, jitter=jitter, lr=lr, return_trace=True,
                                                 min_variance=min_variance)
        st = dict(st, mean=st["m"], c=float(st["c"]), rho_s=float(st["rho_s"]), rho_l=float(st["rho_l"]))
    st["LS"] = np.tril(st["LS"])
    for a in out + (st["Z"], st["mean"], st["LS"]):
        a.setflags(write=False)  # shared among the tests of a process
    return out, st


def reference(case, lr=0.1, jitter=1e-4, min_variance=1e-6, impl="autograd", iters=ITERS):
    """((mu, var, p) float64 at the case's test rows, trained state with the loss trace) of the float64 oracle at the
    given options; two cases on one problem share it."""
    return _reference(_problem_key(case), float(lr), float(jitter), float(min_variance), impl, int(iters))


def state_deviation(a, b):
    """max |a - b| per field of two trained states (dicts, or a GPModel on either side)."""
    get = lambda s, k: np.asarray(s[k] if isinstance(s, dict) else getattr(s, k), dtype=np.float64)  # noqa: E731
    return {k: float(np.max(np.abs(np.tril(get(a, k)) - np.tril(get(b, k))))) if k == "LS"
            else float(np.max(np.abs(get(a, k) - get(b, k)))) for k in STATE_FIELDS}


def state_bound(case, field):
    return max(1e-8, 100.0 * D_REF[case.name][field])


def kzz(Z, rho_s, rho_l):
    """K(Z, Z) of the scaled RBF kernel, float64, without jitter."""
    s = np.log1p(np.exp(-abs(rho_s))) + max(rho_s, 0.0)
    ell = np.log1p(np.exp(-abs(rho_l))) + max(rho_l, 0.0)
    Z = np.asarray(Z, dtype=np.float64)
    return s * np.exp(-0.5 * ((Z[:, None, :] - Z[None, :, :]) ** 2).sum(-1) / (ell * ell))


def cond_figure(K, added):
    """The library's per-fit conditioning figure, (max L_jj / min L_jj)^2 of the Cholesky factor of K + added I."""
    d = np.diagonal(np.linalg.cholesky(K + added * np.eye(len(K))))
    return float((d.max() / d.min()) ** 2)


def raw_variances(state, Xt, jitter=1e-4):
    """The unclamped predictive variances of a trained state at Xt (float64)."""
    from oracle import svgp_oracle as so

    return so.svgp_predict(np.asarray(Xt, dtype=np.float64), state["Z"], state["mean"], state["LS"], state["c"],
                           state["rho_s"], state["rho_l"], jitter=jitter, min_variance=-np.inf)[1]
