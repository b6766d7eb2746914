"""The case tables of predict_edge_cases.py exercise what test_predict_edges_gpu.py claims, and their float64
references are reproducible far inside the float32 half-ulp the kernels are held to.  Oracle and host code only.

Conditions, not tolerances: a case that misses one gets another seed (predict_edge_cases.RESEED, SideCase.seed).
"""
import numpy as np
import pytest

import predict_edge_cases as pc

HAND = [(m, d) for d in pc.HAND_D for m in pc.hand_sizes(d)]


@pytest.mark.parametrize("m,d", HAND, ids=["m%d_d%d" % md for md in HAND])
def test_hand_made_state_preconditions(m, d):
    model = pc.hand_model(m, d)
    rows, kind = pc.hand_table(m, d)
    ref = pc.hand_reference(m, d)
    mu, var, p = ref
    assert rows.dtype == np.float32 and len(rows) == pc.N_ORDINARY + min(m, pc.N_NEAR) + pc.N_FAR
    assert model.status == 0 and model.jitter == 1e-4 and np.array_equal(model.LS, np.tril(model.LS))
    assert abs(model.lengthscale - np.sqrt(d) * pc.std_of(d)) < 1e-12
    # part 0: the reference against an evaluation by an explicit inverse
    dv, dm = pc.reference_gap(ref, model, rows)
    Li = pc.inv_l(model)
    share = pc.offdiag_share(Li) if m > 16 else 0.0
    ties = float((np.abs(p - 0.5) <= 1e-6).mean())
    print("M %d D %d: gap var %.1e mu %.1e; var min %.3f; |p - 0.5| min %.1e; off-diagonal share of inv(L) %.0f %%"
          % (m, d, dv, dm, var.min(), np.abs(p - 0.5).min(), 100 * share))
    assert dv <= pc.GAP_BOUND and dm <= pc.GAP_BOUND
    assert var.min() >= 0.08  # far above the min_variance clamp, and no cancellation in s + jitter + sum (B^2 - A^2)
    assert ties == 0.0  # (_check would allow 0.1 %)
    if m >= 17:
        assert share >= 0.05  # K_ZZ is dense: an error in an off-diagonal tile of L^-1 is not hidden below the tolerance
        blk = np.arange(m) // 16
        off = np.abs(np.tril(model.LS))[blk[:, None] != blk[None, :]]
        assert off.max() > 0.01
    # at six times the scale k(Z, x) vanishes for many rows (not for all: a short draw stays near): there the
    # variance is the prior's within a float32 half-ulp
    if d >= 6:
        prior = model.outputscale + model.jitter
        far = var[kind == 2]
        assert (np.abs(far - prior) <= 2.0 ** -25 * prior).sum() >= pc.N_FAR // 4
    # the shifted inducing points are where the posterior differs most from the prior
    assert np.abs(var[kind == 1] - (model.outputscale + model.jitter)).max() > 1e-3


@pytest.mark.parametrize("d", pc.HAND_D)
def test_mixed_launch_covers_every_t_in_every_class(d):
    entries = pc.mixed_launch(d)
    assert {e.m for e in entries} == set(pc.hand_sizes(d))
    for cls in range(4):
        assert {e.t for e in entries if pc.launch_class(e.m) == cls} == set(pc.HAND_T), cls
    models, feats, rows, local = pc.launch_arrays(d, entries)
    assert len(models) == len(entries) == len(rows) and feats.shape[1] == d
    offs = np.cumsum([0] + [len(r) for r in rows])[:-1]
    assert (offs % 16 != 0).sum() > len(offs) // 2 and (offs % 32 != 0).sum() > len(offs) // 2
    for e, mo, r, loc in zip(entries, models, rows, local):
        assert mo is pc.hand_model(e.m, d) and len(r) == e.t
        assert np.array_equal(feats[r], pc.hand_table(e.m, d)[0][loc])
    # the row vector holds repeats, and every kind of row
    vec = pc.hand_row_vector(17, d)
    assert len(vec) == max(pc.HAND_T) and len(np.unique(vec)) < len(vec)
    assert set(pc.hand_table(17, d)[1][vec]) == {0, 1, 2}
    # the launch classes are the library's: M_p <= 64, <= 128, <= 256, beyond
    assert [pc.launch_class(m) for m in (1, 64, 65, 128, 129, 256, 257, 1040)] == [0, 0, 1, 1, 2, 2, 3, 3]
    if d in (7, 32):
        assert {272, 530, 1040} <= {e.m for e in entries}  # any feature width on a workspace slice


@pytest.mark.parametrize("shape", pc.FIT_SHAPES, ids=pc.FIT_IDS)
def test_fit_shape_runs_on_the_route_it_names(shape):
    from gapro_amd import _lib

    lib = _lib.load()
    assert (int(lib.gapro_fit_route(shape.m, shape.d)), int(lib.gapro_fit_padded_m(shape.m, shape.d))) == \
        (shape.route, shape.mp)
    w = pc.chunk_width(shape)
    ts = pc.fit_ts(shape)
    assert {0, 1, w - 1, w, w + 1, 2 * w + 17} <= set(ts)
    feats, b1, b2, tests = pc.fit_problem(shape)
    assert len(b1) == shape.m // 2 - 3 and len(b1) + len(b2) == shape.m and [len(t) for t in tests] == list(ts)
    assert feats.shape[1] == shape.d and all(t.max() < len(feats) for t in tests if len(t))
    both = np.concatenate(tests)  # ordinary rows, training rows and far rows, and repeats
    assert (both < shape.m).any() and (both >= len(feats) - pc.N_FAR).any() and (both >= shape.m).any()
    longest = tests[0]
    assert len(longest) == 2 * w + 17 and (len(np.unique(longest)) < len(longest) or len(longest) < 100)
    # launch order: see fit_ts -- whatever a tail writes up to the next multiple of W stays inside the launch's outputs
    total, off = sum(ts), np.cumsum((0,) + ts)
    assert ts[-1] == w and all(off[k] + -(-t // w) * w <= total for k, t in enumerate(ts))
    assert 10 <= pc.fit_iters(shape) <= 50


def test_fit_shapes_cover_every_route_and_product_form():
    assert {s.route for s in pc.FIT_SHAPES} == {0, 1, 2, 3, 4, 5}
    assert {s.mp for s in pc.FIT_SHAPES if s.route == 1 and s.d == 6} == {144, 256, 272, 320, 384, 480}
    assert {s.mp // 128 for s in pc.FIT_SHAPES if s.route == 4 and s.d == 6} == {4, 5}


@pytest.mark.parametrize("case", pc.SIDE_CASES, ids=pc.SIDE_IDS)
def test_one_point_sides_have_a_reproducible_reference(case):
    """The trained float64 reference of the one-point-side cases: torch autograd and the NumPy restatement agree on
    (mu, var, p) within 1 % of the tolerances the kernels are compared at; SideCase.gap is what they give."""
    from gapro_amd import _lib

    assert int(_lib.load().gapro_fit_route(case.m1 + case.m2, case.d)) == case.route
    mu_a, var_a, p_a = pc.side_reference(case)
    mu_m, var_m, p_m = pc.side_reference(case, "manual")
    gap = (float(np.max(np.abs(var_m - var_a) / var_a)), float(np.max(np.abs(mu_m - mu_a))),
           float(np.max(np.abs(p_m - p_a))))
    print("(%d, %d) D %d: the two oracles differ by var %.1e  mu %.1e  p %.1e" % ((case.m1, case.m2, case.d) + gap))
    tol = pc.COMPARE_TOL
    np.testing.assert_allclose(var_m, var_a, rtol=0.01 * tol["var_rtol"], atol=0)
    np.testing.assert_allclose(mu_m, mu_a, rtol=0.01 * tol["mu_rtol"], atol=0.01 * tol["mu_atol"])
    np.testing.assert_allclose(p_m, p_a, rtol=0, atol=0.01 * tol["p_atol"])
    # the table is what was measured: not smaller than a fresh measurement by more than the factor ten by which
    # another BLAS or thread count moves last-bit differences (floor: a hundredth of the bounds above)
    for g, t in zip(gap, case.gap):
        assert g <= max(10.0 * t, 1e-11), (gap, case.gap)
    assert (np.abs(p_a - 0.5) <= 1e-6).mean() <= 1e-3


def test_compare_tolerances_are_those_of_the_fit_tests():
    import test_fit_gpu as tf

    assert (tf.VAR_RTOL, tf.MU_ATOL) == (pc.COMPARE_TOL["var_rtol"], pc.COMPARE_TOL["mu_atol"])
