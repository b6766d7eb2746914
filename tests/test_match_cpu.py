"""The matcher without a GPU: gapro_lsap_solve (host-only) against brute force and SciPy, its refusals, the restatement
tests/match_ref.py against the outputs of the real reference (tests/golden/match_*.npz), and what match_cost,
linear_sum_assignment and hungarian_match export and refuse before a device is touched.
"""
import ctypes as C

import numpy as np
import pytest

import match_ref as ref


def _solve(cost, dup=1):
    from gapro_amd import consumer_ops as ops

    rows, cols = ops.linear_sum_assignment(cost, dup)
    assert ref.check_assignment(cost, rows, cols, dup)
    return rows, cols


SMALL = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 3), (6, 6), (6, 3), (5, 2), (3, 6), (2, 5), (4, 3), (5, 4), (6, 2)]


@pytest.mark.parametrize("dup", [1, 2])
@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "%dx%d" % s)
def test_small_problems_equal_brute_force(shape, dup):
    """rows > cols, rows < cols, dup * cols > rows >= cols (4x3, 5x4, 6x3 at dup 2), negative costs."""
    rng = np.random.default_rng(100 * shape[0] + 10 * shape[1] + dup)
    for trial in range(1 if shape == (6, 6) and dup == 2 else 6):  # 6 x 12: 665 280 maps to enumerate, once
        cost = rng.normal(0, 3, shape).astype(np.float32)
        if trial == 1:
            cost = -np.abs(cost)
        if trial == 2:
            cost = rng.integers(-2, 3, shape).astype(np.float32)  # many equal optima
        rows, cols = _solve(cost, dup)
        assert ref.total(cost, rows, cols) == pytest.approx(ref.brute_force(cost, dup), rel=1e-12, abs=1e-12)
        again = _solve(cost, dup)
        assert np.array_equal(rows, again[0]) and np.array_equal(cols, again[1])


@pytest.mark.parametrize("shape,dup", [((4, 4), 1), ((5, 3), 1), ((3, 5), 1), ((6, 2), 2), ((5, 2), 3), ((1, 1), 1)])
def test_all_equal_matrix_gives_a_valid_assignment_with_the_optimal_total(shape, dup):
    cost = np.full(shape, 2.5, dtype=np.float32)
    rows, cols = _solve(cost, dup)
    assert ref.total(cost, rows, cols) == 2.5 * min(shape[0], dup * shape[1])


def test_strided_rows_and_a_fortran_matrix():
    rng = np.random.default_rng(7)
    wide = rng.normal(size=(9, 14)).astype(np.float32)
    view = wide[:, 2:9]  # row stride 14, unit column stride: handed over as it is
    want = _solve(np.ascontiguousarray(view), 2)
    for form in (view, np.asfortranarray(view), wide[:, 2:9][::-1][::-1]):
        got = _solve(form, 2)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("shape,dup", [((256, 40), 4), ((256, 40), 1), ((40, 256), 1), ((64, 33), 4), ((100, 100), 1),
                                       ((17, 5), 3), ((30, 90), 2)])
def test_random_costs_equal_scipy(shape, dup):
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    rng = np.random.default_rng(shape[0] * 1000 + shape[1] + dup)
    cost = rng.uniform(0.5, 3.0, shape).astype(np.float32)
    rows, cols = _solve(cost, dup)
    wide = np.tile(cost.astype(np.float64), (1, dup))
    r, c = lsa(wide)
    assert ref.total(cost, rows, cols) == pytest.approx(float(wide[r, c].sum()), rel=1e-9)
    assert ref.pairs(rows, cols, shape[1]) == ref.pairs(r, c, shape[1])


def test_a_batch_solved_on_threads_equals_the_problems_solved_one_by_one(monkeypatch):
    from gapro_amd import consumer_ops as ops

    rng = np.random.default_rng(12)
    problems = [(rng.uniform(0, 3, (q, i)).astype(np.float32), dup)
                for q, i, dup in ((64, 9, 1), (64, 9, 4), (20, 33, 1), (20, 33, 4), (64, 17, 1), (64, 17, 4), (1, 1, 1))]
    want = [ops.linear_sum_assignment(c, d) for c, d in problems]
    for threads in (1, 3, ops.MATCH_SOLVER_THREADS):
        monkeypatch.setattr(ops, "MATCH_SOLVER_THREADS", threads)
        got = ops._solve_all(problems)
        assert len(got) == len(want)
        for (r, c), (wr, wc) in zip(got, want):
            assert np.array_equal(r, wr) and np.array_equal(c, wc)
    broken = problems[2][0].copy()
    broken[3, 3] = np.nan
    with pytest.raises(ops.GaproError):
        ops._solve_all(problems[:2] + [(broken, 2)] + problems[3:])


def test_the_solver_refuses_non_finite_entries_and_bad_sizes():
    from gapro_amd import _lib
    from gapro_amd import consumer_ops as ops

    lib = _lib.load()
    cost = np.arange(12, dtype=np.float32).reshape(3, 4)
    rows, cols, n = np.zeros(3, np.int32), np.zeros(3, np.int32), C.c_int32(-1)
    ok = (3, 4, cost.ctypes.data, 4, 1, C.byref(n), rows.ctypes.data, cols.ctypes.data)
    assert lib.gapro_lsap_solve(*ok) == 0 and n.value == 3

    def call(**kw):
        names = ("n_rows", "n_cols", "cost", "ld", "dup", "n_out", "rows", "cols")
        return lib.gapro_lsap_solve(*[kw.get(k, v) for k, v in zip(names, ok)])

    for bad in (dict(n_rows=0), dict(n_cols=0), dict(n_rows=-1), dict(dup=0), dict(ld=3), dict(cost=None),
                dict(n_out=None), dict(rows=None), dict(cols=None), dict(dup=1 << 30)):
        assert call(**bad) == _lib.GAPRO_ERR_BAD_ARG, bad
    for v in (np.nan, np.inf, -np.inf):
        broken = cost.copy()
        broken[2, 1] = v
        assert call(cost=broken.ctypes.data) == _lib.GAPRO_ERR_NOT_FINITE
        with pytest.raises(_lib.GaproError) as e:
            ops.linear_sum_assignment(broken)
        assert e.value.code == _lib.GAPRO_ERR_NOT_FINITE
    # a non-finite value beyond the columns of a strided matrix is not looked at
    wide = np.full((3, 6), np.nan, dtype=np.float32)
    wide[:, :4] = cost
    assert call(cost=wide.ctypes.data, ld=6) == 0
    for bad_cost, dup in ((cost.astype(np.float64), 1), (cost[0], 1), (cost.tolist(), 1), (cost, 0), (cost, 1.5),
                          (cost, True), (cost[:0], 1), (cost[:, :0], 1)):
        with pytest.raises(ValueError):
            ops.linear_sum_assignment(bad_cost, dup)


@pytest.mark.parametrize("name", ref.FIXTURES)
def test_restatement_equals_the_reference_within_ref_dev(name):
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    z, samples = ref.fixture(name)
    ref_dev, dup = float(z["ref_dev"]), int(z["dup_gt"])
    assert 0.0 < ref_dev < 1e-5 and dup == ref.DUP_GT
    worst = 0.0
    for b, s in enumerate(samples):
        if s is None:
            continue
        ours = ref.cost(z["cls_logits"][b], s["mask_logits"], z["conf_logits"][b], z["box_preds"][b], s["mask"], s["cls"],
                        s["box"])
        assert ours.dtype == np.float32 and ours.shape == s["ref_cost"].shape
        worst = max(worst, float(np.abs(ours.astype(np.float64) - s["ref_cost"].astype(np.float64)).max()))
        n_inst = len(s["cls"])
        # the reference's assignments are SciPy's on the once-rounded restatement, and the library's
        for d, r, c in ((1, s["row"], s["col"]), (dup, s["aux_row"], s["aux_col"])):
            assert ref.pairs(*lsa(np.tile(ours, (1, d))), n_inst) == ref.pairs(r, c, n_inst)
            assert ref.pairs(*_solve(ours, d), n_inst) == ref.pairs(r, c, n_inst)
            assert ref.pairs(*_solve(s["ref_cost"], d), n_inst) == ref.pairs(r, c, n_inst)
    assert worst <= ref_dev  # the generator measured it as the largest of these differences


def test_restatement_rules():
    rng = np.random.default_rng(3)
    Q, I, S, Cn = 5, 3, 9, 4
    args = [rng.normal(size=(Q, Cn)).astype(np.float32), rng.normal(size=(Q, S)).astype(np.float32),
            rng.normal(size=Q).astype(np.float32), np.sort(rng.normal(size=(Q, 2, 3)), 1).reshape(Q, 6).astype(np.float32),
            (rng.random((I, S)) < 0.4).astype(np.float32), rng.integers(0, Cn, I), np.sort(rng.normal(size=(I, 2, 3)), 1)
            .reshape(I, 6).astype(np.float32)]
    base = ref.cost(*args)
    # the bce identity: BCE(x, 1) . t + BCE(x, 0) . (1 - t) = sum sp - sum x t
    x, t = args[1].astype(np.float64), args[4].astype(np.float64)
    sp = np.logaddexp(0.0, x)
    direct = ((sp - x) @ t.T + sp @ (1 - t).T) / S
    only_bce = ref.cost64(*args, weights=(0, 0, 1, 0, 0))
    assert np.allclose(only_bce, direct, rtol=1e-13, atol=1e-13)
    # NaN and inf become 100000 in whole rows / columns
    for pos, where in ((1, "row"), (2, "row"), (3, "row"), (6, "col")):
        broken = [a.copy() for a in args]
        broken[pos][1] = np.nan if pos != 2 else np.inf
        got = ref.cost(*broken)
        hit = got[1, :] if where == "row" else got[:, 1]
        assert (hit == 100000.0).all() and (got == 100000.0).sum() == hit.size
        rest = np.ones_like(got, dtype=bool)
        if where == "row":
            rest[1, :] = False
        else:
            rest[:, 1] = False
        assert np.array_equal(got[rest], base[rest])


def test_exports():
    import gapro_amd
    from gapro_amd import _lib, consumer_ops

    for n in ("match_cost", "linear_sum_assignment", "hungarian_match"):
        assert n in gapro_amd.__all__ and getattr(gapro_amd, n) is getattr(consumer_ops, n)
        assert n in gapro_amd._EXPORTS["consumer_ops"]
    lib = _lib.load()
    assert lib.gapro_version() == 200
    for n in ("gapro_match_cost", "gapro_match_cost_workspace_bytes", "gapro_lsap_solve"):
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    assert C.sizeof(_lib.MatchTask) == 56 and C.sizeof(_lib.MatchWeights) == 40
    assert consumer_ops.MATCH_WEIGHTS == ref.WEIGHTS
    assert lib.gapro_match_cost_workspace_bytes(4, 256, 160, 6000) > 0
    for bad in ((0, 256, 160, 6000), (4, 0, 160, 6000), (4, 256, 0, 6000), (4, 256, 160, 0), (1025, 256, 160, 6000)):
        assert lib.gapro_match_cost_workspace_bytes(*bad) == 0


def _cpu_batch(Q=6, Cn=4, shapes=((3, 7), None, (2, 5))):
    import torch

    B = len(shapes)
    g = torch.Generator().manual_seed(0)
    args = [torch.randn(B, Q, Cn, generator=g), [None if s is None else torch.randn(Q, s[1], generator=g) for s in shapes],
            torch.randn(B, Q, generator=g), torch.randn(B, Q, 6, generator=g),
            [None if s is None else {"mask": (torch.rand(s[0], s[1], generator=g) < 0.5).float(),
                                     "cls": torch.randint(0, Cn, (s[0],), generator=g),
                                     "box": torch.randn(s[0], 6, generator=g)} for s in shapes]]
    return args


def _variants():
    """(what, change of the arguments) that must be a ValueError before a device is touched."""
    import torch

    def entry(i, key, fn):
        def change(a):
            a[4][i] = dict(a[4][i])
            a[4][i][key] = fn(a[4][i][key])
        return change

    def at(pos, fn):
        def change(a):
            a[pos] = fn(a[pos])
        return change

    def logits(i, fn):
        def change(a):
            a[1] = list(a[1])
            a[1][i] = fn(a[1][i])
        return change

    return [
        ("cls_logits dtype", at(0, lambda t: t.double())), ("cls_logits rank", at(0, lambda t: t[0])),
        ("cls_logits no tensor", at(0, lambda t: t.numpy())), ("conf shape", at(2, lambda t: t[:, :-1])),
        ("conf dtype", at(2, lambda t: t.half())), ("box_preds shape", at(3, lambda t: t[..., :5])),
        ("box_preds dtype", at(3, lambda t: t.double())), ("mask_logits length", at(1, lambda l: l[:-1])),
        ("mask_logits no list", at(1, lambda l: l[0])), ("dc length", at(4, lambda l: l + [None])),
        ("logits None where a mask is", logits(0, lambda t: None)), ("logits columns", logits(0, lambda t: t[:, :-1])),
        ("logits rows", logits(2, lambda t: t[:-1])), ("logits dtype", logits(2, lambda t: t.double())),
        ("logits rank", logits(0, lambda t: t[None])), ("mask dtype", entry(0, "mask", lambda t: t.bool())),
        ("mask rank", entry(0, "mask", lambda t: t[0])), ("mask empty", entry(0, "mask", lambda t: t[:0])),
        ("cls dtype", entry(0, "cls", lambda t: t.float())), ("cls length", entry(2, "cls", lambda t: t[:-1])),
        ("cls dtypes differ", entry(2, "cls", lambda t: t.int())), ("box shape", entry(0, "box", lambda t: t[:, :5])),
        ("box dtype", entry(2, "box", lambda t: t.double())), ("entry no dict", at(4, lambda l: [l[0], None, 5])),
        ("entry without box", at(4, lambda l: [{"mask": l[0]["mask"], "cls": l[0]["cls"]}, None, l[2]])),
        ("device of a mask", entry(0, "mask", lambda t: t.to("meta"))),
        ("device of the logits", logits(2, lambda t: t.to("meta"))),
        ("device of conf", at(2, lambda t: t.to("meta"))),
    ]


@pytest.mark.parametrize("what,change", _variants(), ids=[w for w, _ in _variants()])
def test_value_errors_before_a_device_is_touched(what, change):
    from gapro_amd import consumer_ops as ops

    for fn in (ops.match_cost, ops.hungarian_match):
        args = _cpu_batch()
        change(args)
        with pytest.raises(ValueError):
            fn(*args)


def test_weights_dup_gt_and_the_all_none_batch():
    from gapro_amd import consumer_ops as ops

    for bad in ((1, 2, 3), (1, 2, 3, 4, -1), (1, 2, 3, 4, float("nan")), (1, 2, 3, 4, float("inf")), "abcde",
                {"class": 1}, {"class": 1, "dice": 1, "bce": 1, "conf": 1, "giou": 1, "more": 1}, 3.0):
        with pytest.raises(ValueError):
            ops.match_cost(*_cpu_batch(), weights=bad)
    for bad in (0, -1, 1.0, True, None):
        with pytest.raises(ValueError):
            ops.hungarian_match(*_cpu_batch(), dup_gt=bad)
    # host tensors that pass every check: there is no CPU path
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.match_cost(*_cpu_batch())
    # a batch without instances returns without looking for a device
    args = _cpu_batch(shapes=(None, None))
    assert ops.match_cost(*args) == [None, None]
    gt, aux = ops.hungarian_match(*args, dup_gt=3)
    for d in (gt, aux):
        assert sorted(d) == ["box_labels", "cls_labels", "inst_labels", "row_indices"]
        assert all(v == [None, None] for v in d.values())
