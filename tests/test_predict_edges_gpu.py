"""The six prediction paths at their chunk, tile and size-class edges on the MI355X (cases, generators, references and
the tolerance: predict_edge_cases.py; their preconditions: test_predict_edges_cpu.py).

Part 1: gapro_svgp_predict_batch on hand-made states -- every launch class (M_p <= 64 / 128 / 256 in LDS, a workspace
slice beyond), both feature-width builds in every class, T around the 16- and 32-column tiles, unaligned row and
output offsets.  Part 2: the fit kernels' own tails against the float64 posterior of the state the same fit exported,
T around the tail's column chunk.  Part 3: sides of one point on the strip, staged and cluster routes against the
trained float64 oracle.
"""
import time

import numpy as np
import pytest

import predict_edge_cases as pc
from predict_edge_cases import _check

pytestmark = pytest.mark.gpu


def _worst(devs, what):
    d = np.array(devs).reshape(-1, 3).max(axis=0)
    print("%s: largest deviation var rel %.3e  mu abs %.3e  p abs %.3e" % (what, d[0], d[1], d[2]))


# ---------------------------------------------------------------------------------------------------------------------
# part 1
_MIXED = {}


def _mixed(d):
    """The mixed launch of feature width d, run once per process: (entries, outputs, status, table rows per entry)."""
    if d not in _MIXED:
        from gapro_amd.gaussian_process_utils import predict_gp_batch

        entries = pc.mixed_launch(d)
        models, feats, rows, local = pc.launch_arrays(d, entries)
        t0 = time.perf_counter()
        outs, status = predict_gp_batch(models, feats, rows, return_status=True)
        print("D %d: %d models, %d rows, %.2f s" % (d, len(models), sum(map(len, rows)), time.perf_counter() - t0))
        _MIXED[d] = (entries, outs, status, local)
    return _MIXED[d]


@pytest.mark.parametrize("d", pc.HAND_D)
def test_mixed_launch_against_the_reference(d):
    entries, outs, status, local = _mixed(d)
    assert (status == 0).all()
    devs = []
    for e, out, loc in zip(entries, outs, local):
        assert all(len(o) == e.t for o in out)
        ref = pc.sliced(pc.hand_reference(e.m, d), loc)
        devs.append(pc.deviations(out, ref))
        _check(out, ref, "hand-made M %d D %d T %d" % (e.m, d, e.t))
    _worst(devs, "part 1, D %d" % d)


@pytest.mark.parametrize("d", pc.HAND_D)
def test_a_model_alone_equals_itself_in_the_mixed_launch(d):
    from gapro_amd.gaussian_process_utils import predict_gp_batch

    entries, outs, _, local = _mixed(d)
    for cls in range(4):
        k = max((k for k, e in enumerate(entries) if pc.launch_class(e.m) == cls), key=lambda k: (entries[k].t, k))
        e = entries[k]
        assert e.t == max(pc.HAND_T)
        alone = predict_gp_batch([pc.hand_model(e.m, d)], pc.hand_table(e.m, d)[0], [local[k]])[0]
        for j in range(5):
            assert np.array_equal(alone[j], outs[k][j]), (e, j)


def test_persistent_waves_take_a_second_item():
    """M = 272 at D = 7 with 600 x 32 + 5 rows: 601 column tiles on the 512 persistent waves of the any-width build.  A
    row's result is the row's own: the bits of a launch of the model's table rows taken once, and the reference."""
    from gapro_amd.gaussian_process_utils import predict_gp_batch

    m, d = 272, 7
    model, table = pc.hand_model(m, d), pc.hand_table(m, d)[0]
    rows = np.random.default_rng(5).integers(0, len(table), size=600 * 32 + 5)
    out, st = predict_gp_batch([model], table, [rows], return_status=True)
    once = predict_gp_batch([model], table, [np.arange(len(table))])[0]
    assert st[0] == 0
    for j in range(5):
        assert np.array_equal(out[0][j], once[j][rows]), j
    _check(out[0], pc.sliced(pc.hand_reference(m, d), rows), "M 272 D 7, 601 tiles")


def test_a_model_without_rows_between_two_others():
    from gapro_amd.gaussian_process_utils import predict_gp_batch

    for d, sizes in ((6, (65, 530, 17)), (7, (272, 16, 1040)), (32, (129, 257, 64))):
        entries = [pc.Entry(sizes[0], 33, 5), pc.Entry(sizes[1], 0, 0), pc.Entry(sizes[2], 65, 11)]
        models, feats, rows, local = pc.launch_arrays(d, entries)
        outs, st = predict_gp_batch(models, feats, rows, return_status=True)
        assert (st == 0).all() and all(len(o) == 0 for o in outs[1])
        assert outs[1][0].dtype == np.float32 and outs[1][2].dtype == bool
        two = predict_gp_batch([models[0], models[2]], feats, [rows[0], rows[2]])
        for a, b in ((outs[0], two[0]), (outs[2], two[1])):
            for j in range(5):
                assert np.array_equal(a[j], b[j])
        _check(outs[0], pc.sliced(pc.hand_reference(sizes[0], d), local[0]), "before the empty model")
        _check(outs[2], pc.sliced(pc.hand_reference(sizes[2], d), local[2]), "after the empty model")


# ---------------------------------------------------------------------------------------------------------------------
# part 2
@pytest.mark.parametrize("shape", pc.FIT_SHAPES, ids=pc.FIT_IDS)
def test_fit_tail_against_its_exported_state(shape):
    from gapro_amd import _lib
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch, predict_gp_batch

    lib = _lib.load()
    assert (int(lib.gapro_fit_route(shape.m, shape.d)), int(lib.gapro_fit_padded_m(shape.m, shape.d))) == \
        (shape.route, shape.mp)
    feats, b1, b2, tests = pc.fit_problem(shape)
    ts = pc.fit_ts(shape)
    t0 = time.perf_counter()
    outs, models, status = fit_gp_spp_batch(feats, [(b1, b2, it) for it in tests], training_iter=pc.fit_iters(shape),
                                            return_models=True, return_status=True)
    t_fit = time.perf_counter() - t0
    assert (status == 0).all(), status
    # a fit's training does not depend on its T
    state = models[0].to_state()
    for mo in models[1:]:
        assert np.array_equal(mo.to_state(), state)
    model = models[0]
    trained = float(np.abs(np.tril(model.LS) - np.eye(shape.m)).max())
    assert trained >= pc.LS_TRAINED, trained
    # the reference of every problem of the launch: the float64 posterior of that state at every row of the table
    ref = pc._oracle(model, feats)
    dv, dm = pc.reference_gap(ref, model, feats)
    print("%s M_p %d, %d steps, %d fits in %.2f s: max |tril(L_S) - I| %.3f; reference gap var %.1e mu %.1e"
          % (pc.FIT_IDS[pc.FIT_SHAPES.index(shape)], shape.mp, pc.fit_iters(shape), len(ts), t_fit, trained, dv, dm))
    assert dv <= pc.GAP_BOUND and dm <= pc.GAP_BOUND
    # every problem is compared before the test fails, so that a failure names every T that is wrong
    devs, wrong = [], []
    for path, results in (("fit tail", outs), ("predict kernel", predict_gp_batch(models, feats, list(tests)))):
        for t, it, out in zip(ts, tests, results):
            assert all(len(o) == t for o in out)
            if t == 0:
                assert out[0].dtype == np.float32 and out[2].dtype == bool and out[4].dtype == np.float32
                continue
            devs.append(pc.deviations(out, pc.sliced(ref, it)))
            try:
                _check(out, pc.sliced(ref, it), "%s route %d M_p %d T %d" % (path, shape.route, shape.mp, t))
            except AssertionError as e:
                wrong.append("%s T %d: %s" % (path, t, " ".join(str(e).split())[:200]))
        _worst(devs, "part 2, %s" % path)
        devs = []
    assert not wrong, "\n".join(wrong)


# ---------------------------------------------------------------------------------------------------------------------
# part 3
@pytest.mark.parametrize("case", pc.SIDE_CASES, ids=pc.SIDE_IDS)
def test_one_point_side(case):
    from gapro_amd import _lib
    from gapro_amd.gaussian_process_utils import fit_gp_spp_batch
    from test_fit_gpu import _compare

    assert int(_lib.load().gapro_fit_route(case.m1 + case.m2, case.d)) == case.route
    feats, b1, b2, it = pc.side_problem(case)
    assert len(it) == pc.SIDE_T
    out = fit_gp_spp_batch(feats, [(b1, b2, it)], training_iter=50)[0]
    mu_r, var_r, p_r = ref = pc.side_reference(case)
    print("(%d, %d) D %d route %d: var rel %.3e  mu abs %.3e  p abs %.3e"
          % (case.m1, case.m2, case.d, case.route, np.max(np.abs(out[4] - var_r) / var_r), np.max(np.abs(out[3] - mu_r)),
             np.max(np.abs(out[0] - p_r))))
    _compare(out, ref)
