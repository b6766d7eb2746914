"""The launch structure of the batched GP fit: gapro_fit_launch_plan, the planner gapro_svgp_fit_batch itself calls.

A fit's result is the same bits whatever launch it travels in, so no test of results can see which kernel build a fit
gets, on which stream, with which grid and LDS size, from which ticket counter and behind which gate; only scenes/s can.
Here every field of every step and the upload order are asserted.  No device is needed.

The expected tables below were written by hand from the launch function as it stood before the planner was split out
of it (its FitGroup table, its staged split at M_p > 256 and at 72 KiB, `one_per_cu`, `grid_of`, the gate, the wave
grids) and from the LDS formulas of fit_wg.h / fit_strip.h / common.h -- not by printing what the planner returns.  The
LDS figures, D = 6 (doubles, times 8):
  strip, 512 threads, M_p = 112:  2 D M_p 1344 + 3 M_p 34 = 11424 + 3 NT 1536 + M_p 112 + 4 SW 128 + 32 + 8 M_p 896
                                  = 15472 -> 123776 B;  M_p = 128: 1536 + 13056 + 1536 + 128 + 128 + 32 + 1024 = 17440
                                  -> 139520 B
  small, 256 threads, M_p = 64:   768 + 3 * 64 * 34 = 6528 + 768 + 64 + 128 + 32 + 512 = 8800 -> 70400 B
  staged, M_p = 208:              2496 + Cholesky block column 208 * 17 + 1088 = 4624 -> 56960 B (fits a CU twice)
  staged, M_p = 304:              3648 + 304 * 17 + 1088 = 6256 -> 79232 B
  staged, D = 32, M_p = 144:      9216 + operand ring 4608 -> 110592 B (beyond 72 KiB = 73728 B)
Every case first confirms the routes it relies on with gapro_fit_route_flags.
"""
import ctypes as C

import numpy as np
import pytest

from gapro_amd import _lib

STRIP, STAGED, GENERIC, SMALL, CLUSTER, WAVE = 0, 1, 2, 3, 4, 5  # gapro_fit_route codes = FitLaunchStep.kernel
COPY_FREE = _lib.FIT_STEP_COPY_FREE
FIELDS = ("kernel", "variant", "first", "count", "grid", "stream", "ticket", "timing", "wait_gate", "lds_bytes")

# one fit per route at D = 6: wave M_p = 16 / 32 / 48, small, strip, staged two per CU, staged M_p > 256, cluster
ROUTE_M = (10, 20, 40, 60, 100, 200, 300, 600)
ROUTE_OF = {10: WAVE, 20: WAVE, 40: WAVE, 60: SMALL, 100: STRIP, 200: STAGED, 300: STAGED, 600: CLUSTER}


def plan(ms, d=6, flags=0, n_cu=256, max_steps=_lib.FIT_MAX_STEPS, m1=None):
    """(rc, [step tuples in FIELDS order], upload order) of a batch of fits of ms inducing points."""
    lib = _lib.load()
    descs = (_lib.FitDesc * len(ms))()
    for i, m in enumerate(ms):
        descs[i].m1 = m // 2 if m1 is None else m1
        descs[i].m2 = m - descs[i].m1
        descs[i].t = 3 + i
    steps = (_lib.FitLaunchStep * _lib.FIT_MAX_STEPS)()
    n, order = C.c_int32(-1), (C.c_int32 * len(ms))()
    rc = lib.gapro_fit_launch_plan(C.cast(descs, C.c_void_p), len(ms), d, flags, n_cu, steps, max_steps, C.byref(n),
                                   order)
    if rc != 0:
        return rc, None, None
    assert all(steps[k].reserved == 0 for k in range(n.value))
    return rc, [tuple(getattr(steps[k], f) for f in FIELDS) for k in range(n.value)], list(order)


def routes(ms, d=6, flags=0):
    lib = _lib.load()
    return [lib.gapro_fit_route_flags(m, d, flags) for m in ms]


def expect(ms, steps, order, **kw):
    rc, got, got_order = plan(ms, **kw)
    assert rc == 0
    assert got_order == order
    assert len(got) == len(steps)
    for g, s in zip(got, steps):
        assert dict(zip(FIELDS, g)) == dict(zip(FIELDS, s))


#                kernel, variant, first, count, grid, stream, ticket, timing, wait_gate, lds_bytes
EIGHT = [(CLUSTER, 0, 4, 1, 0, 3, 5, 3, 0, 0),
         (STAGED, 2, 0, 1, 2, 0, 0, 0, 0, 79232),               # M_p = 304: <2, false>
         (STAGED, 2 | COPY_FREE, 1, 1, 2, 4, 2, 0, 1, 56960),   # two-per-CU class; one fit: the <2> build
         (STRIP, 0, 2, 1, 2, 1, 3, 1, 0, 123776),
         (SMALL, 0, 3, 1, 2, 2, 4, 2, 1, 70400),
         (WAVE, 3, 5, 1, 1, 5, 10, 4, 0, 0),
         (WAVE, 2, 6, 1, 1, 6, 9, 4, 0, 0),
         (WAVE, 1, 7, 1, 1, 7, 8, 4, 0, 0)]


def test_one_fit_per_route():
    assert routes(ROUTE_M) == [ROUTE_OF[m] for m in ROUTE_M]
    assert [_lib.load().gapro_fit_padded_m(m, 6) for m in ROUTE_M] == [16, 32, 48, 64, 112, 208, 304, 608]
    expect(ROUTE_M, EIGHT, [6, 5, 4, 3, 7, 2, 1, 0])
    assert [s[5] for s in EIGHT] == [3, 0, 4, 1, 2, 5, 6, 7]
    assert [s[6] for s in EIGHT] == [5, 0, 2, 3, 4, 10, 9, 8]
    assert [s[8] for s in EIGHT] == [0, 0, 1, 0, 1, 0, 0, 0]


def test_without_a_cluster_fit_nothing_waits_behind_a_gate():
    ms = ROUTE_M[:-1]
    assert CLUSTER not in routes(ms)
    steps = [(STAGED, 2, 0, 1, 2, 0, 0, 0, 0, 79232),
             (STAGED, 2 | COPY_FREE, 1, 1, 2, 4, 2, 0, 0, 56960),
             (STRIP, 0, 2, 1, 2, 1, 3, 1, 0, 123776),
             (SMALL, 0, 3, 1, 2, 2, 4, 2, 0, 70400),
             (WAVE, 3, 4, 1, 1, 5, 10, 4, 0, 0),
             (WAVE, 2, 5, 1, 1, 6, 9, 4, 0, 0),
             (WAVE, 1, 6, 1, 1, 7, 8, 4, 0, 0)]
    expect(ms, steps, [6, 5, 4, 3, 2, 1, 0])


def test_the_two_per_cu_staged_step_alone_stays_on_the_staged_stream():
    ms = ROUTE_M[:-2]
    assert routes(ms).count(STAGED) == 1
    steps = [(STAGED, 2 | COPY_FREE, 0, 1, 2, 0, 2, 0, 0, 56960),
             (STRIP, 0, 1, 1, 2, 1, 3, 1, 0, 123776),
             (SMALL, 0, 2, 1, 2, 2, 4, 2, 0, 70400),
             (WAVE, 3, 3, 1, 1, 5, 10, 4, 0, 0),
             (WAVE, 2, 4, 1, 1, 6, 9, 4, 0, 0),
             (WAVE, 1, 5, 1, 1, 7, 8, 4, 0, 0)]
    expect(ms, steps, [5, 4, 3, 2, 1, 0])


@pytest.mark.parametrize("n_cu,wps", [(1, 4), (2, 2), (3, 2)])
def test_two_workgroups_per_cu_only_with_more_fits_than_cus(n_cu, wps):
    assert routes([200, 200]) == [STAGED, STAGED]
    expect([200, 200], [(STAGED, wps | COPY_FREE, 0, 2, 4, 0, 2, 0, 0, 56960)], [0, 1], n_cu=n_cu)


def test_wide_features_beyond_72_kib_are_the_middle_staged_step():
    assert routes([140], d=32) == [STAGED] and _lib.load().gapro_fit_padded_m(140, 32) == 144
    expect([140], [(STAGED, 2 | COPY_FREE, 0, 1, 2, 0, 1, 0, 0, 110592)], [0], d=32)


def _shuffled_strip():
    ms = [int(m) for m in np.random.default_rng(5).permutation(np.arange(100, 124))]
    assert ms != sorted(ms) and ms != sorted(ms, reverse=True)
    assert routes(ms) == [STRIP] * 24 and routes(ms, flags=_lib.FIT_DBG_STATIC_MAP) == [STRIP] * 24
    return ms, [ms.index(m) for m in range(123, 99, -1)]  # longest first


def test_strip_fits_with_tickets_longest_first_on_twice_the_grid():
    ms, desc = _shuffled_strip()
    expect(ms, [(STRIP, 0, 0, 24, 48, 1, 3, 1, 0, 139520)], desc)


def test_strip_fits_without_tickets_serpentine_on_one_workgroup_per_fit():
    ms, desc = _shuffled_strip()
    order = desc[:8] + desc[8:16][::-1] + desc[16:]
    expect(ms, [(STRIP, 0, 0, 24, 24, 1, -1, 1, 0, 139520)], order, flags=_lib.FIT_DBG_STATIC_MAP)


def test_caller_stream_puts_every_step_on_the_callers_stream_and_gates_nothing():
    flags = _lib.FIT_DBG_CALLER_STREAM
    assert routes(ROUTE_M, flags=flags) == [ROUTE_OF[m] for m in ROUTE_M]
    steps = [s[:5] + (-1,) + s[6:8] + (0,) + s[9:] for s in EIGHT]
    expect(ROUTE_M, steps, [6, 5, 4, 3, 7, 2, 1, 0], flags=flags)


def test_no_cluster_sends_a_large_fit_to_the_generic_kernel_without_a_ticket():
    flags = _lib.FIT_DBG_NO_CLUSTER
    assert routes([600], flags=flags) == [GENERIC]
    expect([600], [(GENERIC, 0, 0, 1, 1, 0, -1, 0, 0, 0)], [0], flags=flags)


def test_equal_sizes_keep_their_input_order():
    ms = [100, 110, 100, 110, 100]
    assert routes(ms) == [STRIP] * 5
    expect(ms, [(STRIP, 0, 0, 5, 10, 1, 3, 1, 0, 123776)], [1, 3, 0, 2, 4])


def test_refusals():
    bad_arg = -1
    assert _lib.load().gapro_fit_route_flags(100, 6, 32) == bad_arg
    assert plan(ROUTE_M, flags=32)[0] == bad_arg          # a bit outside GAPRO_FIT_DBG_ALL
    assert plan([100, 200], m1=0)[0] == bad_arg           # an empty side
    assert plan(ROUTE_M, max_steps=7)[0] == bad_arg       # eight steps
    assert plan(ROUTE_M, max_steps=8)[0] == 0
