"""The fit launcher's device-free parts (gapro_amd/fit_runner.py): the result layouts and the FLOP accounting."""
import numpy as np

from gapro_amd import _lib
from gapro_amd.fit_runner import (FIT_FIELDS, ROUTE_CLASS, ROW_FIELDS, block_bytes, block_views, fit_flops,
                                  fit_flops_by_class)

SIZES = (10, 40, 60, 100, 200, 400, 600)
D, ITERS = 6, 50


def _descs(sizes, t=32):
    descs = (_lib.FitDesc * len(sizes))()
    for d, m in zip(descs, sizes):
        d.m1, d.m2, d.t = m // 2, m - m // 2, t
    return descs


def _offset(view, buf):
    return view.__array_interface__["data"][0] - buf.__array_interface__["data"][0]


def test_result_blocks_are_structs_of_arrays_at_fixed_offsets():
    for n_arg in (0, 1, 7):
        n = max(n_arg, 1)  # an empty launch is laid out like one of a single entry
        assert block_bytes(ROW_FIELDS, n_arg) == 17 * n and block_bytes(FIT_FIELDS, n_arg) == 20 * n
        buf = np.zeros(64 + 20 * n, dtype=np.uint8)  # longer than the block, like the pinned staging buffers
        rows = block_views(ROW_FIELDS, buf, n_arg)
        assert list(rows) == ["probs", "probs_new", "mu", "var", "labels"]
        assert [v.dtype for v in rows.values()] == [np.float32] * 4 + [np.uint8]
        assert [len(v) for v in rows.values()] == [n] * 5
        assert [_offset(v, buf) for v in rows.values()] == [0, 4 * n, 8 * n, 12 * n, 16 * n]
        fits = block_views(FIT_FIELDS, buf, n_arg)
        assert list(fits) == ["loss", "cond", "status"]
        assert [v.dtype for v in fits.values()] == [np.float64, np.float64, np.int32]
        assert [len(v) for v in fits.values()] == [n] * 3
        assert [_offset(v, buf) for v in fits.values()] == [0, 8 * n, 16 * n]
        rows["labels"][:] = 7  # views, not copies
        assert buf[16 * n:17 * n].tolist() == [7] * n


def test_flops_are_booked_under_the_kernel_the_library_routes_to():
    lib = _lib.load()
    descs = _descs(SIZES)
    total = fit_flops(descs, len(SIZES), D, ITERS)
    for flags in (0, _lib.FIT_DBG_NO_CLUSTER | _lib.FIT_DBG_CLUSTER_ALL, _lib.FIT_DBG_NO_WAVE, _lib.FIT_DBG_NO_STRIP):
        per = fit_flops_by_class(descs, len(SIZES), D, ITERS, flags)
        assert sorted(per) == ["cluster", "small", "staged", "strip", "wave"]
        assert abs(sum(per.values()) - total) <= 1e-12 * total
        for m in SIZES:  # every size alone lands in the class of its route, whole
            one = _descs([m])
            route = lib.gapro_fit_route_flags(m, D, flags) if flags else lib.gapro_fit_route(m, D)
            got = fit_flops_by_class(one, 1, D, ITERS, flags)
            assert got[ROUTE_CLASS[route]] == fit_flops(one, 1, D, ITERS) > 0, (m, flags, route)
            assert sum(v > 0 for v in got.values()) == 1
    # NO_CLUSTER | CLUSTER_ALL: the strip and small-fit kernels keep their fits; nothing of theirs is "staged"
    flags = _lib.FIT_DBG_NO_CLUSTER | _lib.FIT_DBG_CLUSTER_ALL
    kept = [m for m in SIZES if lib.gapro_fit_route_flags(m, D, flags) in (0, 3)]
    assert kept, "the fixed sizes include strip / small-fit fits"
    per = fit_flops_by_class(descs, len(SIZES), D, ITERS, flags)
    staged = [m for m in SIZES if lib.gapro_fit_route_flags(m, D, flags) in (1, 2)]
    assert per["staged"] == fit_flops(_descs(staged), len(staged), D, ITERS)
    want = fit_flops(_descs(kept), len(kept), D, ITERS)
    assert want > 0 and abs(per["strip"] + per["small"] - want) <= 1e-12 * want
    assert fit_flops_by_class(descs, 0, D, ITERS) == dict.fromkeys(per, 0.0)
