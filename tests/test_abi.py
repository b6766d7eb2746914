"""The C-ABI library loads (no GPU needed) and exports every symbol include/gapro_hip.h declares."""
import ctypes as C
import os
import re

from gapro_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols(header="gapro_hip.h"):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gapro_[a-z0-9_]+)\s*\(", text)))


def test_library_loads_and_exports_every_declared_symbol():
    lib = _lib.load()
    names = _declared_symbols()
    assert len(names) >= 18
    for n in names:
        assert hasattr(lib, n), "missing export " + n
        assert n in _lib.SIGNATURES, "binding lacks " + n
    assert lib.gapro_version() == 200


def test_debug_entry_points_live_in_their_own_library_and_header():
    """VERDICT r03 (housekeeping): the measurement / self-test entry points are not part of the product library nor of
    its public header; libgapro_hip_debug.so exports exactly what include/gapro_hip_debug.h declares."""
    assert not [n for n in _declared_symbols() if n.startswith("gapro_debug_")]
    lib = _lib.load()
    names = _declared_symbols("gapro_hip_debug.h")
    assert len(names) == 9 and all(n.startswith("gapro_debug_") for n in names), names
    dbg = _lib.load_debug()
    for n in names:
        assert hasattr(dbg, n) and n in _lib.DEBUG_SIGNATURES and not hasattr(lib, n), n
    assert not [n for n in _lib.SIGNATURES if n.startswith("gapro_debug_")]


def test_struct_layouts_match_the_header():
    # sizes follow the C declarations (natural alignment)
    assert C.sizeof(_lib.SceneHeader) == 3 * 8 + 3 * 8 + 8 + 8 + 4 + 4 + 4 + 4
    assert C.sizeof(_lib.FitDesc) == 8 * 4 + 3 * 8
    assert C.sizeof(_lib.FitOptions) == 56  # i32 pad | lr, jitter, min_variance f64 | 4 x i32 | psd_jitter f64
    assert C.sizeof(_lib.SceneTask) == 176
    assert C.sizeof(_lib.ScheduleCounts) == 4 + 4 + 8 + 8 + 8 + 4 + 4


def test_fit_options_default_and_workspace_plan():
    opt = _lib.default_fit_options()
    assert (opt.training_iter, opt.lr, opt.jitter, opt.min_variance, opt.eval_stale_chol) == (50, 0.1, 1e-4, 1e-6, 0)
    # gpytorch's psd_safe_cholesky: cholesky_max_tries = 3, cholesky_jitter(float64) = 1e-8; float64 arithmetic
    assert (opt.psd_retries, opt.psd_jitter, opt.precision, opt.reserved) == (3, 1e-8, 0, 0)
    lib = _lib.load()
    descs = (_lib.FitDesc * 3)()
    for i, (m1, m2, t) in enumerate([(3, 4, 5), (40, 60, 20), (100, 120, 300)]):
        descs[i].m1, descs[i].m2, descs[i].t = m1, m2, t
    total = lib.gapro_fit_plan_workspace(C.cast(descs, C.c_void_p), 3, 6)
    sizes = [lib.gapro_fit_workspace_doubles(d.m1 + d.m2, d.t, 6) for d in descs]
    assert total == 8 * sum(sizes)
    assert [d.ws_offset for d in descs] == [0, sizes[0], sizes[0] + sizes[1]]


def test_product_does_not_import_the_oracle():
    """The oracle is test infrastructure: nothing under gapro_amd/ may reference it."""
    pkg = os.path.join(ROOT, "gapro_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".h")):
                text = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", text, flags=re.M), f


def test_padding_and_route_agree_for_every_size_and_feature_width():
    """the padded size must be one the kernel the fit is routed to can run.  Odd multiples of 16
    beyond the strip range exist only on the LDS-staged route; a fit the cluster kernel takes is padded to 32; the
    generic kernel (D > 32) takes any multiple of 16 (its 32 x 32 tiles only at multiples of 32)."""
    lib = _lib.load()
    for d in (6, 16, 32, 40):
        for m in range(2, 1200):
            mp, r = lib.gapro_fit_padded_m(m, d), lib.gapro_fit_route(m, d)
            assert mp >= m and mp % 16 == 0 and mp - m < 32
            if r == 4:
                assert mp % 32 == 0 and mp >= 64, (m, d, mp)
            if r in (0, 3):
                assert mp <= 128
            if r == 5:
                assert (mp <= 48 and d == 6) or (mp <= 32 and d == 32)  # round 6: the wave kernel at D = 32 too
            if r == 2:
                assert d > 32, (m, d, mp)  # nothing the reference's feature widths produce reaches the generic kernel
            if d > 32:
                assert r == 2
    # deep features beyond the staged kernel's LDS: round 3 padded these to 272 / 304 / 336 and the generic kernel
    # then skipped their last 16 rows
    for m, mp in [(260, 288), (272, 288), (300, 320), (304, 320), (330, 352), (336, 352), (200, 208), (209, 224)]:
        assert lib.gapro_fit_padded_m(m, 32) == mp, m
        assert lib.gapro_fit_route(m, 32) == (1 if mp <= 208 else 4), m
    assert [lib.gapro_fit_padded_m(m, 6) for m in (130, 200, 230, 260, 300, 330, 340)] == [144, 208, 256, 272, 304, 336, 352]


def _dbg_enumerators():
    text = open(os.path.join(ROOT, "include", "gapro_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return dict(re.findall(r"\bGAPRO_FIT_DBG_([A-Z_]+)\s*=\s*([0-9| ]+)", text))


def test_debug_bit_names_match_the_header():
    enum = _dbg_enumerators()
    all_bits = sum(int(v) for v in enum.pop("ALL").split("|"))  # distinct powers of two
    assert len(enum) == 10
    for name, value in enum.items():
        assert getattr(_lib, "FIT_DBG_" + name) == int(value), name
    assert sorted(n[8:] for n in dir(_lib) if n.startswith("FIT_DBG_")) == sorted(enum)
    union = 0
    for name in enum:
        union |= getattr(_lib, "FIT_DBG_" + name)
    assert union == all_bits


def test_route_with_flags_agrees_with_the_plain_route_and_honours_every_routing_bit():
    """gapro_fit_route_flags is the launch's own router: flags = 0 is gapro_fit_route, a bit that switches a kernel off
    never yields that kernel's route, and NO_WAVE alone sends exactly the wave kernel's sizes to the small-fit kernel."""
    lib = _lib.load()
    forbids = {_lib.FIT_DBG_NO_WAVE: (5,), _lib.FIT_DBG_NO_CLUSTER: (4,), _lib.FIT_DBG_NO_STRIP: (0, 3),
               _lib.FIT_DBG_NO_SMALL: (3,)}
    for d in (6, 16, 32, 40):
        for m in range(2, 1200):
            r0 = lib.gapro_fit_route(m, d)
            assert lib.gapro_fit_route_flags(m, d, 0) == r0, (m, d)
            for bit, routes in forbids.items():
                r = lib.gapro_fit_route_flags(m, d, bit)
                assert 0 <= r <= 5 and r not in routes, (m, d, bit, r)
            if r0 == 5:
                assert lib.gapro_fit_route_flags(m, d, _lib.FIT_DBG_NO_WAVE) == 3, (m, d)
    for bad in (32, 64, 1 << 21, 1 << 30, 8 | 4096):  # as the launch refuses them
        assert lib.gapro_fit_route_flags(100, 6, bad) == -1  # GAPRO_ERR_BAD_ARG
