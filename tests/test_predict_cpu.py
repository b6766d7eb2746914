"""Exported GP states and the predict entry points: what can be checked without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_model(rng, m, d, status=0):
    from gapro_amd.gp_model import GPModel

    return GPModel(rng.normal(size=(m, d)), rng.normal(size=m), np.tril(rng.normal(size=(m, m))), rng.normal(),
                   rng.normal(), rng.normal(), 1e-4, status)


@pytest.mark.parametrize("m,d", [(2, 6), (3, 6), (50, 6), (22, 32), (45, 40), (1040, 6)])
def test_state_sizes_follow_the_documented_layout(m, d):
    """gapro_gp_state_doubles = 8 header doubles + Z [M, D] + mean [M] + tril(L_S) [M, M], unpadded; gapro_gp_state_plan
    packs the states of a launch in descriptor order and returns the total in bytes."""
    from gapro_amd import _lib
    from gapro_amd.gp_model import state_doubles

    lib = _lib.load()
    assert lib.gapro_gp_state_doubles(m, d) == 8 + m * d + m + m * m == state_doubles(m, d)
    assert lib.gapro_gp_state_doubles(0, d) == 0 and lib.gapro_gp_state_doubles(m, 0) == 0
    sizes = [(1, 1), (m // 2 + 1, m - m // 2 - 1 if m > 2 else 1), (7, 9)]
    descs = (_lib.FitDesc * len(sizes))()
    for k, (m1, m2) in enumerate(sizes):
        descs[k].m1, descs[k].m2, descs[k].t = m1, m2, 5
    off = np.full(len(sizes), -1, dtype=np.int64)
    total = lib.gapro_gp_state_plan(C.cast(descs, C.c_void_p), len(sizes), d, C.c_void_p(off.ctypes.data))
    want = np.cumsum([0] + [lib.gapro_gp_state_doubles(a + b, d) for a, b in sizes])
    assert list(off) == list(want[:-1]) and total == 8 * want[-1]


def test_predict_desc_and_the_old_structs_keep_their_sizes():
    """gapro_predict_desc is three int64 and two int32 (32 bytes), as the header declares it; the fit structs the issue
    pins stay 56 bytes each, and the version stays 200."""
    from gapro_amd import _lib

    assert C.sizeof(_lib.PredictDesc) == 32
    assert C.sizeof(_lib.FitDesc) == 56 and C.sizeof(_lib.FitOptions) == 56
    assert _lib.load().gapro_version() == 200
    hdr = open(os.path.join(ROOT, "include", "gapro_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} gapro_predict_desc;", hdr).group(1)
    fields = re.findall(r"\b(int64_t|int32_t)\s+(\w+);", body)
    assert [f[1] for f in fields] == [n for n, _ in _lib.PredictDesc._fields_]
    assert sum(8 if t == "int64_t" else 4 for t, _ in fields) == 32


def test_predict_workspace_grows_with_the_models():
    from gapro_amd import _lib

    lib = _lib.load()

    def ws(ms, d=6):
        a = np.asarray(ms, dtype=np.int32)
        return lib.gapro_svgp_predict_workspace_bytes(len(ms), d, C.c_void_p(a.ctypes.data))

    assert ws([]) == 0
    one = ws([50])
    assert one >= 8 * (2 * 64 * 64 + 64)  # (L^-1)^T and tril(L_S) padded to the 16-wide tile, and the mean
    assert ws([50, 50]) > one and ws([50, 300]) > ws([50, 200]) > ws([50, 50])


def test_gpmodel_round_trips_bit_for_bit(tmp_path):
    from gapro_amd.gp_model import GPModel, load_models, save_models

    rng = np.random.default_rng(3)
    a = _random_model(rng, 7, 6)
    s = a.to_state()
    assert s[0] == 7 and s[1] == 6 and s[2] == 0 and s[3] == 1e-4 and s[7] == 0 and len(s) == 8 + 42 + 7 + 49
    b = GPModel.from_state(s)
    for k in ("Z", "mean", "LS"):
        assert np.array_equal(getattr(a, k), getattr(b, k))
    assert (a.c, a.rho_s, a.rho_l, a.jitter, a.status) == (b.c, b.rho_s, b.rho_l, b.jitter, b.status)
    assert np.isclose(a.outputscale, np.log1p(np.exp(a.rho_s))) and np.isclose(a.lengthscale, np.log1p(np.exp(a.rho_l)))
    p = tmp_path / "one.npz"
    a.save(p)
    c = GPModel.load(p)
    assert np.array_equal(c.to_state().view(np.uint64), s.view(np.uint64))
    many = [a, _random_model(rng, 50, 32), _random_model(rng, 2, 6, status=-5)]
    q = tmp_path / "many.npz"
    save_models(q, many)
    back = load_models(q)
    assert len(back) == 3 and back[2].status == -5 and back[1].d == 32
    for x, y in zip(many, back):
        assert np.array_equal(x.to_state().view(np.uint64), y.to_state().view(np.uint64))
    with pytest.raises(ValueError):
        GPModel.load(q)  # three models: not the single form


def test_predict_rejects_another_feature_width_before_touching_a_device():
    from gapro_amd.gaussian_process_utils import predict_gp_batch

    rng = np.random.default_rng(4)
    model = _random_model(rng, 5, 6)
    with pytest.raises(ValueError, match="feature width"):
        predict_gp_batch([model], np.zeros((10, 7), np.float32), [np.arange(3)])
    with pytest.raises(ValueError):
        predict_gp_batch([model], np.zeros(10, np.float32), [np.arange(3)])
