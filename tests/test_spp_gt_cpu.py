"""Per-sample ground-truth masks without a GPU: the restatement tests/spp_gt_ref.py against the outputs of the real
reference (tests/golden/spp_gt_*.npz), the integer rule against the reference's float32 comparison, the conditions of
the GPU test's cases, the refusals that happen before a device is touched, and the declared entry points."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import spp_gt_cases as cases
import spp_gt_ref as ref
from gapro_amd import _lib, consumer_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ref.FIXTURES)
def test_restatement_equals_the_reference(name):
    z, want = ref.fixture(name)
    B = int(z["batch_size"])
    if name == "subsample":
        got = ref.get_subsample_gt(z["labels"], z["subsample_idxs"], z["cls"], z["box"], z["offsets"], B)
    else:
        got = ref.get_spp_gt(z["labels"], z["spps"], z["cls"], z["box"], z["offsets"], B)
    assert [g is None for g in got] == [bool(v) for v in z["is_none"]]
    assert ref.same(got, want)
    for g in got:
        if g is not None:
            assert g["mask"].dtype == np.float32 and set(np.unique(g["mask"]).tolist()) <= {0.0, 1.0}


def test_the_fixtures_hold_what_they_are_there_for():
    assert [bool(v) for v in ref.fixture("second_empty")[0]["is_none"]] == [False, True, False]
    assert len(ref.fixture("two")[1]) == 2 and len(ref.fixture("four")[1]) == 4
    z, _ = ref.fixture("shared_spp")
    o = z["offsets"]
    assert set(z["spps"][o[0]:o[1]].tolist()) & set(z["spps"][o[1]:o[2]].tolist())
    z, want = ref.fixture("half_splits")
    o, halves = z["offsets"], 0
    for s in np.unique(z["spps"][o[0]:o[1]]):
        lab = z["labels"][o[0]:o[1]][z["spps"][o[0]:o[1]] == s]
        halves += any(2 * np.sum(lab == i) == len(lab) for i in np.unique(lab[lab >= 0]))
    assert halves >= 4
    # a superpoint split in half between two kept instances belongs to both
    assert (want[0]["mask"].sum(axis=0) == 2).any()
    strict = ref.get_spp_gt(z["labels"], z["spps"], z["cls"], z["box"], o, 2, strict=True)
    assert (strict[0]["mask"] <= want[0]["mask"]).all() and strict[0]["mask"].sum() < want[0]["mask"].sum()
    for name in ref.FIXTURES:
        assert os.path.getsize(os.path.join(ref.GOLDEN_DIR, "spp_gt_%s.npz" % name)) < 300 * 1024


def test_integer_rule_equals_the_float32_comparison():
    """c, n < 2^24 are exact in float32 and their quotient is correctly rounded: it cannot round onto or across 0.5."""
    def check(c, n):
        q = c.astype(np.float32) / n.astype(np.float32)
        assert q.dtype == np.float32
        assert np.array_equal(q >= np.float32(0.5), ref.rule(c, n)), "the >= rule"
        assert np.array_equal(q > np.float32(0.5), ref.rule(c, n, strict=True)), "the > rule"

    rng = np.random.default_rng(20261020)
    top = (1 << 24) - 1
    n = rng.integers(1, top + 1, 2_000_000)
    check((rng.random(len(n)) * (n + 1)).astype(np.int64).clip(0, n), n)
    # the nearest counts on either side of half, for small n exhaustively and for large n at random and at the top
    n = np.concatenate([np.arange(1, 1 << 16), rng.integers(1 << 16, top + 1, 1_000_000), np.arange(top - 4096, top + 1)])
    for two_c in (n - 1, n, n + 1):
        for c in (two_c // 2, (two_c + 1) // 2):
            check(c.clip(0, n), n)


@pytest.mark.parametrize("name", cases.CASE_NAMES)
def test_every_case_meets_its_condition_and_the_restatement_takes_it(name):
    d = cases.build(name)
    want = cases.expected(d)
    if name in cases.REFUSED_NAMES:
        assert isinstance(want, ref.Refused)
        return
    assert not isinstance(want, ref.Refused) and len(want) == d.batch_size
    o = d.offsets
    for b, e in enumerate(want):  # the rule, the long way round, on every cell of the small cases
        if e is None or len(d.labels) > 5000:
            continue
        src = np.arange(o[b], o[b + 1]) if d.idxs is None else d.idxs[o[b]:o[b + 1]]
        lab = d.labels[src]
        cols = np.unique(d.spps[src]) if d.spps is not None else None
        assert e["mask"].shape == (len(e["ids"]), len(cols) if cols is not None else len(src))
        for r, i in enumerate(e["ids"]):
            assert i != d.ignore and d.cls[i] >= 0 and (lab == i).any()
            if cols is None:
                assert np.array_equal(e["mask"][r], (lab == i).astype(np.float32))
                continue
            for k, s in enumerate(cols):
                inside = d.spps[src] == s
                assert e["mask"][r, k] == float(2 * np.sum(lab[inside] == i) >= np.sum(inside))


def _no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a device was touched")

    monkeypatch.setattr(consumer_ops.Context, "get", boom)
    monkeypatch.setattr(consumer_ops, "_ctx_stream", boom)


def test_bad_arguments_raise_before_a_device_is_touched(monkeypatch):
    _no_device(monkeypatch)
    lab = torch.zeros(10, dtype=torch.int64)
    spp = torch.zeros(10, dtype=torch.int64)
    cls = torch.zeros(4, dtype=torch.int64)
    box = torch.zeros((4, 6), dtype=torch.float32)
    off = torch.tensor([0, 4, 10])
    good = (lab, spp, cls, box, off, 2)
    bad_calls = [
        (lab.float(), spp, cls, box, off, 2), (lab.short(), spp, cls, box, off, 2), (lab.view(2, 5), spp, cls, box, off, 2),
        (lab.numpy(), spp, cls, box, off, 2),                                       # labels: dtype, rank, kind
        (lab, spp.float(), cls, box, off, 2), (lab, spp.view(5, 2), cls, box, off, 2), (lab, spp[:9], cls, box, off, 2),
        (lab, spp.bool(), cls, box, off, 2),                                         # superpoints
        (lab, spp, cls.float(), box, off, 2), (lab, spp, cls.view(2, 2), box, off, 2), (lab, spp, cls[:0], box[:0], off, 2),
        (lab, spp, cls, box.double(), off, 2), (lab, spp, cls, box[:3], off, 2), (lab, spp, cls, box.view(6, 4), off, 2),
        (lab, spp, cls, box.view(-1), off, 2),                                      # instance_box not [I, 6] float32
        (lab, spp, cls, box, off, 0), (lab, spp, cls, box, off, -1), (lab, spp, cls, box, off, 2.0),
        (lab, spp, cls, box, off, _lib.SPP_GT_MAX_SAMPLES + 1),                     # batch_size
        (lab, spp, cls, box, off, 3), (lab, spp, cls, box, off[:2], 2), (lab, spp, cls, box, [0, 10], 2),
        (lab, spp, cls, box, off.float(), 2), (lab, spp, cls, box, off.view(3, 1), 2), (lab, spp, cls, box, "abc", 2),
        (lab[:0], spp[:0], cls, box, off, 2),                                       # no points
    ]
    for bad in bad_calls:
        with pytest.raises(ValueError):
            consumer_ops.get_spp_gt(*bad)
        if bad[1] is spp:  # the same refusals with subsample indices in the superpoints' place
            with pytest.raises(ValueError):
                consumer_ops.get_subsample_gt(*bad)
    with pytest.raises(ValueError, match="get_subsample_gt"):
        consumer_ops.get_spp_gt(*good, pool=False)
    for n_spps in (0, -3, 2.5, True):
        with pytest.raises(ValueError):
            consumer_ops.get_spp_gt(*good, n_spps=n_spps)
    for bad_idx in (spp.float(), spp.view(2, 5), spp[:0], spp.numpy()):
        with pytest.raises(ValueError):
            consumer_ops.get_subsample_gt(lab, bad_idx, cls, box, off, 2)
    # host tensors of the right kind: there is no CPU path in consumer_ops, and it says so without touching a device
    for call in (lambda: consumer_ops.get_spp_gt(*good), lambda: consumer_ops.get_spp_gt(*good, n_spps=1),
                 lambda: consumer_ops.get_subsample_gt(*good)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_names_are_exported_declared_and_bound():
    import gapro_amd

    for n in ("get_spp_gt", "get_subsample_gt"):
        assert n in gapro_amd.__all__ and getattr(gapro_amd, n) is getattr(consumer_ops, n)
        assert n in gapro_amd._EXPORTS["consumer_ops"]
    text = open(os.path.join(ROOT, "include", "gapro_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for n in ("gapro_spp_gt_workspace_bytes", "gapro_spp_gt_count", "gapro_spp_gt_fill"):
        assert re.search(r"\b%s\s*\(" % n, code), n
        assert n in _lib.SIGNATURES and hasattr(lib, n)
    assert C.sizeof(_lib.SppGtHeader) == 40
    for name, value in (("MAX_SAMPLES", _lib.SPP_GT_MAX_SAMPLES), ("MAX_BATCH_SPPS", _lib.SPP_GT_MAX_BATCH_SPPS),
                        ("GRID_CAP", _lib.SPP_GT_GRID_CAP)):
        assert int(re.search(r"#define GAPRO_SPP_GT_%s (\d+)" % name, text).group(1)) == value
    assert re.search(r"GAPRO_SPP_GT_HALF = 0, GAPRO_SPP_GT_STRICT = 1", text)
    assert (_lib.SPP_GT_HALF, _lib.SPP_GT_STRICT) == (0, 1)
    assert lib.gapro_version() == 200
    assert "spp_gt.hip" in open(os.path.join(ROOT, "gapro_amd", "csrc", "build.sh")).read()


def test_workspace_bytes_and_bad_arguments_of_the_entry_points():
    lib = _lib.load()
    f = lib.gapro_spp_gt_workspace_bytes
    sizes = [f(n, b, i, s) for n, b, i, s in ((1, 1, 1, 0), (1, 1, 1, 1), (1000, 4, 33, 65), (60000, 4, 160, 6000))]
    assert all(s > 0 and s % 256 == 0 for s in sizes)
    # scalars | three offset tables | two counts | 64 copies of the instance words and 64 of the superpoint words, a
    # 128-byte line each (4 x 2 and 4 x 3 words fit one) | the prefixes of both tables | the table of n
    want = 64 + 3 * 8 * 5 + 2 * 4 * 4 + 2 * 64 * 128 + 4 * 4 * (2 + 3) + 4 * 1000
    assert want <= sizes[2] < want + 256
    assert f(1000, 4, 33, 0) < sizes[2]  # without superpoints: no table of n
    for bad in ((0, 1, 1, 1), ((1 << 31), 1, 1, 1), (10, 0, 1, 1), (10, _lib.SPP_GT_MAX_SAMPLES + 1, 1, 1), (10, 1, 0, 1),
                (10, 1, _lib.INST_PREP_MAX_IDS + 1, 1), (10, 1, 1, -1), (10, 1024, 1, 1 << 21)):
        assert f(*bad) == 0, bad
    assert f((1 << 31) - 1, 1024, _lib.INST_PREP_MAX_IDS, (1 << 21) - 1) > 0
    # without a context every entry refuses at once (nothing is dereferenced)
    assert lib.gapro_spp_gt_count(None, None, 10, 10, None, 3, None, None, 0, 0, None, 3, 4, None, 2, -100, None, 0, None,
                                  None) == -1
    assert lib.gapro_spp_gt_fill(None, None, 10, 10, None, 3, None, None, 0, 0, None, 3, 4, None, None, 2, -100, 0, None,
                                 0, None, 0, None, None, None, 0, None) == -1
