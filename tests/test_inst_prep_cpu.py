"""Instance-label preparation without a GPU: the restatement tests/inst_prep_ref.py against the outputs of the real
reference (tests/golden/inst_prep_*.npz), the closed form of the crop against the hole-filling rule, the conditions of
the GPU test's cases, the refusals that happen before a device is touched, and the workspace function."""
import ctypes as C

import numpy as np
import pytest
import torch

import inst_prep_cases as cases
import inst_prep_ref as ref
from gapro_amd import _lib, consumer_ops, gen_ps_utils


@pytest.mark.parametrize("name", ref.FIXTURES)
def test_restatement_equals_the_reference(name):
    z = ref.fixture(name)
    inst, valid = z["inst"], z["valid"]
    for dt in (np.int64, np.int32, np.float64):
        got = ref.get_cropped_instance_label(inst.astype(dt))
        assert got.dtype == dt and np.array_equal(got, z["cropped"])
        assert np.array_equal(ref.get_cropped_instance_label(inst.astype(dt), valid), z["cropped_valid"])
    labels, cls, box, num, cen, cor = ref.prepare_instance_labels(z["coords"], inst, z["sem"], int(z["label_shift"]))
    assert np.array_equal(labels, z["cropped"]) and np.array_equal(cls, z["cls"]) and cls.dtype == np.int64
    assert np.array_equal(box, z["box"]) and np.array_equal(num, z["pointnum"]) and np.array_equal(cor, z["corners_offset"])
    assert np.array_equal(cen == -100.0, z["centroid_offset"] == -100.0)
    stored = float(ref.summary()["centroid_max_abs_diff"])
    assert np.max(np.abs(cen.astype(np.float64) - z["centroid_offset"].astype(np.float64))) <= stored
    # the two-step form on the cropped labels is the same thing
    two = ref.get_instance_info(z["coords"], z["cropped"], z["sem"], int(z["label_shift"]))
    for a, b in zip(two, (cls, box, cen, cor)):
        assert np.array_equal(ref.bits(a), ref.bits(b))


def test_the_stored_margin_is_a_few_float32_ulps_of_the_coordinates():
    """|coordinate| <= 16 in the fixtures: the reference's float32 mean sits within a few ulps of 16 of the exact one."""
    stored = float(ref.summary()["centroid_max_abs_diff"])
    assert 0.0 < stored <= 4 * np.spacing(np.float32(16.0))
    assert ref.centroid_tolerance() == 4.0 * stored
    assert ref.FIXTURES == [str(n) for n in ref.summary()["names"]]


def test_closed_form_equals_the_hole_filling_rule():
    rng = np.random.default_rng(20261019)
    for trial in range(3000):
        n = int(rng.integers(1, 60))
        top = int(rng.integers(1, 40))
        lab = rng.integers(0, top, n).astype(np.int64)
        lab[rng.random(n) < rng.random() * 0.6] = rng.choice([-100, -1])
        want = ref.crop_loop(lab)
        got = ref.get_cropped_instance_label(lab)
        assert np.array_equal(got, want), (trial, lab)
        p = np.unique(got[got >= 0])
        assert np.array_equal(p, np.arange(len(p))) and np.array_equal(got < 0, lab < 0)
        assert np.array_equal(got[lab < 0], lab[lab < 0])


@pytest.mark.parametrize("name", cases.CASE_NAMES)
def test_every_case_meets_its_condition_and_the_restatement_takes_it(name):
    d = cases.build(name)
    crop = cases.expected(ref.get_cropped_instance_label, d.inst)
    both = cases.expected(ref.prepare_instance_labels, d.coords, d.inst, d.sem, d.shift)
    if name == "an id at the refusal bound":
        assert isinstance(crop, ref.Refused) and isinstance(both, ref.Refused) and both.code == ref.BAD_ARG
    elif name == "only negative labels":
        assert np.array_equal(crop, d.inst) and isinstance(both, ref.Refused) and both.code == ref.BAD_ARG
    elif name == "non-finite coordinate on a labelled point":
        assert not isinstance(crop, ref.Refused) and isinstance(both, ref.Refused) and both.code == ref.NOT_FINITE
    else:
        assert not isinstance(crop, ref.Refused) and not isinstance(both, ref.Refused)
        if d.inst.max() < 5000:  # the rule itself takes one sweep per id
            assert np.array_equal(crop, ref.crop_loop(d.inst))
        assert np.array_equal(both[0], crop) and len(both[1]) == len(cases.present(d))
    alone = cases.expected(ref.get_instance_info, d.coords, d.inst, d.sem, d.shift)
    if len(cases.present(d)) and len(cases.holes(d)):
        assert isinstance(alone, ref.Refused) and alone.code in (ref.BAD_ARG, ref.NOT_FINITE)
    if name == "an instance of one point":
        new = both[0][17]
        assert both[3][new] == 1 and not both[4][17].any() and not both[5][17].any()
        assert np.array_equal(both[2][new], np.r_[d.coords[17], d.coords[17]])
    if name == "signed zeros":
        b = both[2]
        assert np.signbit(b[both[0][d.inst == 2][0]]).all() and not np.signbit(b[both[0][d.inst == 1][0]]).any()
        mixed = both[0][d.inst == 0][0]
        assert np.signbit(b[mixed, :3]).all() and not np.signbit(b[mixed, 3:]).any()  # -0.0 orders below +0.0


def _no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a device was touched")

    monkeypatch.setattr(consumer_ops.Context, "get", boom)
    monkeypatch.setattr(consumer_ops, "_ctx_stream", boom)


def test_bad_arguments_raise_before_a_device_is_touched(monkeypatch):
    _no_device(monkeypatch)
    xyz = torch.zeros((10, 3), dtype=torch.float32)
    inst = torch.zeros(10, dtype=torch.int64)
    sem = torch.zeros(10, dtype=torch.int64)
    for fn in (consumer_ops.get_instance_info, consumer_ops.prepare_instance_labels):
        for bad in [(xyz[:9], inst, sem), (xyz, inst[:9], sem), (xyz, inst, sem[:3]),           # differing lengths
                    (xyz.double(), inst, sem), (xyz.half(), inst, sem), (xyz.view(-1), inst, sem),  # not [V,3] float32
                    (torch.zeros((10, 4)), inst, sem), (xyz.numpy(), inst, sem),
                    (xyz, inst.float(), sem), (xyz, inst.short(), sem), (xyz, inst.bool(), sem),    # unsupported dtypes
                    (xyz, inst, sem.float()), (xyz, inst, sem.to(torch.uint8)),
                    (xyz, inst.view(5, 2), sem), (xyz, inst.numpy(), sem),
                    (xyz[:0], inst[:0], sem[:0])]:                                             # no points
            with pytest.raises(ValueError):
                fn(*bad)
    for bad in (inst.float(), inst.short(), inst.to(torch.uint8), inst.numpy(), inst.view(2, 5), inst[:0]):
        with pytest.raises(ValueError):
            consumer_ops.get_cropped_instance_label(bad)
    with pytest.raises(ValueError):
        consumer_ops.get_cropped_instance_label(inst, torch.zeros(0, dtype=torch.int64))
    # host tensors of the right kind: there is no CPU path in consumer_ops, and it says so without touching a device
    for call in (lambda: consumer_ops.get_instance_info(xyz, inst, sem),
                 lambda: consumer_ops.prepare_instance_labels(xyz, inst, sem)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_names_are_exported_and_bound():
    import gapro_amd

    for n in ("get_cropped_instance_label", "get_instance_info", "prepare_instance_labels"):
        assert n in gapro_amd.__all__ and callable(getattr(gapro_amd, n))
    assert gapro_amd.get_cropped_instance_label is gen_ps_utils.get_cropped_instance_label
    assert gapro_amd.get_instance_info is consumer_ops.get_instance_info
    assert consumer_ops.InstanceLabels._fields == ("instance_labels", "instance_cls", "instance_box", "instance_pointnum",
                                                   "centroid_offset_labels", "corners_offset_labels")
    assert C.sizeof(_lib.InstPrepHeader) == 24
    for n in ("gapro_inst_prep_workspace_bytes", "gapro_inst_crop", "gapro_inst_info", "gapro_inst_prepare"):
        assert n in _lib.SIGNATURES
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gapro_hip.h")).read()
    for name, value in (("MAX_IDS", _lib.INST_PREP_MAX_IDS), ("GRID_CAP", _lib.INST_PREP_GRID_CAP),
                        ("LDS_IDS", _lib.INST_PREP_LDS_IDS)):
        assert int(re.search(r"#define GAPRO_INST_PREP_%s (\d+)" % name, text).group(1)) == value
    assert 1 <= consumer_ops.ID_TABLE < _lib.INST_PREP_MAX_IDS


def test_workspace_bytes_and_bad_arguments_of_the_entry_points():
    lib = _lib.load()
    sizes = [lib.gapro_inst_prep_workspace_bytes(n) for n in (1, 2, 511, 512, 1024, 1 << 20)]
    assert all(s > 0 and s % 256 == 0 for s in sizes) and sizes == sorted(sizes)
    per_id = 8 + 3 * 8 + 4 * 4 + 3 * (3 * 4)  # first, sums | present, map, holes, count | lo, hi, centroid
    for n, s in zip((1, 2, 511, 512, 1024, 1 << 20), sizes):
        assert 64 + n * per_id <= s < 64 + n * per_id + 256
    for bad in (0, -1, (1 << 20) + 1):
        assert lib.gapro_inst_prep_workspace_bytes(bad) == 0
    # without a context every entry refuses at once (nothing is dereferenced)
    assert lib.gapro_inst_crop(None, None, 10, None, 3, 16, None, 0, None, None) == -1
    assert lib.gapro_inst_info(None, None, 10, None, None, 3, None, 3, 0, 16, None, 0, None, None, None, None, None, None,
                               None) == -1
    assert lib.gapro_inst_prepare(None, None, 10, None, None, 3, None, 3, 0, 16, None, 0, None, None, None, None, None,
                                  None, None) == -1
