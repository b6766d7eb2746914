"""Shared cases of the dynamic-convolution mask head tests (tests/test_dyco_cpu.py, tests/test_dyco_gpu.py)."""
import numpy as np

import dyco_ref

KEYS = ("controllers", "mask_features", "locs_float", "box_preds", "queries_locs", "queries_box_preds")
GRAD_KEYS = ("controllers", "mask_features", "box_preds", "queries_box_preds")

# The kernels' edges (gapro_amd/csrc/dyco_head.hip): a wave takes 16 points, a workgroup 64 (four waves); a workgroup
# takes ONE query (so the query group size is 1 and Q = 2 is "group size + 1").  name: (Q, sizes, lead, tail).
SHAPES = {
    "q1_wave_edges": (1, [1, 15, 16, 17], 0, 0),
    "q2_workgroup_edges": (2, [63, 64, 65], 0, 0),
    "q3_empty_middle_odd_offsets": (3, [5, 0, 23], 3, 2),
    "q17_two_workgroups": (17, [130, 33], 0, 1),
}


def make_case(seed, C, Q, sizes, lead=0, tail=0, scale=1.0):
    """Random float32 inputs: ``sizes`` points per sample, ``lead`` / ``tail`` points that no sample owns."""
    rng = np.random.default_rng(seed)
    B, N = len(sizes), lead + sum(sizes) + tail
    P = dyco_ref.param_count(C)
    locs = rng.uniform(0.0, 3.0, (N, 3))
    half = rng.uniform(0.1, 0.8, (N, 2, 3))
    qlocs = rng.uniform(0.0, 3.0, (B, Q, 3))
    qhalf = rng.uniform(0.1, 0.8, (B, Q, 2, 3))
    case = {
        "controllers": rng.normal(0.0, 0.3, (B, Q, P)),
        "mask_features": rng.normal(0.0, 1.0, (N, C)) * scale,
        "locs_float": locs * scale,
        "box_preds": np.concatenate([locs - half[:, 0], locs + half[:, 1]], axis=1) * scale,
        "queries_locs": qlocs * scale,
        "queries_box_preds": np.concatenate([qlocs - qhalf[:, :, 0], qlocs + qhalf[:, :, 1]], axis=2) * scale,
    }
    case = {k: v.astype(np.float32) for k, v in case.items()}
    case["off"] = [int(v) for v in lead + np.concatenate([[0], np.cumsum(sizes)])]
    case["grads"] = [rng.normal(0.0, 1.0, (Q, n)).astype(np.float32) if n else None for n in sizes]
    return case


def reference(case):
    """(logits, gradients) of the restatement for a case, float32."""
    args = [case[k] for k in KEYS] + [case["off"]]
    return dyco_ref.head(*args), dyco_ref.head_backward(*args, case["grads"])


def tolerance(ref):
    """The project's standing bound: one float32 ulp of the value plus 1e-9 times the array's largest magnitude."""
    ref = np.asarray(ref, dtype=np.float32)
    top = float(np.abs(ref).max()) if ref.size else 0.0
    return np.spacing(np.abs(ref)).astype(np.float64) + 1e-9 * top


def assert_close(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref, dtype=np.float32)
    assert got.dtype == np.float32 and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    bound = tolerance(ref)
    worst = float((err - bound).max()) if err.size else 0.0
    print("%s: largest error %.3e, largest magnitude %.3e" % (what, float(err.max()) if err.size else 0.0,
                                                             float(np.abs(ref).max()) if ref.size else 0.0))
    assert np.isfinite(got).all() and worst <= 0.0, "%s: an error exceeds its bound by %.3e" % (what, worst)
