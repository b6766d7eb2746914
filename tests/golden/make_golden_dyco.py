#!/usr/bin/env python3
"""Generate tests/golden/dyco_*.npz by running the REFERENCE's dynamic-convolution mask head in this container.

Run from the repo root:  python tests/golden/make_golden_dyco.py
Needs /root/reference (read-only).  What is executed from the reference, on CPU tensors: ``ISBNet.parse_dynamic_params``
(ISBNet/isbnet/model/isbnet.py:834-853) and ``ISBNet.mask_heads_forward`` (:855-885), unbound, with a
``SimpleNamespace`` as ``self``, in float32 and in float64, with torch's autograd for the four gradients under a fixed
random upstream gradient.  ``isbnet`` is imported behind the stubs of make_golden_proposals.py.

A fixture is only written if the float64 run meets two conditions (asserted below, not tolerances), so that the
float32 and the float64 run agree on every active set:
  (a) no pre-activation of either hidden layer lies within 1e-6, relative to the layer's largest magnitude, of zero
      (the pre-activations are those of tests/dyco_ref.py, whose logits and gradients are first held to the
      reference's float64 ones to 1e-12 relative);
  (b) no box-dimension difference lies in (0, 1e-6).
The fixtures hold the inputs, the upstream gradient, the reference's float64 results and ``ref_dev_*``, the largest
deviation of its float32 results from them, per array.  Nothing of the reference's text is written.  Two queries at
C = 32 keep a file far under 100 KB (a controller row is 1793 floats, and its float64 gradient is kept too).
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, OUT)

import dyco_cases  # noqa: E402
import dyco_ref  # noqa: E402
from make_golden_proposals import install_stubs  # noqa: E402

# name -> seed, C, Q, N (the last one is a workgroup's 64 points and one more)
FIXTURES = (("c32", 601, 32, 2, 37), ("c16", 602, 16, 3, 16), ("c32_tile", 603, 32, 2, 65))
NAMES = ("logits", "grad_controllers", "grad_mask_features", "grad_box_preds", "grad_queries_box_preds")


def run_reference(net, case, dtype):
    C, Q = case["mask_features"].shape[1], case["controllers"].shape[1]
    H = C // 2
    me = types.SimpleNamespace(weight_nums=[(C + 6) * C, C * H, H], bias_nums=[C, H, 1], mask_dim_out=C)
    t = {k: torch.from_numpy(case[k]).to(dtype) for k in dyco_cases.KEYS}
    for k in dyco_cases.GRAD_KEYS:
        t[k].requires_grad_()
    weights, biases = net.ISBNet.parse_dynamic_params(me, t["controllers"][0], C)
    y = net.ISBNet.mask_heads_forward(me, t["mask_features"][:, :, None], weights, biases, Q, t["locs_float"],
                                      t["box_preds"], t["queries_locs"][0], t["queries_box_preds"][0])
    y.backward(torch.from_numpy(case["grads"][0]).to(dtype))
    out = {"logits": y.detach().numpy()}
    for k in dyco_cases.GRAD_KEYS:
        out["grad_" + k] = t[k].grad.numpy()
    return out


def main():
    install_stubs()
    net = importlib.import_module("isbnet.model.isbnet")
    for name, seed, C, Q, N in FIXTURES:
        case = dyco_cases.make_case(seed, C, Q, [N])
        f32, f64 = run_reference(net, case, torch.float32), run_reference(net, case, torch.float64)
        args = [case[k][0] if case[k].ndim == 3 else case[k] for k in dyco_cases.KEYS]
        y, _, d, p1, p2 = dyco_ref.forward(*args, full=True)
        mine = dict(zip(NAMES, (y,) + dyco_ref.backward(*args, case["grads"][0])))
        for k in NAMES:
            want = f64[k].reshape(mine[k].shape)
            assert np.abs(mine[k] - want).max() <= 1e-12 * np.abs(want).max(), (name, k)
        for p in (p1, p2):
            assert np.abs(p).min() > 1e-6 * np.abs(p).max(), (name, "a")          # (a)
        assert not ((np.abs(d) > 0) & (np.abs(d) < 1e-6)).any(), (name, "b")      # (b)
        save = {k: case[k] for k in dyco_cases.KEYS}
        save["upstream"] = case["grads"][0]
        for k in NAMES:
            assert f32[k].dtype == np.float32 and f64[k].dtype == np.float64
            save[k + "_f64"] = f64[k]
            save["ref_dev_" + k] = np.float64(np.abs(f32[k].astype(np.float64) - f64[k]).max())
        path = os.path.join(OUT, "dyco_%s.npz" % name)
        np.savez_compressed(path, **save)
        print("%s: %d bytes; ref_dev %s" % (name, os.path.getsize(path),
                                            ", ".join("%s %.2e" % (k, save["ref_dev_" + k]) for k in NAMES)))


if __name__ == "__main__":
    main()
