#!/usr/bin/env python3
"""Generate tests/golden/spf_predict_*.npz by running the REFERENCE's SPFormer.predict_by_feat in this container.

Run from the repo root:  python tests/golden/make_golden_spf_predict.py
Needs /root/reference (read-only).  What is executed from the reference, on CPU tensors: ``SPFormer.predict_by_feat``
(SPFormer/spformer/model/spformer.py:180-242), unbound, with a ``SimpleNamespace`` as ``self`` that holds ``num_class``,
``decoder.num_query`` and ``test_cfg``, and through it ``rle_encode_gpu_batch``, imported as it is.  IN THIS HARNESS
ONLY: ``gorilla`` is a registry whose decorator returns the class; ``pointgroup_ops``, ``spconv.pytorch`` and
``torch_scatter`` are empty (``torch_scatter`` holds the two names spformer.py imports, set to ``None``);
``spformer.model.backbone``, ``spformer.model.loss`` and ``spformer.model.query_decoder`` hold the imported names set to
``None``; ``spformer.utils`` is the reference's utils/mask_encoder.py loaded by path plus an identity ``cuda_cast``.

``torch.topk`` refuses k beyond the number of scores, so the reference cannot run with ``topk_insts > Q C`` at all; for
the fixture with ``Q C < topk_insts`` its ``test_cfg.topk_insts`` is ``Q C`` (what the library's K = min(topk_insts,
Q C) selects) while the fixture records the larger ``topk_insts`` the library is called with.

The reference leaves the order of its output and every tie to ``torch.topk(sorted=False)``, so a fixture is only written
if the reference's own float32 numbers meet these conditions (asserted below, not tolerances):
  (a) any two scores among the first K + 1 differ by more than 1e-5 relative;
  (b) every final score differs from score_thr by more than 1e-5 relative, or is exactly 0 or negative while the
      threshold is 0;
  (c) no mask logit of a candidate row lies in (-1e-6, 1e-6) other than an exact zero;
  (d) N < 2^24.
The fixtures hold the inputs, the parameters and what the reference returned (label_id, conf, box, the counts of every
instance back to back with their offsets).  Nothing of the reference's text is written.  The restatement
tests/spf_predict_ref.py is run on the same inputs; the largest relative deviation of its conf from the reference's
float32 chain is printed.
"""
import importlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference/SPFormer"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(REPO, "tests"))

import spf_predict_cases  # noqa: E402
import spf_predict_ref  # noqa: E402


def install_stubs():
    gorilla = types.ModuleType("gorilla")

    class Registry:
        def register_module(self, *args, **kwargs):
            return lambda cls: cls

    gorilla.MODELS = Registry()
    empty = {name: types.ModuleType(name) for name in ("pointgroup_ops", "spconv", "spconv.pytorch", "torch_scatter")}
    empty["spconv"].pytorch = empty["spconv.pytorch"]
    empty["torch_scatter"].scatter_max = empty["torch_scatter"].scatter_mean = None
    pkg = types.ModuleType("spformer")
    pkg.__path__ = [os.path.join(REF, "spformer")]
    model = types.ModuleType("spformer.model")
    model.__path__ = [os.path.join(REF, "spformer", "model")]
    holders = {}
    for mod, names in (("backbone", ("MLP", "ResidualBlock", "UBlock")), ("loss", ("Criterion",)),
                       ("query_decoder", ("QueryDecoder",))):
        m = types.ModuleType("spformer.model." + mod)
        for name in names:
            setattr(m, name, None)
        holders["spformer.model." + mod] = m
    spec = importlib.util.spec_from_file_location("spformer.utils.mask_encoder",
                                                  os.path.join(REF, "spformer", "utils", "mask_encoder.py"))
    enc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(enc)
    utils = types.ModuleType("spformer.utils")
    for name in dir(enc):
        if name.startswith("rle_"):
            setattr(utils, name, getattr(enc, name))
    utils.cuda_cast = lambda f: f
    sys.modules.update({"gorilla": gorilla, "spformer": pkg, "spformer.model": model, "spformer.utils": utils,
                        "spformer.utils.mask_encoder": enc, **empty, **holders})


def rel_gap(a, b):
    return abs(float(a) - float(b)) / max(abs(float(a)), abs(float(b)), 1e-30)


def check_conditions(name, c, p, K):
    """(a)-(d) on the reference's own float32 numbers."""
    import torch.nn.functional as F
    C = c["num_class"]
    scores = F.softmax(torch.from_numpy(c["labels"]), dim=-1)[:, :-1] * torch.from_numpy(c["pred_scores"])[:, None]
    top, idx = torch.sort(scores.reshape(-1), descending=True)
    for i in range(min(K, len(top) - 1)):
        assert rel_gap(top[i], top[i + 1]) > 1e-5, (name, "a", i)
    q = torch.div(idx[:K], C, rounding_mode="floor")
    rows = torch.from_numpy(c["masks"])[q]
    near = (rows.abs() < 1e-6) & (rows != 0)
    assert not near.any(), (name, "c")
    on = (rows > 0).float()
    final = top[:K] * ((rows.sigmoid() * on).sum(1) / (on.sum(1) + 1e-6))
    for v in final:
        assert rel_gap(v, p["score_thr"]) > 1e-5 or (p["score_thr"] == 0 and float(v) <= 0), (name, "b")
    assert len(c["superpoints"]) < 2 ** 24, (name, "d")


# name -> scene arguments, parameters
FIXTURES = (
    ("plain", dict(seed=701, N=2500), dict(topk_insts=100, score_thr=0.0, npoint_thr=100)),
    ("few_queries", dict(seed=702, Q=5, C=18, S=60, N=2000, n_inst=4), dict(topk_insts=100, score_thr=0.0, npoint_thr=30)),
    ("score_thr", dict(seed=703, Q=40, S=150, N=2500), dict(topk_insts=100, score_thr=0.3, npoint_thr=100)),
    ("npoint_negative", dict(seed=704, Q=20, S=90, N=2000, n_inst=20, negative=5, amp=2.0),
     dict(topk_insts=300, score_thr=0.0, npoint_thr=600)),
)


def main():
    install_stubs()
    net = importlib.import_module("spformer.model.spformer")
    worst = 0.0
    for name, scene_args, p in FIXTURES:
        c = spf_predict_cases.make_scene(grid=True, **scene_args)
        Q, C, N = c["labels"].shape[0], c["num_class"], len(c["superpoints"])
        K = min(p["topk_insts"], Q * C)
        check_conditions(name, c, p, K)
        me = types.SimpleNamespace(
            num_class=C, decoder=types.SimpleNamespace(num_query=Q),
            test_cfg=types.SimpleNamespace(topk_insts=K, score_thr=p["score_thr"], npoint_thr=p["npoint_thr"]))
        out = dict(labels=torch.from_numpy(c["labels"])[None].clone(),
                   scores=torch.from_numpy(c["pred_scores"])[None, :, None].clone(),
                   masks=[torch.from_numpy(c["masks"]).clone()])
        insts = [types.SimpleNamespace(gt_instances=None)]
        got = net.SPFormer.predict_by_feat(me, ["scene"], out, torch.from_numpy(c["superpoints"]), insts,
                                           torch.from_numpy(c["coords_float"]))["pred_instances"]
        label = np.array([int(g["label_id"]) for g in got], np.int64)
        conf = np.array([np.float32(g["conf"]) for g in got], np.float32)
        box = np.array([np.asarray(g["box"], np.float32) for g in got], np.float32).reshape(-1, 6)
        counts = [np.asarray(g["pred_mask"]["counts"], np.int64) for g in got]
        assert all(g["pred_mask"]["length"] == N for g in got)
        offsets = np.concatenate([[0], np.cumsum([len(x) for x in counts])]).astype(np.int64)
        ours = spf_predict_ref.predict_ref(**c, **p)
        dev = spf_predict_ref.compare_with_reference(ours, label, conf, counts, box)
        worst = max(worst, dev)
        path = os.path.join(OUT, "spf_predict_%s.npz" % name)
        np.savez_compressed(
            path, num_class=np.int64(C), topk_insts=np.int64(p["topk_insts"]), score_thr=np.float64(p["score_thr"]),
            npoint_thr=np.int64(p["npoint_thr"]), ref_label_id=label, ref_conf=conf, ref_box=box,
            ref_counts=np.concatenate(counts) if counts else np.zeros(0, np.int64), ref_offsets=offsets,
            **{k: c[k] for k in spf_predict_ref.INPUTS})
        print("%-16s candidates=%3d after score_thr=%3d instances=%3d  runs=%5d  conf deviation %.3g  %d bytes"
              % (name, ours["stages"][0], ours["stages"][1], len(got), int(offsets[-1]) // 2, dev, os.path.getsize(path)))
    assert [f[0] for f in FIXTURES] == spf_predict_ref.FIXTURES
    print("wrote %d fixtures; largest relative conf deviation of the restatement: %.3g" % (len(FIXTURES), worst))


if __name__ == "__main__":
    main()
