#!/usr/bin/env python3
"""Golden outputs of the reference's two vote functions (gen_ps_utils.py:99-129 spp_align_label, :132-166
spp_major_voting) on the golden scenes, by running the REAL reference functions in this container
(python tests/golden/make_golden_votes.py), with the torch_scatter shim of make_golden_labelers.py.

Inputs per scene: ids = np.unique(spp, return_inverse=True) (dense: the reference's :141-143 indexes with the raw ids);
occupancy = point inside gi_box widened by 0.005 (:502-504); rng = default_rng(7); label = a random occupied box + 1, or 0
where no box is occupied; prob = rng.random(N) as float32.  spp_align_label runs plain, with bb_occupancy_spp = superpoint
mean of the occupancy >= 0.7 (:546), and with prob_label.  Writes data-only tests/golden/votes_<scene>.npz (inputs and
outputs) and votes_SUMMARY.json: per scene the number of superpoints whose masked counts tie or are all masked, and the
largest |reference probability - tests/vote_ref.py| -- the reference sums in float32 in an unspecified order, and four
times that figure is the tolerance of the fixture tests.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import make_golden_labelers as mgl  # noqa: E402
import vote_ref  # noqa: E402


def main():
    mg.install_stubs()
    mgl.extend_shim()
    sys.path.insert(0, mg.REF)
    import gen_ps_utils as ref

    summary = {"scenes": {}, "max_abs_prob_diff": 0.0}
    for name, _ in mg.SCENES:
        d = np.load(os.path.join(HERE, name + ".npz"), allow_pickle=True)
        xyz = np.asarray(d["xyz_aligned"], dtype=np.float32)
        box = np.asarray(d["gi_box"], dtype=np.float32)
        _, ids = np.unique(d["spp"], return_inverse=True)
        ids = ids.astype(np.int64)
        n, B, S = len(ids), len(box), int(ids.max()) + 1
        occ = np.all(xyz[:, None, :] >= box[None, :, :3] - 0.005, axis=-1) & \
            np.all(xyz[:, None, :] <= box[None, :, 3:] + 0.005, axis=-1)  # [N, B]
        rng = np.random.default_rng(7)
        n_occ = occ.sum(axis=1)
        pick = np.minimum((rng.random(n) * n_occ).astype(np.int64), np.maximum(n_occ - 1, 0))
        rank = np.cumsum(occ, axis=1) - 1  # rank of every occupied box among the point's occupied boxes
        label = np.where(n_occ > 0, np.argmax(occ & (rank == pick[:, None]), axis=1) + 1, 0).astype(np.int64)
        prob = rng.random(n).astype(np.float32)
        occ_mean = np.zeros((B, S), dtype=np.float32)
        np.add.at(occ_mean.T, ids, occ.astype(np.float32))
        occ_spp = (occ_mean / np.bincount(ids, minlength=S).astype(np.float32)[None, :]) >= 0.7  # [B, S]

        t_ids, t_label, t_prob = torch.from_numpy(ids), torch.from_numpy(label), torch.from_numpy(prob)
        C = B + 1
        mj_label, mj_prob = ref.spp_major_voting(t_ids, t_label, t_prob, torch.from_numpy(occ), C)
        al_label = ref.spp_align_label(t_ids, t_label, n_classes=C)
        al_gated = ref.spp_align_label(t_ids, t_label, n_classes=C, bb_occupancy_spp=torch.from_numpy(occ_spp))
        al_label2, al_prob = ref.spp_align_label(t_ids, t_label, n_classes=C, prob_label=t_prob)
        assert torch.equal(al_label, al_label2)
        out = dict(ids=ids, label=label, prob=prob, occ=occ, occ_spp=occ_spp,
                   major_label=mj_label.numpy().astype(np.int64), major_prob=mj_prob.numpy().astype(np.float32),
                   align_label=al_label.numpy().astype(np.int64), align_gated_label=al_gated.numpy().astype(np.int64),
                   align_prob=al_prob.numpy().astype(np.float32))
        np.savez_compressed(os.path.join(HERE, "votes_" + name + ".npz"), **out)

        # the restatement against the reference: labels equal, probabilities measured
        r_label, r_prob = vote_ref.spp_major_voting(ids, label, prob, occ, C)
        a_label, a_prob = vote_ref.spp_align_label(ids, label, C, None, prob)
        g_label = vote_ref.spp_align_label(ids, label, C, occ_spp)
        assert np.array_equal(r_label, out["major_label"]) and np.array_equal(a_label, out["align_label"])
        assert np.array_equal(g_label, out["align_gated_label"])
        diff = max(float(np.max(np.abs(r_prob.astype(np.float64) - out["major_prob"]))),
                   float(np.max(np.abs(a_prob.astype(np.float64) - out["align_prob"]))))
        cnt = np.zeros((S, C), dtype=np.int64)
        np.add.at(cnt, (ids, label), 1)
        occn = np.zeros((S, B), dtype=np.int64)
        np.add.at(occn, ids, occ.astype(np.int64))
        m = cnt.copy()
        m[:, 1:] *= occn == cnt.sum(axis=1)[:, None]
        top = m.max(axis=1)
        ties = int((((m == top[:, None]).sum(axis=1) > 1) | ((cnt[:, 1:].sum(axis=1) > 0) & (m[:, 1:].sum(axis=1) == 0))).sum())
        summary["scenes"][name] = dict(points=n, superpoints=S, classes=C, tied_or_masked_superpoints=ties,
                                       largest_superpoint=int(cnt.sum(axis=1).max()), max_abs_prob_diff=diff)
        summary["max_abs_prob_diff"] = max(summary["max_abs_prob_diff"], diff)
        print(name, summary["scenes"][name])
    with open(os.path.join(HERE, "votes_SUMMARY.json"), "w") as f:
        json.dump(summary, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
