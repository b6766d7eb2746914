"""Host side of the superpoint vote (no GPU needed): the NumPy restatement tests/vote_ref.py against the reference's
recorded outputs (tests/golden/votes_<scene>.npz, written by make_golden_votes.py), its block vote on hand-made cases
with known answers, point_level="vote" as a value, the ABI of gapro_spp_vote / gapro_point_refine_vote and the CLI's
refusal of --point_vote beside another point mode."""
import ctypes as C

import numpy as np
import pytest

import vote_ref
from gapro_amd import _lib
from gapro_amd.pipeline import Pipeline, point_mode
from vote_ref import SCENES, fixture, prob_tolerance

@pytest.mark.parametrize("name", SCENES)
def test_restatement_against_the_reference(name):
    d = fixture(name)
    C_ = d["occ"].shape[1] + 1
    tol = prob_tolerance()
    lab, prob = vote_ref.spp_major_voting(d["ids"], d["label"], d["prob"], d["occ"], C_)
    assert np.array_equal(lab, d["major_label"])
    assert prob.dtype == np.float32 and np.max(np.abs(prob.astype(np.float64) - d["major_prob"])) <= tol
    assert np.array_equal(vote_ref.spp_align_label(d["ids"], d["label"], C_), d["align_label"])
    assert np.array_equal(vote_ref.spp_align_label(d["ids"], d["label"]), d["align_label"])  # n_classes = -1
    assert np.array_equal(vote_ref.spp_align_label(d["ids"], d["label"], C_, d["occ_spp"]), d["align_gated_label"])
    lab, prob = vote_ref.spp_align_label(d["ids"], d["label"], C_, None, d["prob"])
    assert np.array_equal(lab, d["align_label"])
    assert np.max(np.abs(prob.astype(np.float64) - d["align_prob"])) <= tol
    assert (d["align_label"] != d["label"]).any()  # the fixture is not trivial: the vote changes labels


def test_the_gates_matter_in_the_fixtures():
    """On at least one scene each, the all-inside gate and the >= 0.7 gate mask votes that the plain vote counts."""
    ds = [fixture(n) for n in SCENES]
    assert any((d["major_label"] != d["align_label"]).any() for d in ds)
    assert any((d["align_gated_label"] != d["align_label"]).any() for d in ds)


def test_restatement_rules():
    # first maximum: 2 : 2 between classes 1 and 2 -> 1; every box class masked -> 0; a superpoint of one point
    spp = np.array([5, 5, 5, 5, 9, 9, 2])
    label = np.array([2, 1, 2, 1, 1, 1, 2])
    assert vote_ref.spp_align_label(spp, label, 3).tolist() == [1, 1, 1, 1, 1, 1, 2]
    gate = np.array([[1, 0, 0], [1, 1, 0]])  # [C - 1, S], superpoints by ascending id: 2, 5, 9
    assert vote_ref.spp_align_label(spp, label, 3, gate).tolist() == [2, 2, 2, 2, 0, 0, 2]
    occ = np.ones((7, 2), bool)
    occ[0, 0] = False  # one point of superpoint 5 outside box 0: class 1 is masked there
    lab, prob = vote_ref.spp_major_voting(spp, label, np.full(7, 0.5, np.float32), occ, 3)
    assert lab.tolist() == [2, 2, 2, 2, 1, 1, 2]
    # class 2 of superpoint 5: mean 1.0 / (2 + 1e-4) times share 2 / 4, in float64, rounded once
    assert prob[0] == np.float32((1.0 / (2 + 1e-4)) * (2 / 4))
    assert prob[4] == np.float32((1.0 / (2 + 1e-4)) * (2 / 2))


def test_block_vote_rules():
    f32 = np.float32
    ok = [True, True]
    # an exact 2 : 2 tie between box 7 (first tester's b1) and box 3 (second tester's b1): the lower index, 3
    p = np.array([[.9, .9, .1, .1], [.2, .2, .8, .8]], f32)
    lab = np.zeros((2, 4), np.uint8)
    mu = np.array([[1, 2, 3, 4], [5, 6, 7, 9]], f32)
    r = vote_ref.vote_block(4, [(7, 9), (3, 8)], ok, p, lab, mu, mu)
    assert (r["box"], r["votes"], r["seg"], r["second"]) == (3, 2, 1, False)
    assert r["prob"] == f32(1.6 / 4) or abs(r["prob"] - 0.4) < 1e-7
    assert r["mu"] == f32(8.0)
    # one box argued by two fits: box 5 gets 3 + 2 votes against 4 for box 9; the representative is the fit with 3
    p = np.array([[.9] * 3 + [.1] * 2 + [.9] * 4, [.2] * 3 + [.8] * 2 + [.2] * 4], f32)
    lab = np.array([[0] * 5 + [1] * 4, [0] * 9], np.uint8)
    r = vote_ref.vote_block(9, [(5, 9), (5, 11)], ok, p, lab, p, p)
    assert (r["box"], r["votes"], r["seg"], r["second"]) == (5, 5, 0, False)
    # prob: ALL five voters for the box over the block's nine rows; mu: the representative's three voters alone
    assert abs(float(r["prob"]) - (3 * float(f32(.9)) + 2 * float(f32(.8))) / 9) < 1e-7 and r["mu"] == f32(.9)
    # a tie between representative fits: the earliest in tester order; label 1 voters -> second
    p = np.array([[.9, .9, .1, .1], [.2, .2, .8, .8]], f32)
    lab = np.array([[1] * 4, [0] * 4], np.uint8)
    r = vote_ref.vote_block(4, [(11, 5), (5, 9)], ok, p, lab, p, p)
    assert (r["box"], r["votes"], r["seg"], r["second"]) == (5, 4, 0, True)
    # a skipped model, NaN rows, nobody
    r = vote_ref.vote_block(4, [(11, 5), (5, 9)], [False, True], p, lab, p, p)
    assert (r["box"], r["votes"], r["seg"]) == (5, 4, 1)
    assert vote_ref.vote_block(4, [(11, 5)], [True], np.full((1, 4), np.nan, f32), lab, p, p) is None
    assert vote_ref.vote_block(4, [(11, 5)], [False], p[:1], lab, p, p) is None
    # a non-finite summand poisons that value alone
    mu = p.copy()
    mu[0, 0] = np.inf
    r = vote_ref.vote_block(4, [(11, 5), (5, 9)], ok, p, lab, mu, p)
    assert np.isnan(r["mu"]) and r["mu"].view(np.uint32) == 0x7fc00000 and np.isfinite(r["var"])


def test_point_vote_value_and_abi():
    assert point_mode("vote") == "vote"
    with pytest.raises(ValueError):
        point_mode("Vote")
    V = _lib.PointRefineVoteScene
    assert C.sizeof(V) == 48
    assert [getattr(V, f).offset for f, _ in V._fields_] == [0, 8, 16, 24, 32, 40, 44]
    lib = _lib.load()
    for name in ("gapro_spp_vote", "gapro_spp_vote_workspace_bytes", "gapro_point_refine_vote"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    # sizes the call would refuse have no workspace; the others hold the header, P, cnt, occn and the two tables
    assert lib.gapro_spp_vote_workspace_bytes(0, 1, 1) == 0 and lib.gapro_spp_vote_workspace_bytes(5, 6, 1) == 0
    assert lib.gapro_spp_vote_workspace_bytes(10, 3, -1) == 0 and lib.gapro_spp_vote_workspace_bytes(2 ** 31, 2 ** 30, 4) == 0
    assert lib.gapro_spp_vote_workspace_bytes(100, 10, 4) == 64 + 320 + 160 + 128 + 48 + 48
    # without a device there is no context: every call is refused before it looks at anything else
    z = np.zeros(64, np.int64)
    p = C.c_void_p(z.ctypes.data)
    assert lib.gapro_spp_vote(None, None, 0, 4, 2, 3, p, p, 0, p, p, p, 4096, p, p, p) == -1
    assert lib.gapro_spp_vote(None, None, 1, -4, -2, -3, None, None, 0, None, None, None, 0, None, None, None) == -1
    assert lib.gapro_spp_vote(None, None, 7, 0, 0, 0, None, None, 0, None, None, None, 0, None, None, None) == -1
    args = (1, p, p, 1, p, p, p, p, 1, p, p, p, p, 1, p, p)
    assert lib.gapro_point_refine_vote(None, None, *args, 10, 10, p, p, p, p, None, None) == -1
    assert lib.gapro_point_refine_vote(None, None, *args, 10, 2 ** 31, p, p, p, p, None, None) == -1
    assert lib.gapro_point_refine_vote(None, None, -1, None, None, -1, None, None, None, None, -1, None, None, None, None,
                                       -1, None, None, -1, -1, None, None, None, None, None, None) == -1
    # refused before a context is made
    with pytest.raises(ValueError):
        Pipeline(point_level="votes")


def test_cli_refuses_point_vote_beside_another_point_mode(tmp_path, capsys):
    from gapro_amd import gen_ps

    base = ["--save_folder", str(tmp_path / "out"), "--data_root", str(tmp_path), "--point_vote"]
    for other in ("--point_compete", "--point_level"):
        with pytest.raises(SystemExit) as e:
            gen_ps.main(base + [other])
        assert e.value.code == 2  # argparse's status
        assert "--point_vote cannot be combined" in capsys.readouterr().err
    assert not (tmp_path / "out").exists()
