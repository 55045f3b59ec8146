"""CPU: the float64 reference of the pose-head stages (tests/posehead_ref.py) against the reference's own fixture, against the fp32
oracle, and the conditions under which test_posehead_stages_gpu.py compares labels and hypotheses, on the inputs it uses."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import posehead_ref as P  # noqa: E402
from oracle import unopose_ref as O  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def err(a, b):
    return (a.double() - b.double()).abs().max().item()


def test_coarse_rt_fixture():
    """On the reference's recorded run (B = 2, 196 x 196, 6000 hypotheses): the float64 chain, its CDF cast to fp32 before the
    search as the reference searches an fp32 CDF, reproduces the 36000 sampled indices except for draws within 2e-6 of a CDF step
    (which side of a step such a draw falls on depends on the CDF's rounding), fewer than 0.5 % of them, and the winning pose."""
    z = np.load(os.path.join(GOLD, "coarse_rt.npz"))
    z = {k: torch.from_numpy(z[k]) for k in z.files if z[k].ndim}
    N1 = z["p1"].shape[1]
    Rm, tm, _, det = P.coarse_chain(z["atten"], z["score"][:, :N1], z["score"][:, N1:], z["p1"], z["p2"], z["rand"], 6000, 300)
    hyp = det["hyp"]
    near = P.near_step(det["cdf"].float(), z["rand"], hyp["idx"])
    differ = hyp["idx"] != z["hyp_idx"].long()
    print(f"draws near a step: {near.float().mean().item():.4%}; indices that differ: {differ.sum().item()}")
    assert not (differ & ~near).any()
    assert near.float().mean().item() < 5e-3
    assert err(Rm, z["R"]) < 1e-4 and err(tm, z["t"]) < 1e-4, (err(Rm, z["R"]), err(tm, z["t"]))


@pytest.mark.parametrize("name", ["196x196", "37x53"])
def test_agrees_with_the_fp32_oracle(name):
    """Stage by stage against oracle.unopose_ref (fp32, the reference's formulation) on a square and a non-square case."""
    c = P.make_case(name)
    score = torch.cat((c["score1"], c["score2"]), 1)
    nprop, ncand = c["nprop"], 100
    Ro, to, so, det = O.compute_coarse_rt_overlap(c["atten"], score, c["p1"], c["p2"], c["rand"], nprop, ncand, detail=True)
    _, w1, w2, _, _ = P.assignment(c["atten"], c["score1"], c["score2"])
    assert torch.equal(w1.float(), det["w1"])
    cdf64, _ = P.cdf(c["atten"], c["score1"], c["score2"], w1, w2)
    # fp32 elements (relative error ~1e-6 each after ~10 fp32 operations and a pow) summed by torch's cumsum
    assert err(cdf64, det["cs"]) < 4e-6
    hyp = P.hypotheses(det["cs"], c["rand"], c["p1"], c["p2"])  # behind the oracle's own CDF: the same indices
    assert torch.equal(hyp["idx"], det["idx"])
    keep = P.kept(hyp)
    assert err(hyp["dis"][keep], det["dis"][keep]) < 1e-6  # fp32 Procrustes residual of O(1) points
    assert err(hyp["R"][keep], det["rs"][keep]) < 1e-4 and err(hyp["t"][keep], det["ts"].squeeze(2)[keep]) < 1e-4
    # scores on the oracle's own candidates.  Its distances come from |a|^2 + |b|^2 - 2 a.b in fp32: ~1e-7 of absolute noise on
    # d^2 ~ 1e-5 (the 3 mm the clouds were built with), i.e. ~1 % of d -> 2 % relative, as for the fixture in test_model_gpu.py
    Rc, tc = P.take(det["rs"], det["ts"].squeeze(2), det["top"])
    sc = P.candidate_scores(c["p1"], c["p2"], Rc, tc, w1)
    assert ((sc - det["sc"]).abs() / sc).max().item() < 2e-2
    Rm, tm, _, _ = P.coarse_chain(c["atten"], c["score1"], c["score2"], c["p1"], c["p2"], c["rand"], nprop, ncand)
    assert err(Rm, Ro) < 1e-4 and err(tm, to) < 1e-4
    assert err(Rm, c["R_gt"]) < 2e-2
    # fine stage
    Rf, tf, sf = P.fine_chain(c["atten"], c["score1"], c["score2"], c["p1"], c["p2"])
    Rfo, tfo, sfo = O.compute_fine_rt_overlap(c["atten"], score, c["p1"], c["p2"])
    assert err(Rf, Rfo) < 1e-4 and err(tf, tfo) < 1e-4 and err(sf, sfo) < 1e-5
    assert err(Rf, c["R_gt"]) < 2e-2


def test_oracle_takes_the_second_scores_from_n1():
    """With N1 != N2 the oracle takes the second cloud's scores from column N1 on (the reference's `N2:` is the same slice only
    for equal counts): its CDF is the float64 one of (score1, score2), also after column N1, the second cloud's first score and
    one that `N2:` would skip here, is halved."""
    c = P.make_case("5x7")
    N1 = c["N1"]
    score = torch.cat((c["score1"], c["score2"]), 1)
    moved = score.clone()
    moved[:, N1] *= 0.5
    cdfs = []
    for s in (score, moved):
        det = O.compute_coarse_rt_overlap(c["atten"], s, c["p1"], c["p2"], c["rand"], c["nprop"], 50, detail=True)[3]
        _, w1, w2, _, _ = P.assignment(c["atten"], s[:, :N1], s[:, N1:])
        assert err(P.cdf(c["atten"], s[:, :N1], s[:, N1:], w1, w2)[0], det["cs"]) < 4e-6
        cdfs.append(det["cs"])
    assert err(cdfs[0], cdfs[1]) > 1e-3  # the halved score is read


def test_coarse_pose_refuses_a_score_of_the_wrong_width():
    """Both coarse_pose and its torch composite take score as (B, N1 + N2) and say so before anything is launched (the tensors
    here are on the CPU: nothing could be)."""
    from unopose_amd import ops
    c = P.make_case("5x7")
    score = torch.cat((c["score1"], c["score2"]), 1)
    for f in (ops.coarse_pose, ops.coarse_pose_torch):
        for bad in (score[:, :-1], torch.cat((score, score[:, :1]), 1), score[:, :c["N1"]], score[0]):
            with pytest.raises(ValueError, match=r"N1 \+ N2"):
                f(c["atten"], bad, c["p1"], c["p2"], c["rand"], c["nprop"], 50)


def _conditions(name):
    c = P.make_case(name)
    _, w1, w2, m1, m2 = P.assignment(c["atten"], c["score1"], c["score2"])
    cdf64, _ = P.cdf(c["atten"], c["score1"], c["score2"], w1, w2)
    hyp = P.hypotheses(cdf64.float(), c["rand"], c["p1"], c["p2"])
    low = ((m1 <= P.MARGIN_MIN).sum() + (m2 <= P.MARGIN_MIN).sum()).item() / (m1.numel() + m2.numel())
    return c, low, P.kept(hyp), hyp


@pytest.mark.parametrize("name", list(P.CASES) + list(P.SPECIAL))
def test_gpu_comparison_conditions(name):
    """What the GPU tests leave out of a comparison is bounded here, on the reference alone.  Labels are compared where the
    relative margin exceeds 1e-4: at most 1 % of rows and columns may fall below.  R and t of a hypothesis are compared where no
    draw is within 2e-6 of a CDF step and sigma_2 / sigma_1 > 0.03 for H: at least 75 % of the hypotheses must be kept.
    Caps of their own, because of what the case is and not of what a kernel does with it:
      * 5x7: 4 matched pairs per element, so the same pair is often drawn twice in a hypothesis (rank <= 1): at least 20 % kept and
        at least 50 hypotheses in absolute number.
      * 1x1: one pair; every hypothesis is three times the same point, H = 0, none is kept.  The case is there for the
        statistics, labels, CDF and the checks made on all hypotheses.
      * allbg: the cap holds on the ordinary elements 0 and 2; element 1 has an all-zero CDF and keeps none.
      * spiked: a row or column raised by 30 concentrates the CDF on that one row (element 0) or column (element 1), so every
        hypothesis there draws pairs that share a point and none is kept; they are checked by the all-hypotheses assertions.
        The cap holds on element 2, where a row and a column are only lowered."""
    c, low, keep, hyp = _conditions(name)
    share = keep.float().mean().item()
    print(f"{name}: rows+cols under the margin {low:.3%}; hypotheses kept {share:.1%} ({int(keep.sum())}); near a step "
          f"{hyp['near'].float().mean().item():.3%}")
    assert low <= 0.01
    if name == "5x7":
        assert share >= 0.20 and keep.sum().item() >= 50
    elif name == "1x1":
        assert keep.sum().item() == 0
    elif name == "allbg":
        assert keep[[0, 2]].float().mean().item() >= 0.75 and keep[1].sum().item() == 0
        assert (hyp["idx"][1] == c["N1"] * c["N2"]).all()  # every draw lands past the end of an all-zero CDF
        assert (hyp["i1"][1] == c["N1"] - 1).all() and (hyp["i2"][1] == 0).all()
    elif name == "spiked":
        assert keep[2].float().mean().item() >= 0.75 and keep[:2].sum().item() == 0
    else:
        assert share >= 0.75


def test_reference_stages_are_consistent():
    """The stages against each other and against closed forms: softmax statistics rebuild a; weights and the CDF's last element
    are sums of the same masked matrix; min_dist with a transform equals the residual of the hypothesis that made it."""
    c = P.make_case("37x53")
    x, s1, s2 = c["atten"], c["score1"], c["score2"]
    rmax, irs, cmax, ics = P.stats(x)
    a, w1, w2, _, _ = P.assignment(x, s1, s2)
    xd = x.double()
    rebuilt = torch.exp(xd - rmax[:, :, None]) * irs[:, :, None] * torch.exp(xd - cmax[:, None, :]) * ics[:, None, :]
    rebuilt[:, 1:, :] *= s1.double()[:, :, None]
    rebuilt[:, :, 1:] *= s2.double()[:, None, :]
    assert err(rebuilt, a) < 1e-14
    weight, pred = P.fine_rows(x, s1, s2, w1, w2, c["p2"])
    assert (weight[w1 == 0] == 0).all() and (pred[w1 == 0] == 0).all()
    cdf64, last = P.cdf(x, s1, s2, w1, w2)
    assert (cdf64[:, 1:] >= cdf64[:, :-1]).all() and err(cdf64[:, -1], last / (last + 1e-8)) < 1e-15
    hyp = P.hypotheses(cdf64.float(), c["rand"], c["p1"], c["p2"])
    Rm = hyp["R"]
    assert err(Rm @ Rm.transpose(2, 3), torch.eye(3).expand_as(Rm)) < 1e-12 and err(torch.det(Rm), torch.ones(Rm.shape[:2])) < 1e-12
    # three congruent points are fitted to the noise they carry
    keep = P.kept(hyp)
    assert hyp["dis"][keep].max().item() < 0.02
    d = P.min_dist(c["p1"], c["p2"], Rm[:, :3].reshape(-1, 3, 3), hyp["t"][:, :3].reshape(-1, 3), cand_per_b=3)
    assert d.shape == (c["B"] * 3, c["N1"])
    plain = P.min_dist(c["p1"], c["p2"])
    brute = (c["p1"].double()[:, :, None] - c["p2"].double()[:, None]).norm(dim=3).amin(2)
    assert err(plain, brute) < 1e-15
