"""csrc/posehead.hip stage by stage through the C ABI against the float64 reference of tests/posehead_ref.py: the softmax statistics,
the labels, the fine stage's row weights and soft correspondences, the CDF, every hypothesis (not only the winner), the candidate
scores and min_dist.  The cases are chosen for the kernels' boundaries (posehead_ref.CASES); what a comparison leaves out (near-tie
labels, draws on a CDF step, ill-conditioned 3-point rotations) is bounded on the reference alone in test_posehead_ref_cpu.py.

Each case runs every kernel once and computes the reference once (`run`); the tests assert on that record.  Output buffers start
as NaN, so an element that a kernel does not write fails its comparison."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import posehead_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu
ALL = list(P.CASES) + list(P.SPECIAL)
NCAND = 40
NULL = ctypes.c_void_p(None)
_runs = {}


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def maxerr(got, want):
    """max |got - want| in float64; NaN or inf in `got` is an error of its own."""
    got = got.detach().cpu().to(P.F64)
    assert torch.isfinite(got).all(), "non-finite output"
    return (got - want.to(P.F64)).abs().max().item() if got.numel() else 0.0


def maxrel(got, want):
    got, want = got.detach().cpu().to(P.F64), want.to(P.F64)
    assert torch.isfinite(got).all(), "non-finite output"
    return ((got - want).abs() / want.abs().clamp_min(1e-300)).max().item() if got.numel() else 0.0


def split_stats(stats, B, R, C):
    """[rmax B*R | 1/rsum B*R | cmax B*C | 1/csum B*C]"""
    s = stats.cpu()
    return (s[:B * R].view(B, R), s[B * R:2 * B * R].view(B, R), s[2 * B * R:2 * B * R + B * C].view(B, C),
            s[2 * B * R + B * C:].view(B, C))


def labels(x, s1, s2):
    from unopose_amd._lib import call, ptr, stream_ptr
    B, R, C = x.shape
    stats, w1, w2 = nan(2 * B * (R + C)), nan(B, R - 1), nan(B, C - 1)
    call("unopose_assign_labels", ptr(x), B, R, C, ptr(s1), ptr(s2), ptr(stats), ptr(w1), ptr(w2), stream_ptr())
    return stats, w1, w2


def fine(x, s1, s2, stats, w1, w2, q):
    from unopose_amd._lib import call, ptr, stream_ptr
    B, R, C = x.shape
    weight, pred = nan(B, R - 1), nan(B, R - 1, 3)
    call("unopose_fine_correspondences", ptr(x), B, R, C, ptr(s1), ptr(s2), ptr(stats), ptr(w1), ptr(w2), ptr(q), ptr(weight), ptr(pred),
         stream_ptr())
    return weight, pred


def coarse(x, s1, s2, stats, w1, w2, rand, nprop, p1, p2):
    from unopose_amd._lib import call, ptr, stream_ptr
    B, R, C = x.shape
    cdf, Rk, tk, dis = nan(B, (R - 1) * (C - 1)), nan(B, nprop, 3, 3), nan(B, nprop, 3), nan(B, nprop)
    call("unopose_coarse_hypotheses", ptr(x), B, R, C, ptr(s1), ptr(s2), ptr(stats), ptr(w1), ptr(w2), ptr(rand), nprop, ptr(p1),
         ptr(p2), ptr(cdf), ptr(Rk), ptr(tk), ptr(dis), stream_ptr())
    return cdf, Rk, tk, dis


def scores(p1, p2, Rk, tk, top, w1):
    from unopose_amd._lib import call, ptr, stream_ptr
    B, N1, N2 = p1.shape[0], p1.shape[1], p2.shape[1]
    sc = nan(B, top.shape[1])
    call("unopose_coarse_scores", ptr(p1), ptr(p2), B, N1, N2, ptr(Rk), ptr(tk), Rk.shape[1], ptr(top), top.shape[1], ptr(w1), ptr(sc),
         stream_ptr())
    return sc


def run(name):
    """Every kernel once on the case's inputs, and the reference of each stage on the same inputs.  Each later stage of the
    reference is fed the kernel's own output of the stage before (labels, CDF, poses), so a stage answers for itself alone."""
    if name in _runs:
        return _runs[name]
    from unopose_amd._lib import call, ptr, stream_ptr
    c = P.make_case(name)
    B, N1, N2, nprop = c["B"], c["N1"], c["N2"], c["nprop"]
    d = {k: c[k].cuda().contiguous() for k in ("atten", "score1", "score2", "p1", "p2", "rand")}
    x, s1, s2 = d["atten"], d["score1"], d["score2"]
    stats, w1, w2 = labels(x, s1, s2)
    stats_alone = nan(stats.numel())
    call("unopose_softmax_stats", ptr(x), B, N1 + 1, N2 + 1, ptr(stats_alone), stream_ptr())
    weight, pred = fine(x, s1, s2, stats, w1, w2, d["p2"])
    cdf, Rk, tk, dis = coarse(x, s1, s2, stats, w1, w2, d["rand"], nprop, d["p1"], d["p2"])
    # candidates: an unsorted slice of a random permutation that holds the first and the last hypothesis
    g = torch.Generator().manual_seed(nprop + N1)
    top = torch.stack([torch.randperm(nprop, generator=g)[:NCAND] for _ in range(B)])
    top[:, 3], top[:, NCAND - 2] = nprop - 1, 0
    topd = top.cuda().contiguous()
    sc = scores(d["p1"], d["p2"], Rk, tk, topd, w1)
    sc_zero = scores(d["p1"], d["p2"], Rk, tk, topd, torch.zeros_like(w1))
    w_any = 0.5 + torch.rand(B, N1, generator=g)  # every row counts, the last one too (the labels end in background rows)
    sc_any = scores(d["p1"], d["p2"], Rk, tk, topd, w_any.cuda())
    torch.cuda.synchronize()

    r = dict(case=c, dev=d, stats=split_stats(stats, B, N1 + 1, N2 + 1), stats_same=torch.equal(stats, stats_alone), w1=w1.cpu(),
             w2=w2.cpu(), weight=weight.cpu(), pred=pred.cpu(), cdf=cdf.cpu(), R=Rk.cpu(), t=tk.cpu(), dis=dis.cpu(), top=top,
             sc=sc.cpu(), sc_zero=sc_zero.cpu(), sc_any=sc_any.cpu(), w_any=w_any)
    r["ref_stats"] = P.stats(c["atten"])
    r["ref_labels"] = P.assignment(c["atten"], c["score1"], c["score2"])[1:]
    r["ref_fine"] = P.fine_rows(c["atten"], c["score1"], c["score2"], r["w1"], r["w2"], c["p2"])
    r["ref_cdf"] = P.cdf(c["atten"], c["score1"], c["score2"], r["w1"], r["w2"])
    r["ref_hyp"] = P.hypotheses(r["cdf"], c["rand"], c["p1"], c["p2"])
    Rc, tc = P.take(r["R"], r["t"], top)
    r["ref_sc"] = P.candidate_scores(c["p1"], c["p2"], Rc, tc, r["w1"])
    r["ref_sc_any"] = P.candidate_scores(c["p1"], c["p2"], Rc, tc, w_any)
    _runs[name] = r
    return r


@pytest.mark.parametrize("name", ALL)
def test_statistics(name):
    """rmax and cmax are selections: equal to the reference.  1/rsum and 1/csum within 2e-6 relative: every term is
    v_exp_f32((x - max) log2 e) at ~2 ulp plus the rounding of its argument, the largest term is exactly 1, and one reciprocal
    follows.  The same formula evaluated in fp32 on the CPU gives at most 4.9e-7.
    Measured on the MI355X: 1/rsum 2.6e-7, 1/csum 7.1e-7 (257x64, the longest columns).  unopose_softmax_stats
    writes the same bits as unopose_assign_labels."""
    r = run(name)
    rmax, irs, cmax, ics = r["stats"]
    rmax64, irs64, cmax64, ics64 = r["ref_stats"]
    assert torch.equal(rmax.double(), rmax64) and torch.equal(cmax.double(), cmax64)
    er, ec = maxrel(irs, irs64), maxrel(ics, ics64)
    print(f"{name}: 1/rsum max rel err {er:.2e}, 1/csum {ec:.2e}")
    assert er < 2e-6 and ec < 2e-6
    assert r["stats_same"]


@pytest.mark.parametrize("name", ALL)
def test_labels(name):
    """w1 and w2 are 0 or 1 and equal to the reference wherever the relative margin between the best foreground entry and the
    background entry exceeds 1e-4 (fp32 products of four factors carry ~1e-6).  Every margin of these cases is above 1e-4 (test_posehead_ref_cpu.py), so every label is compared."""
    r = run(name)
    w1r, w2r, m1, m2 = r["ref_labels"]
    for w, wr, m in ((r["w1"], w1r, m1), (r["w2"], w2r, m2)):
        assert ((w == 0) | (w == 1)).all()
        sure = m > P.MARGIN_MIN
        print(f"{name}: labels that differ {(w.double() != wr).sum().item()} of {w.numel()}, compared {sure.sum().item()}")
        assert torch.equal(w.double()[sure], wr[sure])
    if name == "allbg":
        assert (r["w1"][1] == 0).all() and (r["w2"][1] == 0).all()
        assert r["w1"][0].sum() > 0 and r["w1"][2].sum() > 0


@pytest.mark.parametrize("name", ALL)
def test_fine_rows(name):
    """weight within 1e-5 relative + 1e-12 absolute, pred within 1e-5 absolute where weight > 1e-3 (coordinates are O(1)),
    both exactly 0 on rows with w1 = 0 -- also where the kernel skips four background rows at once.  The error is that of one
    exponential per element whose argument 2 x log2 e - (rmax + cmax) log2 e is rounded at a magnitude of up to ~50.
    The same formula in fp32 on the CPU: weight 1.1e-6 relative (4.1e-6 in the spiked case), pred 3.3e-7.
    Measured on the MI355X: pred 1.3e-7; weight 4.2e-7 relative at 1x1.  For the other cases the run recorded only that no
    row exceeded the bound (largest excess 0.0); the test prints their relative error over the rows with weight > 1e-6."""
    r = run(name)
    weight64, pred64 = r["ref_fine"]
    ew = ((r["weight"].double() - weight64).abs() - 1e-5 * weight64).max().item()
    on = r["weight"] > 1e-3
    ep = maxerr(r["pred"][on], pred64[on])
    big = weight64 > 1e-6  # where the bound's absolute share is nothing
    print(f"{name}: weight max rel err {maxrel(r['weight'][big], weight64[big]):.2e} on {big.sum().item()} rows (excess over the bound {ew:.1e}), "
          f"pred max err {ep:.2e} on {on.sum().item()} rows")
    assert torch.isfinite(r["weight"]).all() and torch.isfinite(r["pred"]).all()
    assert ew <= 1e-12
    assert ep < 1e-5
    bg = r["w1"] == 0
    assert (r["weight"][bg] == 0).all() and (r["pred"][bg] == 0).all()
    if name not in ("allbg", "spiked"):
        assert on.sum().item() >= 0.5 * (r["w1"] == 1).sum().item() > 0  # the comparison of pred is not empty


@pytest.mark.parametrize("name", ALL)
def test_cdf(name):
    """The CDF is non-decreasing, ends at last / (last + 1e-8) and lies within 4e-6 absolute of the float64 CDF of the same labels.
    The 4e-6: an element (a w1 w2)^1.5 carries a relative error delta of ~9e-7 (two exponentials at 2 ulp, two reciprocals, five
    products, powf with exponent 1.5); a cumulative sum normalised by its own last element carries at most 2 delta, plus one
    rounding.  The same formula in fp32 on the CPU: at most 1.0e-7.
    Measured on the MI355X: 1.2e-7 (5x7), last element 1.5e-8.  An all-background element gives exactly 0 everywhere."""
    r = run(name)
    cdf = r["cdf"]
    cdf64, last = r["ref_cdf"]
    assert torch.isfinite(cdf).all()
    assert (cdf[:, 1:] >= cdf[:, :-1]).all() and (cdf >= 0).all() and (cdf <= 1).all()
    end = last / (last + 1e-8)
    # three fp32 roundings (the sum, the denominator, the quotient) and the elements' 2 delta through d end / d last
    e_end = (cdf[:, -1].double() - end).abs()
    e = maxerr(cdf, cdf64)
    print(f"{name}: cdf max err {e:.2e}, last element err {e_end.max().item():.2e}, last {last.tolist()}")
    assert (e_end <= 3 * 2.0 ** -24 + 2e-6 * 1e-8 / (last + 1e-8)).all()
    assert e < 4e-6
    if name == "allbg":
        assert (cdf[1] == 0).all()


@pytest.mark.parametrize("name", ALL)
def test_hypotheses(name):
    """Every hypothesis behind the kernel's own CDF (so the search and the solver answer for themselves, not for CDF rounding).
    On the kept ones (no draw within 2e-6 of a CDF step, sigma_2 / sigma_1 > 0.03): R and t within 1e-4, the project's
    Procrustes tolerance, and dis within 1e-6 (fp32 arithmetic on O(1) coordinates).  On all of them: R is a proper rotation to
    1e-4, and the residual recomputed in float64 from the kernel's R, t and the points the REFERENCE sampled equals the kernel's
    dis to 1e-6 -- which pins the sampled indices and the draw layout also where the rotation itself is ill-conditioned.
    Measured on the MI355X, largest over the cases: kept R 1.7e-6, t 5.1e-7, dis 2.1e-7; all: R R^T - I 1.6e-6, det - 1 1.5e-6,
    recomputed residual 4.2e-8.  Before kabsch_from_H (jacobi3.h) orthogonalised its second left vector twice, 5x7 gave
    R R^T - I = 2.2e-4 on hypotheses that drew one pair twice: H is then rank 1 up to rounding."""
    r = run(name)
    c, hyp = r["case"], r["ref_hyp"]
    keep = P.kept(hyp)
    Rk, tk, dis = r["R"], r["t"], r["dis"]
    eR, et, ed = maxerr(Rk[keep], hyp["R"][keep]), maxerr(tk[keep], hyp["t"][keep]), maxerr(dis[keep], hyp["dis"][keep])
    Rd = Rk.double()
    e_orth = maxerr(Rd @ Rd.transpose(2, 3), torch.eye(3).expand_as(Rd))
    e_det = (torch.det(Rd) - 1).abs().max().item()
    e_res = maxerr(dis, P.residual(hyp["P1"], hyp["P2"], Rd, tk.double()))
    print(f"{name}: kept {keep.sum().item()} of {keep.numel()}: R {eR:.2e} t {et:.2e} dis {ed:.2e}; all: orth {e_orth:.2e} "
          f"det {e_det:.2e} recomputed residual {e_res:.2e}")
    assert eR < 1e-4 and et < 1e-4 and ed < 1e-6
    assert e_orth < 1e-4 and e_det < 1e-4
    assert e_res < 1e-6
    if name != "1x1":  # the comparison on the kept is not empty (the shares are asserted on the CPU); 1x1 can keep none
        assert keep.sum().item() >= 50
    if name == "spiked":  # in the element whose row and column are only lowered
        assert keep[2].sum().item() >= 50
    if name == "allbg":  # an all-zero CDF: every draw lands on idx = L, i.e. on points (N1 - 1, 0)
        assert (hyp["idx"][1] == c["N1"] * c["N2"]).all()


@pytest.mark.parametrize("name", ["5x7", "37x53"])
def test_draws_on_cdf_steps(name):
    """searchsorted takes the FIRST index with cdf >= u.  Random draws never meet a CDF value, so here every draw IS one: the
    kernel's own fp32 CDF at random indices (the CDF has flat runs wherever a label is 0, so most of these values occur more than
    once and `first` matters), u = 0 and the CDF's last value.  Such hypotheses are not `kept`; the residual recomputed from the
    kernel's R, t and the points the reference sampled pins the indices, to 1e-6 as in test_hypotheses."""
    r = run(name)
    c, d = r["case"], r["dev"]
    B, N1, N2, nprop = c["B"], c["N1"], c["N2"], c["nprop"]
    g = torch.Generator().manual_seed(N2)
    at = torch.randint(0, N1 * N2, (B, 3 * nprop), generator=g)
    rand = torch.gather(r["cdf"], 1, at)
    rand[:, 0], rand[:, 1] = 0.0, r["cdf"][:, -1]
    at[:, :2] = N1 * N2 - 1  # where those two can land at the latest
    assert (torch.gather(r["cdf"], 1, (at - 1).clamp(min=0)) == rand).float().mean() > 0.3  # flat runs are met
    stats = torch.cat([x.reshape(-1) for x in r["stats"]]).cuda()
    cdf, Rk, tk, dis = coarse(d["atten"], d["score1"], d["score2"], stats, r["w1"].cuda(), r["w2"].cuda(), rand.cuda().contiguous(),
                              nprop, d["p1"], d["p2"])
    torch.cuda.synchronize()
    assert torch.equal(cdf.cpu(), r["cdf"])
    hyp = P.hypotheses(r["cdf"], rand, c["p1"], c["p2"])
    assert (hyp["idx"] <= at).all() and (hyp["idx"] < at).float().mean() > 0.3
    e_res = maxerr(dis, P.residual(hyp["P1"], hyp["P2"], Rk.cpu().double(), tk.cpu().double()))
    print(f"{name}: draws on CDF values: recomputed residual {e_res:.2e}")
    assert e_res < 1e-6


@pytest.mark.parametrize("name", ALL)
def test_candidate_scores(name):
    """score[b, c] for an unsorted candidate list that holds hypothesis 0 and nprop - 1, within 1e-5 relative of the float64 score
    of the kernel's own R, t and labels; exactly 0 with w1 = 0 everywhere (0 / (0 + 1e-8)), as for an all-background element.
    1x1 has a bound of its own: with one point and the one pose that maps it onto its partner, the denominator
    D = |(p1 - t) R - p2| is 3e-6 of deliberate slack (the 1e-5 in the Procrustes weights) plus fp32 rounding of O(1)
    coordinates, so the score 1 / (D + 1e-8) has no 1e-5 relative meaning; there D itself is within 2e-7: a few roundings of
    coordinates of up to 1.3, at 6e-8 each.
    The same with weights of 0.5..1.5 on every row: the labels of these cases end in background rows, which alone would leave
    the last rows of the sum unseen.
    Measured on the MI355X: 2.6e-6 (5x7), 4.5e-7 at 196x196; the denominator of 1x1 within 6.5e-10."""
    r = run(name)
    sc, want = r["sc"], r["ref_sc"]
    assert torch.isfinite(sc).all()
    assert (r["sc_zero"] == 0).all()
    sc_any, want_any = r["sc_any"], r["ref_sc_any"]
    assert torch.isfinite(sc_any).all() and (want_any > 0).all()
    if name == "1x1":
        assert (r["w1"] == 1).all()
        for got, ref, W in ((sc, want, 1.0), (sc_any, want_any, r["w_any"].double().sum(1, keepdim=True))):
            e = (W / got.double() - W / ref).abs().max().item()
            print(f"{name}: denominator max err {e:.2e}")
            assert e < 2e-7
        return
    e = ((sc.double() - want).abs() / want.clamp_min(1e-300))[want > 0]
    e_any = maxrel(sc_any, want_any)
    print(f"{name}: score max rel err {e.max().item():.2e}, with weights on every row {e_any:.2e}")
    assert (sc[want == 0] == 0).all()
    assert e.max().item() < 1e-5 and e_any < 1e-5
    if name == "allbg":
        assert (sc[1] == 0).all()


@pytest.mark.parametrize("name", ["37x53", "130x70"])
def test_weights_enter_as_factors(name):
    """A_ij = a_ij w1_i w2_j with the weights as the ABI gives them, factors and not switches: with weights of 0, 0.5, 1 and 2
    the fine rows, the CDF and the candidate scores follow the reference at the tolerances of the 0/1 case."""
    r = run(name)
    c, d = r["case"], r["dev"]
    B, N1, N2, nprop = c["B"], c["N1"], c["N2"], c["nprop"]
    g = torch.Generator().manual_seed(N1)
    vals = torch.tensor([0.0, 0.5, 1.0, 2.0])
    w1 = vals[torch.randint(0, 4, (B, N1), generator=g)] * r["w1"]
    w2 = vals[torch.randint(0, 4, (B, N2), generator=g)] * r["w2"]
    from unopose_amd._lib import call, ptr, stream_ptr
    stats = nan(2 * B * (N1 + N2 + 2))
    call("unopose_softmax_stats", ptr(d["atten"]), B, N1 + 1, N2 + 1, ptr(stats), stream_ptr())
    w1d, w2d = w1.cuda(), w2.cuda()
    weight, pred = fine(d["atten"], d["score1"], d["score2"], stats, w1d, w2d, d["p2"])
    cdf, Rk, tk, _ = coarse(d["atten"], d["score1"], d["score2"], stats, w1d, w2d, d["rand"], nprop, d["p1"], d["p2"])
    sc = scores(d["p1"], d["p2"], Rk, tk, r["top"].cuda(), w1d)
    torch.cuda.synchronize()
    weight64, pred64 = P.fine_rows(c["atten"], c["score1"], c["score2"], w1, w2, c["p2"])
    assert ((weight.cpu().double() - weight64).abs() <= 1e-5 * weight64 + 1e-12).all()
    on = weight.cpu() > 1e-3
    assert maxerr(pred.cpu()[on], pred64[on]) < 1e-5
    assert maxerr(cdf, P.cdf(c["atten"], c["score1"], c["score2"], w1, w2)[0]) < 4e-6
    Rc, tc = P.take(Rk.cpu(), tk.cpu(), r["top"])
    assert maxrel(sc, P.candidate_scores(c["p1"], c["p2"], Rc, tc, w1)) < 1e-5


def test_min_dist():
    """min_j |p'_i - q_j| within 1e-6 of float64 (direct differences of O(1) coordinates in fp32), with a transform per candidate
    (cand_per_b = 3) and without one (R = t = null); N = 300 is no multiple of the 256 points of a block, M = 53 of nothing.
    Measured on the MI355X: 7.4e-8 with a transform, 2.3e-8 without."""
    from unopose_amd._lib import call, ptr, stream_ptr
    g = torch.Generator().manual_seed(3)
    B, N, M, K = 2, 300, 53, 3
    p, q = torch.rand(B, N, 3, generator=g) - 0.5, torch.rand(B, M, 3, generator=g) - 0.5
    Rm, t = P.random_pose(B * K, g)
    pd, qd, Rd, td = p.cuda(), q.cuda(), Rm.cuda().contiguous(), t.cuda().contiguous()
    out, plain = nan(B * K, N), nan(B, N)
    call("unopose_min_dist", ptr(pd), ptr(qd), B, N, M, ptr(Rd), ptr(td), K, ptr(out), stream_ptr())
    call("unopose_min_dist", ptr(pd), ptr(qd), B, N, M, NULL, NULL, 1, ptr(plain), stream_ptr())
    torch.cuda.synchronize()
    e1, e2 = maxerr(out, P.min_dist(p, q, Rm, t, K)), maxerr(plain, P.min_dist(p, q))
    print(f"min_dist: with a transform {e1:.2e}, without {e2:.2e}")
    assert e1 < 1e-6 and e2 < 1e-6


def test_documented_refusals():
    """Sizes whose points do not fit the LDS, and a transform given by half, raise the ABI's error and launch nothing: the
    output keeps its NaN.  The buffers have the sizes the arguments state."""
    from unopose_amd._lib import call, ptr, stream_ptr
    M = 64 * 1024 // 12 + 1  # M * 12 > 64 KiB
    p, q, eye, zero, out = nan(1, 8, 3), nan(1, M, 3), torch.eye(3, device="cuda").reshape(1, 3, 3), torch.zeros(1, 3, device="cuda"), nan(1, 8)
    with pytest.raises(RuntimeError, match="min_dist: bad sizes"):
        call("unopose_min_dist", ptr(p), ptr(q), 1, 8, M, NULL, NULL, 1, ptr(out), stream_ptr())
    with pytest.raises(RuntimeError, match="min_dist: null pointer"):
        call("unopose_min_dist", ptr(p), ptr(q), 1, 8, 16, ptr(eye), NULL, 1, ptr(out), stream_ptr())
    with pytest.raises(RuntimeError, match="min_dist: null pointer"):
        call("unopose_min_dist", ptr(p), ptr(q), 1, 8, 16, NULL, ptr(zero), 1, ptr(out), stream_ptr())
    n2 = 60 * 1024 // 12 + 1  # n2 * 12 > 60 KiB
    p2, top, w1, sc = nan(1, n2, 3), torch.zeros(1, 1, dtype=torch.int64, device="cuda"), torch.ones(1, 8, device="cuda"), nan(1, 1)
    with pytest.raises(RuntimeError, match="coarse_scores: bad sizes"):
        call("unopose_coarse_scores", ptr(p), ptr(p2), 1, 8, n2, ptr(eye), ptr(zero), 1, ptr(top), 1, ptr(w1), ptr(sc), stream_ptr())
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(sc).all()


@pytest.mark.parametrize("name", ["37x53", "130x70"])
def test_coarse_pose_end_to_end(name):
    """ops.coarse_pose with unequal counts: the second cloud's overlap scores are score[:, N1:].  The winner equals the float64
    chain's to 1e-4 and is the pose the clouds were built with (rotation within 2e-2: 3 mm of noise on three points ~0.5 apart).
    Measured on the MI355X: R 4.5e-7 and t 7.5e-8 from the float64 chain, 3.4e-3 from the pose of the clouds."""
    from unopose_amd import ops
    c = P.make_case(name)
    ncand = 300
    score = torch.cat((c["score1"], c["score2"]), 1)
    Rh, th, _ = ops.coarse_pose(c["atten"].cuda(), score.cuda(), c["p1"].cuda(), c["p2"].cuda(), c["rand"].cuda(), c["nprop"], ncand)
    R64, t64, _, _ = P.coarse_chain(c["atten"], c["score1"], c["score2"], c["p1"], c["p2"], c["rand"], c["nprop"], ncand)
    eR, et, eg = maxerr(Rh, R64), maxerr(th, t64), maxerr(Rh, c["R_gt"])
    print(f"{name}: coarse_pose vs the float64 chain R {eR:.2e} t {et:.2e}; vs the pose of the clouds {eg:.2e}")
    assert eR < 1e-4 and et < 1e-4
    assert eg < 2e-2
    Rt, tt, _ = ops.coarse_pose_torch(c["atten"].cuda(), score.cuda(), c["p1"].cuda(), c["p2"].cuda(), c["rand"].cuda(), c["nprop"], ncand)
    assert maxerr(Rt, R64) < 1e-4 and maxerr(tt, t64) < 1e-4
