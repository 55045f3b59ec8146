"""Float64 reference of the pose-head stages of csrc/posehead.hip, one plain function per stage, written from the notation in that
file's header (x = atten (B,R,C), row / column 0 = the background token):

    a_ij = softmax_row(x)_ij * softmax_col(x)_ij * s1_i * s2_j                    (s1_0 = s2_0 = 1)
    w1_i = [max_{j>=1} a_ij > a_i0]  (i >= 1),   w2_j = [max_{i>=1} a_ij > a_0j]  (j >= 1)

Everything is torch on the CPU in float64 and materialises what the kernels stream.  Nothing here is used by the package; the tests
of the kernels (test_posehead_stages_gpu.py) compare against it and test_posehead_ref_cpu.py checks it against the fixtures and the
fp32 oracle.  The generator of the test problems, `constructed_case`, and the list of cases are here too, so that the conditions
under which the GPU tests compare (label margins, kept hypotheses) are checked on the same inputs without a GPU."""
import torch

F64 = torch.float64
STEP_EPS = 2e-6   # a draw closer than this to a CDF step may legitimately land on either side of it
SIGMA_MIN = 0.03  # sigma_2 / sigma_1 of H below which a 3-point rotation is ill-conditioned
MARGIN_MIN = 1e-4  # relative margin below which a label is a near-tie


# ------------------------------------------------------------------------------------------------------------ stages
def stats(atten):
    """Row and column softmax statistics: rmax (B,R), 1 / sum_j exp(x_ij - rmax_i), cmax (B,C), 1 / sum_i exp(x_ij - cmax_j)."""
    x = atten.to(F64)
    rmax, cmax = x.amax(2), x.amax(1)
    irs = 1.0 / torch.exp(x - rmax[:, :, None]).sum(2)
    ics = 1.0 / torch.exp(x - cmax[:, None, :]).sum(1)
    return rmax, irs, cmax, ics


def _with_one(s):
    return torch.cat((torch.ones(s.shape[0], 1, dtype=F64), s.to(F64)), 1)


def soft_assignment(atten, s1, s2):
    """The full a (B,R,C)."""
    x = atten.to(F64)
    return torch.softmax(x, 2) * torch.softmax(x, 1) * _with_one(s1)[:, :, None] * _with_one(s2)[:, None, :]


def assignment(atten, s1, s2):
    """a, the labels w1 (B,R-1), w2 (B,C-1) (first-index argmax: the background, index 0, wins a tie) and the relative margin
    |fg - bg| / max(fg, bg) between each row's / column's best foreground entry and its background entry: what decides a label."""
    a = soft_assignment(atten, s1, s2)
    fg1, bg1 = a[:, 1:, 1:].amax(2), a[:, 1:, 0]
    fg2, bg2 = a[:, 1:, 1:].amax(1), a[:, 0, 1:]
    w1, w2 = (fg1 > bg1).to(F64), (fg2 > bg2).to(F64)
    m1 = (fg1 - bg1).abs() / torch.maximum(fg1, bg1).clamp_min(1e-300)
    m2 = (fg2 - bg2).abs() / torch.maximum(fg2, bg2).clamp_min(1e-300)
    return a, w1, w2, m1, m2


def _masked(atten, s1, s2, w1, w2):
    return soft_assignment(atten, s1, s2)[:, 1:, 1:] * w1.to(F64)[:, :, None] * w2.to(F64)[:, None, :]


def fine_rows(atten, s1, s2, w1, w2, pts2):
    """A_ij = a_ij w1_i w2_j;  weight_i = sum_j A_ij;  pred_i = sum_j A_ij q_j / (weight_i + 1e-6)."""
    A = _masked(atten, s1, s2, w1, w2)
    weight = A.sum(2)
    pred = (A @ pts2.to(F64)) / (weight + 1e-6)[:, :, None]
    return weight, pred


def cdf(atten, s1, s2, w1, w2):
    """Cumulative sum of (a w1 w2)^1.5 over the foreground block, row-major, divided by last + 1e-8.  Returns (cdf (B,L), last (B,))."""
    ps = _masked(atten, s1, s2, w1, w2).reshape(atten.shape[0], -1) ** 1.5
    cs = torch.cumsum(ps, 1)
    last = cs[:, -1]
    return cs / (last[:, None] + 1e-8), last


def procrustes(src, ref, w=None, thresh=0.0, eps=1e-5):
    """Weighted Procrustes, ref ~ R src + t, for src, ref (M,n,3): weights below `thresh` dropped, normalised by sum + eps;
    H = sum w (src - sc)(ref - rc)^T = U S V^T, R = V diag(1, 1, det(V U^T)) U^T, t = rc - R sc.  Returns R, t, S."""
    src, ref = src.to(F64), ref.to(F64)
    w = torch.ones(src.shape[:2], dtype=F64) if w is None else w.to(F64)
    w = torch.where(w < thresh, torch.zeros_like(w), w)
    w = (w / (w.sum(1, keepdim=True) + eps))[:, :, None]
    sc, rc = (src * w).sum(1, keepdim=True), (ref * w).sum(1, keepdim=True)
    H = (src - sc).transpose(1, 2) @ (w * (ref - rc))
    U, S, Vh = torch.linalg.svd(H)
    V = Vh.transpose(1, 2)
    D = torch.eye(3, dtype=F64).repeat(src.shape[0], 1, 1)
    D[:, 2, 2] = torch.sign(torch.det(V @ U.transpose(1, 2)))
    Rm = V @ D @ U.transpose(1, 2)
    t = (rc.transpose(1, 2) - Rm @ sc.transpose(1, 2)).squeeze(2)
    return Rm, t, S


def near_step(cdf_f32, rand, idx):
    """Per draw: u lies within STEP_EPS of the CDF value on either side of its index idx = searchsorted(cdf, u)."""
    L = cdf_f32.shape[1]
    c, u = cdf_f32.to(F64), rand.to(F64)
    at = torch.gather(c, 1, idx.clamp(max=L - 1))
    before = torch.gather(c, 1, (idx - 1).clamp(min=0))
    return ((idx < L) & ((at - u).abs() < STEP_EPS)) | ((idx > 0) & ((u - before).abs() < STEP_EPS))


def take(Rm, t, top):
    """The poses R (B,n,3,3), t (B,n,3) of the candidates top (B,K)."""
    return (torch.gather(Rm, 1, top[:, :, None, None].expand(-1, -1, 3, 3)), torch.gather(t, 1, top[:, :, None].expand(-1, -1, 3)))


def hypotheses(cdf_f32, rand, p1, p2):
    """The coarse stage behind a given fp32 CDF (B,N1*N2): draw d = 3 h + c of rand (B,3*nprop) is point c of hypothesis h;
    idx = searchsorted(cdf, u) (first index with cdf >= u), i1 = min(idx // N2, N1-1), i2 = min(idx % N2, N2-1); a 3-point
    Procrustes p1 ~ R p2 + t with weights 1/(3 + 1e-5) and dis = mean_c |(p1_c - t) R - p2_c|.
    `near`: some draw of the hypothesis lies within STEP_EPS of the CDF value on either side of its index."""
    assert cdf_f32.dtype == torch.float32 and rand.dtype == torch.float32
    B, N1, N2 = p1.shape[0], p1.shape[1], p2.shape[1]
    nprop = rand.shape[1] // 3
    idx = torch.searchsorted(cdf_f32.contiguous(), rand.contiguous())
    i1 = torch.clamp(idx // N2, max=N1 - 1)
    i2 = torch.clamp(idx % N2, max=N2 - 1)
    P1 = torch.gather(p1.to(F64), 1, i1[:, :, None].expand(-1, -1, 3)).reshape(B, nprop, 3, 3)
    P2 = torch.gather(p2.to(F64), 1, i2[:, :, None].expand(-1, -1, 3)).reshape(B, nprop, 3, 3)
    Rm, t, S = procrustes(P2.reshape(-1, 3, 3), P1.reshape(-1, 3, 3))
    Rm, t, S = Rm.reshape(B, nprop, 3, 3), t.reshape(B, nprop, 3), S.reshape(B, nprop, 3)
    dis = residual(P1, P2, Rm, t)
    near = near_step(cdf_f32, rand, idx)
    return dict(idx=idx, i1=i1, i2=i2, P1=P1, P2=P2, R=Rm, t=t, S=S, dis=dis, near=near.reshape(B, nprop, 3).any(2))


def residual(P1, P2, Rm, t):
    """mean_c |(p1_c - t) R - p2_c| for sampled points (B,n,3,3) and poses R (B,n,3,3), t (B,n,3), all float64."""
    return ((P1 - t.to(F64)[:, :, None, :]) @ Rm.to(F64) - P2).norm(dim=3).mean(2)


def kept(hyp):
    """The hypotheses on which R and t are compared: no draw near a CDF step and a well-conditioned H."""
    S = hyp["S"]
    return (~hyp["near"]) & (S[..., 1] > SIGMA_MIN * S[..., 0])


def _nearest(moved, q):
    return torch.cdist(moved, q, compute_mode="donot_use_mm_for_euclid_dist").amin(-1)


def candidate_scores(p1, p2, Rm, t, w1):
    """sum_i w1_i / (sum_i w1_i min_j |(p1_i - t) R - p2_j| + 1e-8) for candidate poses R (B,K,3,3), t (B,K,3) -> (B,K)."""
    p1, p2, w1 = p1.to(F64), p2.to(F64), w1.to(F64)
    out = []
    for b in range(p1.shape[0]):
        moved = (p1[b][None] - t[b].to(F64)[:, None, :]) @ Rm[b].to(F64)  # (K,N1,3)
        d = _nearest(moved, p2[b][None].expand(moved.shape[0], -1, -1))
        out.append(w1[b].sum() / ((d * w1[b][None]).sum(1) + 1e-8))
    return torch.stack(out)


def min_dist(p, q, Rm=None, t=None, cand_per_b=1):
    """out[b * cand_per_b + c, i] = min_j |p'_i - q_j|, p' = (p_i - t_bc) R_bc with a transform (R (B*cand,3,3), t (B*cand,3)),
    p' = p without one."""
    p, q = p.to(F64), q.to(F64)
    pp = p.repeat_interleave(cand_per_b, 0)
    if Rm is not None:
        pp = (pp - t.to(F64)[:, None, :]) @ Rm.to(F64)
    return _nearest(pp, q.repeat_interleave(cand_per_b, 0))


# ------------------------------------------------------------------------------------------------------------ chains
def coarse_chain(atten, s1, s2, p1, p2, rand, nprop, ncand):
    """The whole coarse stage: labels, CDF (cast to fp32 before the search, as the reference searches an fp32 CDF), hypotheses,
    the `ncand` smallest residuals, their scores, the first best one.  Returns R (B,3,3), t (B,3), score (B,) and the stages."""
    _, w1, w2, _, _ = assignment(atten, s1, s2)
    c, _ = cdf(atten, s1, s2, w1, w2)
    hyp = hypotheses(c.float(), rand.float(), p1, p2)
    top = torch.topk(hyp["dis"], ncand, dim=1, largest=False)[1]
    Rc, tc = take(hyp["R"], hyp["t"], top)
    sc = candidate_scores(p1, p2, Rc, tc, w1)
    score, best = sc.max(1)
    bi = torch.arange(atten.shape[0])
    return Rc[bi, best], tc[bi, best], score, dict(w1=w1, w2=w2, cdf=c, hyp=hyp, top=top, sc=sc, best=best)


def fine_chain(atten, s1, s2, p1, p2, dis_thres=0.15):
    """The whole fine stage: labels, soft correspondences, weighted Procrustes (weights below 1e-3 dropped), min-distance score."""
    _, w1, w2, _, _ = assignment(atten, s1, s2)
    weight, pred = fine_rows(atten, s1, s2, w1, w2, p2)
    Rm, t, _ = procrustes(pred, p1, weight, thresh=0.001)
    d = min_dist(p1, p2, Rm, t)
    score = ((d < dis_thres).to(F64) * w1).sum(1) / (w1.sum(1) + 1e-8) * w1.mean(1)
    return Rm, t, score


# --------------------------------------------------------------------------------------------------------- test problems
def random_pose(B, gen):
    """Uniformly random proper rotations (B,3,3) and translations of ~0.1 (B,3), float32."""
    Q = torch.linalg.qr(torch.randn(B, 3, 3, generator=gen, dtype=F64))[0]
    Q = Q * torch.sign(torch.det(Q))[:, None, None]
    return Q.float(), 0.1 * torch.randn(B, 3, generator=gen)


def constructed_case(B, N1, N2, gen, n_bg, hi=8.0, noise=1.5):
    """The non-square relative of helpers.constructed_similarity.  With nm = min(N1 - n_bg, N2), row 1+i (i < nm) has a peak of
    `hi`..`hi`+1 over +-`noise` at column 1+perm[i] and p1_i = Q p2_perm[i] + t + 3 mm of noise; the other rows (the last n_bg at
    least) and every unmatched column peak at the background token, get overlap scores of 0.05..0.15 instead of 0.8..0.99, and
    the rows get unrelated points.  All coordinates are O(1): |p2| <= 0.87, |p1| <= 1.3.
    Returns atten (B,N1+1,N2+1), score1 (B,N1), score2 (B,N2), p1, p2, R_gt = Q, t_gt (all float32)."""
    atten = noise * (torch.rand(B, N1 + 1, N2 + 1, generator=gen) * 2 - 1)
    s1 = 0.8 + 0.19 * torch.rand(B, N1, generator=gen)
    s2 = 0.8 + 0.19 * torch.rand(B, N2, generator=gen)
    p2 = torch.rand(B, N2, 3, generator=gen) - 0.5
    p1 = torch.rand(B, N1, 3, generator=gen) - 0.5
    Q, tg = random_pose(B, gen)
    nm = min(N1 - n_bg, N2)
    for b in range(B):
        perm = torch.randperm(N2, generator=gen)
        rows, cols = torch.arange(nm), perm[:nm]
        atten[b, 1 + rows, 1 + cols] = hi + torch.rand(nm, generator=gen)
        p1[b, :nm] = p2[b, cols] @ Q[b].T + tg[b] + 0.003 * torch.randn(nm, 3, generator=gen)
        atten[b, 1 + nm:, 0] = hi + torch.rand(N1 - nm, generator=gen)
        s1[b, nm:] = 0.05 + 0.1 * torch.rand(N1 - nm, generator=gen)
        free = perm[nm:]
        atten[b, 0, 1 + free] = hi + torch.rand(N2 - nm, generator=gen)
        s2[b, free] = 0.05 + 0.1 * torch.rand(N2 - nm, generator=gen)
    return dict(atten=atten, score1=s1, score2=s2, p1=p1, p2=p2, R_gt=Q, t_gt=tg)


def all_background_(case, b, gen, hi=8.0, noise=1.5):
    """Make element b of a case all background, in place: every row and every column peaks at token 0."""
    R, C = case["atten"].shape[1:]
    x = noise * (torch.rand(R, C, generator=gen) * 2 - 1)
    x[:, 0] += hi
    x[0, :] += hi
    case["atten"][b] = x
    case["score1"][b] = 0.05 + 0.1 * torch.rand(R - 1, generator=gen)
    case["score2"][b] = 0.05 + 0.1 * torch.rand(C - 1, generator=gen)


# name -> (B, N1, N2, n_bg, nprop); nprop is never a multiple of the hypothesis kernel's 256 threads
CASES = {
    "1x1": (1, 1, 1, 0, 300),        # R = C = 2, the minimum the ABI accepts; idle row groups in the column kernels
    "5x7": (2, 5, 7, 1, 300),        # L = 35 < 512 threads of the CDF kernel; fewer rows than one wave's four
    "37x53": (2, 37, 53, 9, 1500),   # nothing divides; C - 1 < 64
    "130x70": (3, 130, 70, 20, 1500),  # the 16-row block tail, the 64-column tail, N1 > N2
    "196x196": (2, 196, 196, 40, 6000),  # the production coarse shape
    "257x64": (1, 257, 64, 30, 1500),  # exactly one full column block plus the background; a row tail of one
}
# the same generator with special inputs
SPECIAL = {
    "allbg": (3, 37, 53, 9, 700),   # element 1 is all background: w = 0, an all-zero CDF, 0 / (0 + 1e-8)
    "spiked": (3, 37, 53, 9, 700),  # a row and a column at +-30: online rescaling of the column sums, underflowing products
}
SPIKE = 30.0


def make_case(name):
    """The inputs of a named case, from a seed that depends on the name alone; rand (B,3*nprop) is the uniform draw."""
    B, N1, N2, n_bg, nprop = CASES.get(name) or SPECIAL[name]
    gen = torch.Generator().manual_seed(1000 * N1 + N2 + 7 * len(name))
    own = 1 if name == "spiked" else 0  # spiked: its last element comes from a generator of its own, after the others
    case = constructed_case(B - own, N1, N2, gen, n_bg)
    if name == "allbg":
        all_background_(case, 1, gen)
    # element 0: row up, column down; element 1: row down, column up: all of the CDF lies in that one row / column, so no
    # hypothesis is well conditioned.  Element 2: row down, column down: the rest of it is untouched and keeps its hypotheses
    if name == "spiked":
        case["atten"][0, 5, :] += SPIKE
        case["atten"][0, :, 11] -= SPIKE
        case["atten"][1, 30, :] -= SPIKE
        case["atten"][1, :, 50] += SPIKE
    case["rand"] = torch.rand(B - own, 3 * nprop, generator=gen)
    if own:
        gen = torch.Generator().manual_seed(53)
        last = constructed_case(1, N1, N2, gen, n_bg)
        last["atten"][0, 7, :] -= SPIKE
        last["atten"][0, :, 20] -= SPIKE
        last["rand"] = torch.rand(1, 3 * nprop, generator=gen)
        case = {k: torch.cat((case[k], last[k])) for k in case}
    case.update(name=name, B=B, N1=N1, N2=N2, nprop=nprop)
    return case
