"""GPU parity of the fused geometry kernels (LRF, QueryAndLRFGroup, Procrustes) against the
golden fixtures captured from the reference and against the CPU oracle at full size."""
import os

import numpy as np
import pytest
import torch

from helpers import object_cloud

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    return {k: torch.from_numpy(z[k]) if z[k].ndim else z[k].item() for k in z.files}


def norm_clouds(n, B, seed, repl_every=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.stack([object_cloud(g, n, with_replacement=(i % repl_every == repl_every - 1)) for i in range(B)])
    c = x.mean(1, keepdim=True)
    return (x / (x - c).norm(dim=2).max(1)[0].reshape(-1, 1, 1)).contiguous()


def test_lrf_global_golden_and_oracle():
    from unopose_amd import ops
    from oracle import unopose_ref as R

    z = load("lrf_global")
    out = ops.lrf_global(z["pts"].cuda()).cpu()
    assert (out - z["out"]).abs().max() < 1e-4  # fp32; tolerance stated by north_star: 1e-4
    g = torch.Generator().manual_seed(7)
    pts = torch.stack([object_cloud(g, 5000) for _ in range(4)])
    assert (ops.lrf_global(pts.cuda()).cpu() - R.get_batch_lrf(pts)).abs().max() < 1e-4
    pts = torch.stack([object_cloud(g, 2048, True) for _ in range(4)])
    assert (ops.lrf_global(pts.cuda()).cpu() - R.get_batch_lrf(pts)).abs().max() < 1e-4


def _well_conditioned(ref, radius):
    """Points whose reference frame is well defined: the smallest eigenvalue of
    the neighbourhood covariance is separated, the sign vote is not near a tie, and the x-axis
    accumulator is not ~0.  Computed in float64 from the reference output's own channels 0-2."""
    rel = ref[:, :3].double().permute(0, 2, 1, 3)  # (B,N,3,S) = p_k - c
    S = rel.shape[-1]
    cov = rel @ rel.transpose(-1, -2) / S
    lam, vec = torch.linalg.eigh(cov)  # ascending
    gap = (lam[..., 1] - lam[..., 0]) / lam[..., 2].clamp(min=1e-30)
    z = vec[..., 0]
    proj = -(z.unsqueeze(-2) @ rel).squeeze(-2)  # z . (c - p_k)
    vote = (proj > 1e-3).sum(-1) - (proj < -1e-3).sum(-1)
    near = ((proj.abs() - 1e-3).abs() < 2e-5).sum(-1)  # neighbours sitting on the vote threshold
    zp = torch.where((vote < 0).unsqueeze(-1), -z, z)
    nrm = (zp.unsqueeze(-2) @ rel).squeeze(-2)
    vi = rel - zp.unsqueeze(-1) * nrm.unsqueeze(-2)
    ab = (radius - rel.norm(dim=-2)) ** 2 * nrm ** 2
    acc = (ab.unsqueeze(-2) * vi).sum(-1).norm(dim=-1)
    scale = (ab.unsqueeze(-2) * vi).norm(dim=-2).sum(-1).clamp(min=1e-30)
    return (gap > 2e-2) & ((vote.abs() - near) >= 1) & (acc / scale > 1e-2)


def _frame_invariants(out, ref, radius):
    """What must hold for EVERY point whose frame exists, however ill-conditioned its neighbourhood: channels
    3-5 are F^T (p_k - c) / r for ONE orthonormal frame F = [x, y, z] per point with y = x x z (P:470-471) -- a LEFT-handed frame,
    det F = -1 -- so (i) every neighbour keeps its length, (ii) an orthogonal map of determinant -1 takes the relative coordinates onto
    them, (iii) the z-axis is orthogonal to the dominant direction of the neighbourhood whenever that direction is defined (z = +-v_min;
    any unit vector of span(v_0, v_1) if the two smallest eigenvalues tie).  The frame does NOT exist where the x-axis accumulator
    vanishes (rank-deficient neighbourhoods: duplicated / collinear / coplanar points): the reference then emits x = y = 0, and such points
    are compared with the reference output directly.  float64 throughout.
    Returns (frame-exists mask, worst length error, worst residual of the fitted det -1 map, worst |z . v_max|) over the points with a frame."""
    rel = ref[:, :3].double().permute(0, 2, 1, 3)            # (B,N,3,S)
    o = out[:, 3:].double().permute(0, 2, 1, 3) * radius       # (B,N,3,S) = F^T (p_k - c)

    def fit(o):
        U, _, Vh = torch.linalg.svd(o @ rel.transpose(-1, -2))  # sum_k o_k rel_k^T
        d = torch.det(U @ Vh)
        Ft = U @ torch.diag_embed(torch.stack([torch.ones_like(d), torch.ones_like(d), -d], -1)) @ Vh  # the closest det -1 orthogonal map
        return Ft, (o - Ft @ rel).abs().amax(dim=(2, 3))

    # the frame exists where the REFERENCE output is an orthogonal image of the relative coordinates
    exists = fit(ref[:, 3:].double().permute(0, 2, 1, 3) * radius)[1] < 5e-5  # (fp32 outputs: an existing frame fits to ~1e-5, a missing one misses by O(0.1))
    Ft, resid = fit(o)
    len_err = (o.norm(dim=2) - rel.norm(dim=2)).abs().amax(-1)
    lam, vec = torch.linalg.eigh(rel @ rel.transpose(-1, -2) / rel.shape[-1])
    constrained = exists & ((lam[..., 2] - lam[..., 1]) / lam[..., 2].clamp(min=1e-30) > 2e-2)
    zdot = (Ft[..., 2, :] * vec[..., 2]).sum(-1).abs()
    return exists, len_err[exists].max().item(), resid[exists].max().item(), zdot[constrained].max().item()


def _check_group(out, ref, radius, expect_well, tol=2e-3):
    """`expect_well`: the well-conditioned fraction per cloud, a property of the REFERENCE output measured once
    (clouds sampled with replacement are full of duplicated neighbourhoods and score low); asserted as measured
    minus 0.01, so the set on which every point is compared cannot silently shrink."""
    # channels 0-2 are plain differences of the same fp32 numbers: bit-exact
    assert torch.equal(out[:, :3], ref[:, :3])
    # channels 3-5 depend on a 3x3 eigenvector (torch.svd vs register Jacobi).  Where the frame is
    # well conditioned EVERY point must agree within tol; ill-conditioned frames (degenerate or
    # duplicated neighbourhoods, tied sign votes) are implementation-defined in the reference itself.
    err = (out[:, 3:] - ref[:, 3:]).abs().amax(dim=(1, 3))  # (B,N)
    well = _well_conditioned(ref, radius)
    frac = well.float().mean(1)
    print("well-conditioned fraction per cloud:", [round(f, 4) for f in frac.tolist()],
          "worst error on them: %.2e" % err[well].max().item(), "; all points within tol: %.4f" % (err < tol).float().mean().item())
    assert all(f >= e - 0.01 for f, e in zip(frac.tolist(), expect_well)), (frac.tolist(), expect_well)
    bad = (err >= tol) & well
    assert not bad.any(), f"{int(bad.sum())} well-conditioned points differ, worst {err[well].max().item():.3e}"
    # ALL points, ill-conditioned ones included: the output is a proper rotation of the relative coordinates whose z-axis avoids the
    # neighbourhood's dominant direction -- for the kernel AND (as a sanity check of the invariants) for the reference output
    for name, x in (("kernel", out), ("reference", ref)):
        exists, len_err, resid, zdot = _frame_invariants(x, ref, radius)
        print(f"{name}: frame exists on {exists.double().mean().item():.3f} of ALL points; there |len| {len_err:.1e}, det -1 residual {resid:.1e}, "
              f"|z.v_max| {zdot:.1e}")
        assert len_err < 2e-4 and resid < 2e-4 and zdot < 2e-2, (name, len_err, resid, zdot)
    # Everywhere else the reference's own x-axis is  acc / (|acc| + 1e-10)  with |acc| <~ 1e-9 (P:466: smooth patches at a small radius,
    # duplicated / coplanar neighbours), i.e. SHORTER than a unit vector or pure rounding noise: x and y shrink (to 0 in the limit), z stays
    # a unit vector.  What still holds for every point of both outputs: no neighbour gets longer than it is.
    rel_len = ref[:, :3].double().norm(dim=1) / radius
    for name, x in (("kernel", out), ("reference", ref)):
        grow = (x[:, 3:].double().norm(dim=1) - rel_len).max().item()
        assert grow < 1e-4, (name, grow)
    noframe = ~exists
    if noframe.any():
        dz = (out[:, 5] - ref[:, 5]).abs().amax(-1)[noframe]
        print("points whose reference frame is not orthonormal (shrunk or missing x-axis): %d; worst z-channel deviation there %.2e"
              % (int(noframe.sum()), dz.max().item()))
    if (~well).any():
        print("worst deviation on the ill-conditioned points (frame implementation-defined): %.2e" % err[~well].max().item())
    return frac


@pytest.mark.parametrize("name,expect", [("query_lrf_group_r0.2_ns32", (0.9258, 0.0977)),
                                         ("query_lrf_group_r0.4_ns64", (0.9922, 0.7852))])
def test_query_lrf_group_golden(name, expect):
    from unopose_amd import ops

    z = load(name)
    out = ops.query_lrf_group(z["xyz"].cuda(), z["radius"], z["nsample"]).cpu()
    _check_group(out, z["out"], z["radius"], expect)


# N = 777: not a multiple of 64, a list shorter than a wave, and centres that fill the list early (12 %: 40 or more points inside the
# radius) beside padded ones (the smallest neighbourhood holds 3 points): the tail guards of the ball query's multi-step scan
@pytest.mark.parametrize("N,r,ns,expect", [(2048, 0.1, 64, (0.9321, 0.9712, 0.4658)), (2048, 0.2, 256, (0.9858, 0.9951, 0.9697)),
                                           (777, 0.2, 40, (0.9820, 0.9846, 0.8378))],
                         ids=["0.1-64-expect0", "0.2-256-expect1", "N777-0.2-40"])  # (the 2048-point cases keep the ids they had)
def test_query_lrf_group_full_size_vs_oracle(oracle_ext, N, r, ns, expect):
    from unopose_amd import ops
    from oracle import unopose_ref as R

    x = norm_clouds(N, 3, seed=11)
    out = ops.query_lrf_group(x.cuda(), r, ns).cpu()
    ref = R.query_and_lrf_group(x, r, ns, oracle_ext)
    _check_group(out, ref, r, expect)


def test_weighted_procrustes_golden():
    from unopose_amd import ops

    z = load("weighted_procrustes")
    R, t = ops.weighted_procrustes(z["src"].cuda(), z["ref"].cuda(), z["w"].cuda(), 0.001)
    assert (R.cpu() - z["R"]).abs().max() < 1e-4 and (t.cpu() - z["t"]).abs().max() < 1e-4
    R, t = ops.weighted_procrustes(z["src3"].cuda(), z["ref3"].cuda(), None, 0.5)
    assert (R.cpu() - z["R3"]).abs().max() < 1e-4 and (t.cpu() - z["t3"]).abs().max() < 1e-4


def test_weighted_procrustes_stress_256_hypotheses():
    """BASELINE config 5: P pairs x 256 hypotheses x N in {3,196,2048}, 30 % zero weights."""
    from unopose_amd import ops
    from oracle import unopose_ref as Rf

    g = torch.Generator().manual_seed(3)
    for N in (3, 196, 2048):
        M = 4 * 256
        src = torch.randn(M, N, 3, generator=g)
        Q = torch.linalg.qr(torch.randn(M, 3, 3, generator=g))[0]
        Q = Q * torch.sign(torch.det(Q)).reshape(-1, 1, 1)
        t = torch.randn(M, 1, 3, generator=g)
        ref = src @ Q.transpose(1, 2) + t + 1e-3 * torch.randn(M, N, 3, generator=g)
        w = torch.rand(M, N, generator=g)
        if N > 3:
            w[torch.rand(M, N, generator=g) < 0.3] = 0
        R, tt = ops.weighted_procrustes(src.cuda(), ref.cuda(), w.cuda(), 0.0)
        Rr, tr = Rf.weighted_procrustes(src, ref, w, 0.0)
        assert (R.cpu() - Rr).abs().max() < 1e-4, N
        # t = c_ref - R c_src amplifies R's error by |c_src| (~2 here); near-collinear 3-point sets are
        # ill-conditioned, so N == 3 gets 3e-4 on t
        assert (tt.cpu() - tr).abs().max() < (3e-4 if N == 3 else 1e-4), N
        # property: proper rotations
        assert (torch.det(R) - 1).abs().max() < 1e-4
        assert (R @ R.transpose(1, 2) - torch.eye(3, device="cuda")).abs().max() < 1e-4


def test_procrustes_degenerate_inputs_are_rotations():
    from unopose_amd import ops

    src = torch.zeros(3, 3, 3)
    ref = torch.zeros(3, 3, 3)
    src[1] = torch.tensor([[0., 0, 0], [1, 0, 0], [1, 0, 0]])  # rank 1 (duplicate correspondence)
    ref[1] = torch.tensor([[1., 1, 1], [1, 2, 1], [1, 2, 1]])
    src[2] = torch.tensor([[0., 0, 0], [1, 0, 0], [0, 1, 0]])  # rank 2
    ref[2] = torch.tensor([[0., 0, 0], [0, 1, 0], [-1, 0, 0]])
    R, t = ops.weighted_procrustes(src.cuda(), ref.cuda(), None, 0.5)
    R = R.cpu()
    assert torch.allclose(R[0], torch.eye(3))  # H = 0 -> identity (LAPACK returns U = V = I)
    assert (torch.det(R) - 1).abs().max() < 1e-5
    assert torch.allclose(R[2], torch.tensor([[0., -1, 0], [1, 0, 0], [0, 0, 1]]), atol=1e-5)
    # rank 1: the correspondences themselves are still mapped exactly
    assert torch.allclose(src[1] @ R[1].T + t.cpu()[1], ref[1], atol=1e-5)


# ---------------------------------------------------------------- the other QueryAndGroup / QueryAndLRFGroup options ------
def _oracle_lrf_group(oracle_ext, x, new, r, ns, idx=None):
    """P:548-565 step by step on the CPU oracle: (idx, grouped - new (B,3,N,S), lrf (B,3,N,S), grouped - xyz)."""
    from oracle import unopose_ref as R

    if idx is None:
        idx = oracle_ext.ball_query(new.contiguous(), x.contiguous(), r, ns)
    grouped = oracle_ext.group_points(x.transpose(1, 2).contiguous(), idx)
    lrf = R.lrf_batch(x, grouped.transpose(1, 2), r).transpose(1, 2)
    return idx, grouped - new.transpose(1, 2).unsqueeze(-1), lrf, grouped - x.transpose(1, 2).unsqueeze(-1)


def test_query_and_lrf_group_centres_off_the_points_and_all_options(oracle_ext):
    """new_xyz != xyz, normalize_xyz, ret_grouped_xyz, use_feature (P:484-584): the neighbour lists are the balls around
    new_xyz, channels 0-2 are relative to new_xyz (divided by the radius), the frame stays centred on xyz (P:555)."""
    from unopose_amd.pointnet2 import pointnet2_utils as P

    r, ns = 0.2, 32
    x = norm_clouds(1024, 2, seed=5, repl_every=9)
    g = torch.Generator().manual_seed(6)
    new = (x + 0.03 * torch.randn(x.shape, generator=g)).contiguous()
    feats = torch.randn(2, 5, 1024, generator=g)
    idx, rel_new, lrf, rel_x = _oracle_lrf_group(oracle_ext, x, new, r, ns)

    m = P.QueryAndLRFGroup(r, ns, use_xyz=True, use_feature=True, normalize_xyz=True, ret_grouped_xyz=True)
    out, grouped = m(x.cuda(), new.cuda(), feats.cuda())
    out, grouped = out.cpu(), grouped.cpu()
    assert out.shape == (2, 5 + 6, 1024, ns) and grouped.shape == (2, 3, 1024, ns)
    assert torch.equal(out[:, :5], oracle_ext.group_points(feats, idx))
    # `tensor / python_float` on the device is a multiply by the reciprocal (1 ulp from the host's true division), in the reference too
    torch.testing.assert_close(grouped, rel_new / r, rtol=3e-7, atol=0)
    assert torch.equal(out[:, 5:8], grouped)
    err = (out[:, 8:] - lrf).abs().amax(dim=(1, 3))
    well = _well_conditioned(torch.cat([rel_x, lrf], 1), r)
    assert well.float().mean() > 0.85, well.float().mean()
    assert err[well].max() < 2e-3, err[well].max()
    # not normalised, lrf only (use_xyz=False needs features, P:561-566) and the features=None form
    only = P.QueryAndLRFGroup(r, ns, use_xyz=False)(x.cuda(), new.cuda(), feats.cuda()).cpu()
    assert torch.equal(only, out[:, 8:])
    both = P.QueryAndLRFGroup(r, ns, use_xyz=True)(x.cuda(), new.cuda(), feats.cuda()).cpu()
    assert torch.equal(both[:, :3], rel_new) and torch.equal(both[:, 3:], only)
    assert torch.equal(P.QueryAndLRFGroup(r, ns, use_xyz=True)(x.cuda(), new.cuda()).cpu(), only)
    # centres == points through the general route is the fused kernel's answer, bit for bit
    xc = x.cuda()
    fused = P.QueryAndLRFGroup(r, ns, use_xyz=True)(xc, xc, feats.cuda())
    general = P.QueryAndLRFGroup(r, ns, use_xyz=True)(xc, xc.clone(), feats.cuda())
    assert torch.equal(fused, general)
    with pytest.raises(ValueError, match="npoint == N"):
        P.QueryAndLRFGroup(r, ns, use_xyz=True)(xc, xc[:, :512].contiguous(), feats.cuda())


@pytest.mark.parametrize("cls", ["QueryAndGroup", "QueryAndLRFGroup"])
def test_sample_uniformly_redraws_every_neighbour_list_from_its_distinct_members(oracle_ext, cls):
    """sample_uniformly / ret_unique_cnt (P:343-351, 536-544): every list becomes its distinct indices (ascending) followed by
    uniform draws from them, unique_cnt counts them; everything downstream is computed from the re-drawn lists."""
    from unopose_amd.pointnet2 import pointnet2_utils as P

    r, ns = 0.15, 32
    x = norm_clouds(512, 2, seed=8, repl_every=9)
    xc = x.cuda()
    torch.manual_seed(0)
    m = getattr(P, cls)(r, ns, use_xyz=True, ret_grouped_xyz=True, sample_uniformly=True, ret_unique_cnt=True)
    out, grouped, cnt = m(xc, xc, None if cls == "QueryAndGroup" else torch.zeros(2, 1, 512, device="cuda"))
    assert cnt.shape == (2, 512) and cnt.dtype == torch.float32 and cnt.device.type == "cpu"
    base = oracle_ext.ball_query(x, x, r, ns)
    # recover the re-drawn lists from the grouped coordinates (the clouds hold no duplicate points) and check them row by row
    got = grouped.cpu().permute(0, 2, 3, 1) + x.unsqueeze(2)  # (B,N,S,3) absolute coordinates
    redrawn = torch.cdist(got.reshape(2, -1, 3), x).argmin(-1).reshape(2, 512, ns)
    back = x.gather(1, redrawn.reshape(2, -1, 1).expand(-1, -1, 3)).reshape(2, 512, ns, 3)
    assert (back - got).abs().max() < 1e-5  # (p - c) + c is p up to rounding
    multi = 0
    for b in range(2):
        for j in range(512):
            u = torch.unique(base[b, j].long())
            n = len(u)
            assert cnt[b, j] == n
            assert torch.equal(redrawn[b, j, :n], u)
            assert torch.isin(redrawn[b, j, n:], u).all()
            multi += int(len(torch.unique(redrawn[b, j, n:])) > 1)
    assert multi > 100  # the tails are draws, not one repeated index
    if cls == "QueryAndLRFGroup":
        _, rel_new, lrf, rel_x = _oracle_lrf_group(oracle_ext, x, x, r, ns, idx=redrawn.int())
        out = out.cpu()
        assert torch.equal(out[:, :3], rel_new)
        well = _well_conditioned(torch.cat([rel_x, lrf], 1), r)
        err = (out[:, 3:] - lrf).abs().amax(dim=(1, 3))
        assert well.float().mean() > 0.5 and err[well].max() < 2e-3, (well.float().mean(), err[well].max())
    else:
        assert torch.equal(out, grouped)
