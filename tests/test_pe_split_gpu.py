"""GPU: the bf16x3 positional encoding as a geometry launch (lists, counts, frames of one or two scales) + MLP launches
(csrc/pe.hip pe_geometry_kernel / pe_group_mlp_max_bf16x3_kernel).  Every assertion is an equality, or a bound of tests/test_geom_gpu.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

R2, S2, R1, S1 = 0.2, 256, 0.1, 64  # the model's two scales


@pytest.fixture(scope="module")
def pe():
    from unopose_amd.model import UNOPose, default_model_cfg
    from unopose_amd.synthetic import trained_like_

    return trained_like_(UNOPose(default_model_cfg())).cuda().eval().fine_point_matching.PE


def bits(t):
    """Bitwise view (NaN frames of degenerate neighbourhoods compare equal to themselves)."""
    return t.contiguous().view(torch.int32) if t.is_floating_point() else t


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def ids(lists):
    return lists.to(torch.int32) & 0xFFFF


def full(counts, S):
    """A count as its consumers read it: -1 (more than S points inside the radius) and S both mean a full list of S distinct hits --
    the MLP runs all S / 32 tiles, a narrower pass tests all S candidates or scans, with equal results.  The index-order scan of a
    cloud the grid does not take stops at a full list and reports -1 where exactly S points were inside; a pass over a wider
    scale's list counts them all and reports S."""
    return torch.where((counts < 0) | (counts >= S), torch.full_like(counts, S), counts)


def clouds(N, B, seed):
    from test_geom_gpu import norm_clouds

    return norm_clouds(N, B, seed=seed).cuda()


def check_two_scale(pe, x, r2=R2, s2=S2, r1=R1, s1=S1):
    """One two-scale geometry launch + the MLP launches == the per-scale calls, on every centre; returns the two-scale geometry."""
    from unopose_amd import ops

    g2, g1, cand = ops.pe_geometry(x, r2, s2, r1, s1, want_cand=True)
    for g, r, s, mlp in ((g2, r2, s2, pe.mlp2), (g1, r1, s1, pe.mlp1)):
        one = ops.pe_geometry(x, r, s)[0]
        for a, b, what in zip(g, one, ("lists", "counts", "frames")):
            if what == "counts":
                a, b = full(a, s), full(b, s)
            assert same(a, b), (what, r, s, int((bits(a) != bits(b)).sum()))
        feat, (l, c) = ops.pe_group_mlp_max(x, r, s, mlp, bf16x3=True, want_cand=True)
        assert same(ops.pe_mlp_max(x, r, s, mlp, g), feat), (r, s)
        assert torch.equal(l, ids(g[0])) and torch.equal(full(c, s), full(g[1], s))
    assert torch.equal(cand[0], ids(g2[0])) and torch.equal(cand[1], g2[1])
    # the narrow scale fed with the wide scale's int32 lists (the hand-off of ops.pe_group_mlp_max) is the same again
    assert same(ops.pe_group_mlp_max(x, r1, s1, pe.mlp1, bf16x3=True, cand_in=cand), ops.pe_mlp_max(x, r1, s1, pe.mlp1, g1))
    return g2, g1


def check_lists(x, g, r, s):
    from unopose_amd.pointnet2 import _ext

    ref = _ext.ball_query(x, x, r, s)
    assert torch.equal(ids(g[0]), ref), (r, s, int((ids(g[0]) != ref).sum()))


@torch.no_grad()
def test_two_scale_launch_equals_per_scale_calls_and_module_paths(pe):
    x = clouds(2048, 3, 5)
    x[1, 1000:1400] = x[1, :400]  # duplicated points
    g2, g1 = check_two_scale(pe, x)
    check_lists(x, g2, R2, S2)
    check_lists(x, g1, R1, S1)
    from unopose_amd import ops

    with torch.autocast("cuda", dtype=torch.bfloat16):
        both = pe.groups(x)
        buf = torch.zeros(4, 2048, 512, dtype=torch.bfloat16, device="cuda")
        pe.groups_split(x, buf, 1)
        ref = torch.zeros_like(buf)
        ops.pe_group_mlp_max(x, pe.r2, pe.ns2, pe.mlp2, bf16x3=True, out_split=(ref, 1, 128))
        ops.pe_group_mlp_max(x, pe.r1, pe.ns1, pe.mlp1, bf16x3=True, out_split=(ref, 1, 0))
    f1 = ops.pe_group_mlp_max(x, pe.r1, pe.ns1, pe.mlp1, bf16x3=True)
    f2 = ops.pe_group_mlp_max(x, pe.r2, pe.ns2, pe.mlp2, bf16x3=True)
    assert same(both, torch.cat([f1, f2], 2))
    assert torch.equal(buf.view(torch.int16), ref.view(torch.int16))


@torch.no_grad()
@pytest.mark.parametrize("N", [2048, 2043])
def test_rows_do_not_depend_on_batch_position_or_batch_fill(pe, N):
    """The same cloud alone (one centre per wave: every eigen-solve batch holds one centre) and as cloud 31 of 32 (sixteen centres per
    wave: full batches; N = 2043 leaves the last wave of a cloud a partial one) and at every centres-per-wave setting in between."""
    from unopose_amd import ops

    x = clouds(N, 32, 9)
    full = ops.pe_geometry(x, R2, S2, R1, S1)[:2]
    feats = [ops.pe_mlp_max(x, r, s, m, g) for g, r, s, m in ((full[0], R2, S2, pe.mlp2), (full[1], R1, S1, pe.mlp1))]
    for B in (1, 4, 8, 16):
        part = ops.pe_geometry(x[32 - B:].contiguous(), R2, S2, R1, S1)[:2]
        for gf, gp in zip(full, part):
            for a, b, what in zip(gf, gp, ("lists", "counts", "frames")):
                assert same(a[31], b[B - 1]), (B, what)
        if B == 1:
            for f, g, r, s, m in ((feats[0], part[0], R2, S2, pe.mlp2), (feats[1], part[1], R1, S1, pe.mlp1)):
                assert same(ops.pe_mlp_max(x[31:].contiguous(), r, s, m, g)[0], f[31])


@torch.no_grad()
@pytest.mark.parametrize("N", [255, 256, 1000, 4096, 4100])
def test_point_counts_around_the_grid_limits(pe, N):
    """N not a multiple of 64, the smallest / largest clouds the grid takes and their neighbours that are scanned instead."""
    x = clouds(N, 2, 30 + N % 7)
    g2, g1 = check_two_scale(pe, x)
    check_lists(x, g2, R2, S2)
    check_lists(x, g1, R1, S1)


@torch.no_grad()
def test_identical_points(pe):
    x = torch.full((2, 2048, 3), 0.125, device="cuda")
    g2, g1 = check_two_scale(pe, x)
    check_lists(x, g2, R2, S2)
    check_lists(x, g1, R1, S1)
    assert bool((g2[1] == -1).all()) and bool((g1[1] == -1).all())  # 2048 points inside every radius


@torch.no_grad()
def test_nan_centre_runs_one_tile_of_point_zero(pe):
    from unopose_amd import ops

    x = clouds(2048, 2, 13)
    x[0, 5] = float("nan")
    x[1, 2047] = float("nan")
    g2, g1 = check_two_scale(pe, x)
    check_lists(x, g2, R2, S2)
    check_lists(x, g1, R1, S1)
    for g in (g2, g1):
        for b, j in ((0, 5), (1, 2047)):
            assert int(g[1][b, j]) == 0 and bool((ids(g[0])[b, j] == 0).all())
    # the row of such a centre: one tile of the all-point-0 list == the same list handed in as candidates
    f = ops.pe_mlp_max(x, R1, S1, pe.mlp1, g1)
    assert same(f, ops.pe_group_mlp_max(x, R1, S1, pe.mlp1, bf16x3=True))


@torch.no_grad()
def test_overflowed_wide_list_falls_back_per_centre(pe):
    """32-entry lists at radius 0.5 overflow for nearly every centre (count -1): the narrow scale of those centres is found by the
    grid / scan, of the others from the wide list; both equal the narrow scale's own launch."""
    from unopose_amd import ops

    x = clouds(2048, 3, 5)
    gw, gn, _ = ops.pe_geometry(x, 0.5, 32, R1, S1)
    assert (gw[1] == -1).float().mean() > 0.9
    check_lists(x, gw, 0.5, 32)
    one = ops.pe_geometry(x, R1, S1)[0]
    for a, b in zip(gn, one):
        assert same(a, b)  # (grid: both counts are exact)
    x4 = clouds(4100, 2, 6)  # no grid: the fall-back is the scan
    gw, gn, _ = ops.pe_geometry(x4, 0.5, 32, R1, S1)
    assert (gw[1] == -1).float().mean() > 0.9
    for i, (a, b) in enumerate(zip(gn, ops.pe_geometry(x4, R1, S1)[0])):
        assert same(a, b) if i != 1 else same(full(a, S1), full(b, S1))


@torch.no_grad()
@pytest.mark.parametrize("r,ns", [(R1, S1), (R2, S2)])
def test_frames_keep_the_invariants_of_the_grouping_kernel(oracle_ext, r, ns):
    """The frames the geometry kernel writes, applied to the neighbours of its lists, against tests/test_geom_gpu.py's frame
    invariants, with its bounds; the relative coordinates are the reference grouping's, bit for bit."""
    from oracle import unopose_ref as R
    from test_geom_gpu import _frame_invariants, norm_clouds
    from unopose_amd import ops

    x = norm_clouds(2048, 3, seed=11)
    lists, _, frames = ops.pe_geometry(x.cuda(), r, ns)[0]
    idx = ids(lists).cpu().long()                                        # (B,N,S)
    F = frames.cpu().reshape(3, 2048, 3, 3)                              # rows x, y, z
    nb = torch.gather(x.unsqueeze(1).expand(3, 2048, 2048, 3), 2, idx.unsqueeze(-1).expand(-1, -1, -1, 3))
    rel = nb - x.unsqueeze(2)                                            # (B,N,S,3) = p_k - c
    loc = (torch.einsum("bnij,bnsj->bnsi", F.double(), rel.double()) / r).float()
    out = torch.cat([rel, loc], 3).permute(0, 3, 1, 2).contiguous()      # (B,6,N,S)
    ref = R.query_and_lrf_group(x, r, ns, oracle_ext)
    assert torch.equal(out[:, :3], ref[:, :3])
    exists, len_err, resid, zdot = _frame_invariants(out, ref, r)
    assert len_err < 2e-4 and resid < 2e-4 and zdot < 2e-2, (len_err, resid, zdot)
