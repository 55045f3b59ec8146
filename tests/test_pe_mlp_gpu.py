"""GPU: the two neighbourhood-MLP kernels of csrc/pe.hip (pe_group_mlp_max_bf16x3_kernel, pe_group_mlp_max_kernel) against the float64
reference and the propagated error bound of tests/pe_mlp_ref.py.  The bf16x3 kernel takes lists, counts and frames as inputs, so its
MLP stage is tested apart from the ill-conditioned frame computation, on inputs built to sit on every edge of its tile loop; the
teeth of these comparisons (what a dropped lo term, a tile loop that stops early or a wrong channel permutation would do to them) are
checked without a GPU in test_pe_mlp_ref_cpu.py.  The float64 references run in torch on the GPU, in chunks of centres."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pe_mlp_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def built(B, N, S):
    """A case of `make_case` with its stand-in module, reference and bound (shared between tests, never changed)."""
    c = P.make_case(B, N, S, seed=B + N + S, device="cuda")
    c.mlp = P.FoldedMLP(c.folded).cuda()
    c.ref, c.bound = P.pe_mlp_ref(c.pts, c.radius, c.lists, c.frames, c.folded)
    assert bool((c.ref[:, :, c.dead] == 0).all())
    return c


def geom(c):
    return (c.lists, c.counts, c.frames)


def worst(out, ref, bound, rows=None):
    """max err / bound (over the centres `rows`); a non-finite output counts as infinite."""
    r = (out.double() - ref).abs() / bound.clamp_min(1e-300)
    r = torch.where(torch.isfinite(out), r, torch.full_like(r, float("inf")))
    return float((r if rows is None else r[rows]).max())


# ------------------------------------------------------------------------------------------------------------ a. bf16x3 MLP in isolation
SHAPES = [
    (2, 1, 32),       # one centre
    (2, 5, 64),       # five-point cloud
    (3, 70, 96),      # N not divisible by 4; S / 2 = 48 < 64
    (3, 700, 64),     # cpw = 2
    (4, 2100, 256),   # cpw = 4; both prefetch words full
    (2, 300, 320),    # lists longer than 256: the loop that is not fetched ahead
    (17, 2043, 32),   # cpw = 8; the last wave of a cloud is partial
    (33, 2043, 32),   # cpw = 16; 67 419 centres
]


@torch.no_grad()
@pytest.mark.parametrize("B,N,S", SHAPES)
def test_bf16x3_mlp_on_constructed_lists(B, N, S):
    """ops.pe_mlp_max on the lists / counts / frames of `make_case` (counts on every tile boundary, the far point in the last valid
    slot, a decade of dynamic range in the weights, dead channels): |out - ref| <= bound element-wise, dead channels exactly 0.
    The shapes are the smallest that reach each branch of unopose_pe_mlp_max_packed's centres-per-wave rule and of the list fetch.

    Worst err / bound measured on the MI355X (the CPU emulation of the arithmetic sits near 0.02-0.04):
    (2,1,32) 0.008   (2,5,64) 0.020   (3,70,96) 0.032   (3,700,64) 0.023   (4,2100,256) 0.056   (2,300,320) 0.020
    (17,2043,32) 0.025   (33,2043,32) 0.025"""
    from unopose_amd import ops

    c = built(B, N, S)
    out = ops.pe_mlp_max(c.pts, c.radius, S, c.mlp, geom(c))
    w = worst(out, c.ref, c.bound)
    print(f"bf16x3 ({B}, {N}, {S}): worst err / bound = {w:.4f}")
    assert out.shape == (B, N, 128) and out.dtype == torch.float32
    assert bool(torch.isfinite(out).all())
    assert bool((out[:, :, c.dead] == 0).all())
    assert bool(((out.double() - c.ref).abs() <= c.bound).all()), w


# ------------------------------------------------------------------------------------------------------------ b. output forms
SENTINEL = 0x5AA5


@torch.no_grad()
def test_padded_rows_through_the_c_abi():
    """out_ld = 160, out_split = 0 into a sentinel-filled buffer: columns 0-127 are the dense call's bits, 128-159 are untouched."""
    from unopose_amd import ops
    from unopose_amd._lib import call, ptr, stream_ptr
    from unopose_amd.ops.geometry import _pe_image

    c = built(3, 700, 64)
    B, N, S = 3, 700, 64
    dense = ops.pe_mlp_max(c.pts, c.radius, S, c.mlp, geom(c))
    buf = torch.full((B, N, 160), SENTINEL * 65537, dtype=torch.int32, device="cuda")
    image = _pe_image(c.mlp, c.pts.device)[2]
    call("unopose_pe_mlp_max_packed", ptr(c.pts), B, N, float(c.radius), S, ptr(image), ptr(c.lists), ptr(c.counts), ptr(c.frames),
         ptr(buf), 160, 0, stream_ptr())
    assert torch.equal(buf[:, :, :128], dense.view(torch.int32))
    assert bool((buf[:, :, 128:] == SENTINEL * 65537).all())


@torch.no_grad()
@pytest.mark.parametrize("c0", [0, 128])
def test_split_layout_output_at_a_cloud_and_column_offset(c0):
    """out_split = (buf, 1, c0) with buf (5,N,512) bf16 filled with a sentinel bit pattern: the 128 channels land in the blocks
    [hi (32 x bf16) | lo (32 x bf16)] of clouds 1..3 at channel c0, hi == bf16(out), |hi + lo - out| <= 2^-16 |out|; every other
    element of the buffer keeps the sentinel."""
    from unopose_amd import ops

    c = built(3, 700, 64)
    B, N, S = 3, 700, 64
    dense = ops.pe_mlp_max(c.pts, c.radius, S, c.mlp, geom(c))
    buf = torch.full((5, N, 512), SENTINEL, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    assert ops.pe_mlp_max(c.pts, c.radius, S, c.mlp, geom(c), out_split=(buf, 1, c0)) is buf
    blocks = buf.view(5, N, 8, 2, 32)                      # (cloud, centre, 32-channel block, hi | lo, channel)
    mine = blocks[1:4, :, c0 // 32:c0 // 32 + 4]
    hi, lo = mine[:, :, :, 0].reshape(B, N, 128), mine[:, :, :, 1].reshape(B, N, 128)
    assert torch.equal(hi.view(torch.int16), dense.bfloat16().view(torch.int16))
    assert bool(((hi.double() + lo.double() - dense.double()).abs() <= 2.0 ** -16 * dense.double().abs()).all())
    rest = torch.ones(5, N, 8, dtype=torch.bool, device="cuda")
    rest[1:4, :, c0 // 32:c0 // 32 + 4] = False
    assert bool((blocks.view(torch.int16)[rest] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------ c. fold and cache
@torch.no_grad()
def test_module_fold_and_in_place_edits_follow_the_reference():
    """A real _SharedMLP with non-trivial BatchNorm statistics (its fold is pinned to float64 in test_pe_mlp_ref_cpu.py) matches the
    reference of its folded weights within the bound; after each in-place edit the next call follows the reference of the NEW fold
    (the staleness rule of ops._pe_image), which the output of before the edit does not.  Worst err / bound measured on the MI355X:
    0.015 as built, 0.015 / 0.015 / 0.017 after the three edits."""
    from unopose_amd import ops
    from unopose_amd.model.modules import _SharedMLP

    c = built(3, 700, 64)
    torch.manual_seed(4)
    mlp = P.randomise_bn_(_SharedMLP([6, 32, 64, 128]), seed=2).cuda().eval()
    l0, l1, l2 = mlp.layers()

    def check(what, stale=None):
        folded = [l.folded() for l in mlp.layers()]
        for (w, b), (w64, b64) in zip(folded, P.fold64(mlp)):  # fp32 fold = float64 fold of the raw parameters to a few fp32 roundings
            assert bool(((w - w64).abs() <= 8 * 2.0 ** -24 * w64.abs()).all()), what
        ref, bound = P.pe_mlp_ref(c.pts, c.radius, c.lists, c.frames, folded)
        out = ops.pe_mlp_max(c.pts, c.radius, c.S, mlp, geom(c))
        w = worst(out, ref, bound)
        print(f"module, {what}: worst err / bound = {w:.4f}")
        assert bool(torch.isfinite(out).all()) and float(ref.max()) > 0.1
        assert bool(((out.double() - ref).abs() <= bound).all()), (what, w)
        if stale is not None:
            assert bool(((stale.double() - ref).abs() > bound).any()), what  # the edit matters: the old output is outside the new bound
        return out

    out = check("as built")
    l1.normlayer.bn.running_var.mul_(1.7)
    out = check("running_var * 1.7 on layer 1", out)
    l2.normlayer.bn.bias.add_(0.3)
    out = check("bias + 0.3 on layer 2", out)
    l0.conv.weight.mul_(-1)
    check("conv weight * -1 on layer 0", out)


# ------------------------------------------------------------------------------------------------------------ d. real geometry, both kernels
def real_clouds(B, N):
    from test_geom_gpu import norm_clouds

    x = norm_clouds(N, B, seed=B + N)
    if N >= 2048:
        x[1, 1000:1400] = x[1, :400]  # duplicated points
    return x.cuda()


@torch.no_grad()
@pytest.mark.parametrize("r,S", [(0.1, 64), (0.2, 256), (0.3, 32)])
@pytest.mark.parametrize("B,N", [(2, 300), (3, 2048)])
def test_fused_fp32_kernel_and_bf16x3_on_real_geometry(B, N, r, S):
    """The exact-fp32 fused kernel (ball query + frame + MLP in one launch) with u_l = (K_l + 2) * 2^-24:
    (i) with columns 3-5 of w1 zero the frame cannot matter: the reference runs on the lists of _ext.ball_query (pinned bit-exact to
    the oracle elsewhere) and zero frames;
    (ii) with the full w1 the reference runs on the lists and frames of ops.pe_geometry, whose per-centre operations are the fused
    kernel's; the bf16x3 kernel on the same geometry is held to its own bound.
    Centres whose frame is not finite (the kernels' ReLU turns a NaN into 0, the reference keeps it) are left out: at most 1 %.

    Measured on the MI355X, worst err / bound of (i), (ii), bf16x3 and the share of centres left out:
    (2,300)  r=0.1 S=64: 0.015 0.013 0.028 0 %    r=0.2 S=256: 0.010 0.011 0.022 0 %    r=0.3 S=32: 0.011 0.013 0.033 0 %
    (3,2048) r=0.1 S=64: 0.018 0.013 0.029 0 %    r=0.2 S=256: 0.012 0.013 0.025 0 %    r=0.3 S=32: 0.011 0.013 0.046 0 %"""
    from unopose_amd import ops
    from unopose_amd.pointnet2 import _ext

    x = real_clouds(B, N)
    folded = [(w.cuda(), b.cuda()) for w, b in P.make_weights(seed=int(1000 * r) + S)]
    lists, counts, frames = ops.pe_geometry(x, r, S)[0]
    ok = torch.isfinite(frames).all(2)
    left_out = 1.0 - ok.float().mean().item()
    assert left_out <= 0.01, left_out

    # (i)
    nofr = [(folded[0][0].clone(), folded[0][1])] + folded[1:]
    nofr[0][0][:, 3:] = 0
    ref, bound = P.pe_mlp_ref(x, r, _ext.ball_query(x, x, r, S), torch.zeros_like(frames), nofr, u=P.U_FP32)
    out = ops.pe_group_mlp_max(x, r, S, P.FoldedMLP(nofr).cuda(), bf16x3=False)
    w1 = worst(out, ref, bound, ok)
    assert float(ref.max()) > 0.1
    assert bool(((out.double() - ref).abs() <= bound)[ok].all()), ("(i)", w1)

    # (ii)
    mlp = P.FoldedMLP(folded).cuda()
    ref, bound = P.pe_mlp_ref(x, r, lists, frames, folded, u=P.U_FP32)
    out = ops.pe_group_mlp_max(x, r, S, mlp, bf16x3=False)
    w2 = worst(out, ref, bound, ok)
    _, bound3 = P.pe_mlp_ref(x, r, lists, frames, folded)
    out3 = ops.pe_mlp_max(x, r, S, mlp, (lists, counts, frames))
    w3 = worst(out3, ref, bound3, ok)
    print(f"real geometry ({B}, {N}) r={r} S={S}: fp32 (i) {w1:.4f}  fp32 (ii) {w2:.4f}  bf16x3 {w3:.4f}  left out {left_out:.3%}")
    assert bool(((out.double() - ref).abs() <= bound)[ok].all()), ("(ii)", w2)
    assert bool(((out3.double() - ref).abs() <= bound3)[ok].all()), ("bf16x3", w3)
