"""GPU: every ViT attention kernel against the float64 reference of tests/vit_attn_ref.py, ELEMENTWISE against a bound that is a
multiple of the softmax-weighted magnitude A (bf16: 1.05 * 2^-7 A; fp32 class: the derived hard bound AND C32 * A), on probe inputs
that put weight where these kernels can go wrong -- every key slot, the last key, the first key of the partial tile, chunk borders,
a reference point that moves in every tile -- at sequence lengths on both sides of every dispatch threshold, with B * H that is and
is not a multiple of 8, H = 12 and H != 12.  tests/test_vit_attn_ref_cpu.py shows on the CPU that the mutants these probes are for
leave the bounds by 4x and more.

  bf16 (unopose_vit_attention)   vit_attn_kernel<1,1,4>  T < 512;  <2,2,4>  512 <= T < 1024;  vit_attn_kernel_dma<4>  T >= 1024;
                                 <2,2,8>  T >= 1024 with a qkv image of 2 GiB or more (test_two_gib_dispatch_boundary)
  fp32 class                     unopose_vit_attention_f32, _f32_split (attn_f32.hip), _f32_ss (vit_attn_f32s.hip)
  (the stages all of them share: csrc/vit_attn_common.h)

Each check prints `PROBE <kernel> T B H family worst err/bound` (pytest -s shows them)."""
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vit_attn_ref as V  # noqa: E402

pytestmark = pytest.mark.gpu
BF = torch.bfloat16

ROUTE_NAME = {0: "vit_attn_kernel<1,1,4>", 1: "vit_attn_kernel<2,2,4>", 2: "vit_attn_kernel_dma<4>", 3: "vit_attn_kernel<2,2,8>"}
# the lengths put: a chunk end (128, 512, 1024), one key into a tile or chunk (33, 129, 513, 1025, 1153) and one key short of one
# (31, 511, 767, 1023, 1535), a last query block of one row, a last workgroup with inactive waves, a single token
T_BF16 = {0: (1, 31, 32, 33, 128, 129, 261, 511), 1: (512, 513, 545, 767, 1023), 2: (1024, 1025, 1153, 1374, 1535)}
BH_BF16 = ((1, 12), (3, 3), (2, 12))      # B * H = 12 and 9 (both through the `bh >= BH` guard) and 24
T_F32 = (1, 33, 129, 261, 385, 513, 1025, 1374)
BH_F32 = ((3, 3), (1, 12))
EVERYWHERE = ("sharp", "match")
AT_3_3 = ("lastkey", "stair+9", "stair+5", "stair-9")


def _families(B, H):
    return EVERYWHERE + (AT_3_3 if (B, H) == (3, 3) else ())


def _seed(T, B, H, family):
    return 100000 * list(V.FAMILIES).index(family) + 64 * T + 8 * B + H


def _route(T, H):
    from unopose_amd import _lib

    return _lib.lib().unopose_vit_attention_route(T, H)


def _check(bad, kernel, T, B, H, family, out, ref, bound, what=""):
    """Elementwise `err <= bound`; failures are collected so that one run reports every figure."""
    r, (b, t, c) = V.worst(out, ref, bound)
    print("PROBE %-24s T=%-5d B=%d H=%-5d %-8s %s worst err/bound = %.3f" % (kernel, T, B, H, family, what, r))
    if not bool(((out.to(V.F64) - ref).abs() <= bound).all()):
        bad.append("%s T=%d B=%d H=%d %s %s: %s" % (kernel, T, B, H, family, what, V.describe(out, ref, bound)))


def _f32_outputs(x, H):
    """The three fp32-class entry points on one fp32 qkv (B,T,3 H 64): [(name, out float64, the qkv it actually saw)]; also asserts that
    _f32_split is split_f32 of _f32, bit for bit."""
    from unopose_amd import ops

    B, T, C3 = x.shape
    o32 = ops.vit_attention(x, H)
    assert o32.dtype == torch.float32 and o32.shape == (B, T, C3 // 3)
    osp = ops.vit_attention_f32_split(x, H)
    assert torch.equal(osp, ops.split_f32(o32.reshape(B * T, C3 // 3))), "the split output is not split_f32 of the fp32 output"
    qs = ops.split_f32(x.reshape(B * T, C3))
    oss = ops.vit_attention_f32_ss(qs, B, T, H)
    return [("vit_attention_f32", o32.to(V.F64), x),
            ("vit_attention_f32_ss", V.from_split_layout(oss).reshape(B, T, C3 // 3), V.from_split_layout(qs).reshape(B, T, C3))]


# ------------------------------------------------------------------------------------------------------------- bf16
@torch.no_grad()
@pytest.mark.parametrize("T", [T for r in sorted(T_BF16) for T in T_BF16[r]])
def test_bf16_kernels_elementwise_vs_float64(T):
    from unopose_amd import ops

    route = [r for r in T_BF16 if T in T_BF16[r]][0]
    bad = []
    for B, H in BH_BF16:
        assert _route(T, H) == route
        for family in _families(B, H):
            x = V.FAMILIES[family](B, T, H, _seed(T, B, H, family), bf16=True).cuda()
            out = ops.vit_attention(x.to(BF), H)
            assert out.dtype == BF and out.shape == (B, T, H * 64)
            ref, A = V.vit_attn_ref(x, H)
            _check(bad, ROUTE_NAME[route], T, B, H, family, out, ref, V.bf16_bound(A))
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------------- fp32 class
@torch.no_grad()
@pytest.mark.parametrize("T", T_F32)
def test_fp32_class_kernels_elementwise_vs_float64(T):
    bad = []
    for B, H in BH_F32:
        for family in _families(B, H):
            x = V.FAMILIES[family](B, T, H, _seed(T, B, H, family), bf16=False).cuda()
            for name, out, seen in _f32_outputs(x, H):
                ref, A = V.vit_attn_ref(seen, H)
                _check(bad, name, T, B, H, family, out, ref, V.f32_hard_bound(seen, H, A), "hard ")
                _check(bad, name, T, B, H, family, out, ref, V.C32 * A, "sharp")
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ batch independence
@torch.no_grad()
@pytest.mark.parametrize("T", [261, 545, 1153])
def test_an_image_does_not_depend_on_its_batch(T):
    """One workgroup computes an (image, head, query block) in a fixed key order that does not depend on B: out(B = 2)[b] must be the
    single-image run of image b BIT FOR BIT, on the input whose neighbour image holds exactly what each query looks for."""
    from unopose_amd import ops

    bad = []
    for H in (12, 3):
        xb = V.bait(2, T, H, _seed(T, 2, H, "bait"), bf16=True).cuda()
        both = ops.vit_attention(xb.to(BF), H)
        ref, A = V.vit_attn_ref(xb, H)
        _check(bad, ROUTE_NAME[_route(T, H)], T, 2, H, "bait", both, ref, V.bf16_bound(A))
        for b in range(2):
            assert torch.equal(both[b:b + 1], ops.vit_attention(xb[b:b + 1].to(BF).contiguous(), H)), ("bf16", H, b)
        x = V.bait(2, T, H, _seed(T, 2, H, "bait"), bf16=False).cuda()
        qs = ops.split_f32(x.reshape(2 * T, 3 * H * 64))
        for name, out, seen in _f32_outputs(x, H):
            ref, A = V.vit_attn_ref(seen, H)
            _check(bad, name, T, 2, H, "bait", out, ref, V.f32_bound(seen, H, A), "both ")
        o32, osp, oss = ops.vit_attention(x, H), ops.vit_attention_f32_split(x, H), ops.vit_attention_f32_ss(qs, 2, T, H)
        for b in range(2):
            one = x[b:b + 1].contiguous()
            assert torch.equal(o32[b:b + 1], ops.vit_attention(one, H)), ("f32", H, b)
            assert torch.equal(osp[b * T:(b + 1) * T], ops.vit_attention_f32_split(one, H)), ("f32_split", H, b)
            assert torch.equal(oss[b * T:(b + 1) * T], ops.vit_attention_f32_ss(qs[b * T:(b + 1) * T].contiguous(), 1, T, H)), ("f32_ss", H, b)
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------------------ guards
@torch.no_grad()
@pytest.mark.parametrize("T", [33, 545, 1025])
def test_nothing_past_the_sequence_is_read_or_written(T):
    """B = 1 through the C ABI on views into larger allocations: 256 rows of NaN after qkv (in both planes of the split layout), 64
    sentinel rows after out.  The result is finite, within the bound, bit-equal to the plain call, and the sentinel rows are untouched.
    (Nothing is provoked: the kernels clamp rows to T - 1 or read through a per-image buffer descriptor.)"""
    from unopose_amd import ops
    from unopose_amd._lib import call, ptr, stream_ptr

    H, C = 12, 768
    SENT = 7.0
    bad = []

    def guarded(name, rows_in, width_out, dtype_out):
        buf = torch.full((T + 256, rows_in.shape[1]), float("nan"), dtype=rows_in.dtype, device="cuda")
        buf[:T] = rows_in
        outbuf = torch.full((T + 64, width_out), SENT, dtype=dtype_out, device="cuda")
        call(name, ptr(buf), 1, T, H, ptr(outbuf), stream_ptr())
        torch.cuda.synchronize()
        assert bool((outbuf[T:] == SENT).all()), name + ": rows past the output were written"
        assert bool(torch.isnan(buf[T:]).all())
        return outbuf[:T]

    for family in ("lastkey", "match"):
        xb = V.FAMILIES[family](1, T, H, _seed(T, 1, H, family), bf16=True).cuda()
        out = guarded("unopose_vit_attention", xb.to(BF).reshape(T, 3 * C), C, BF)
        assert bool(torch.isfinite(out.float()).all())
        assert torch.equal(out, ops.vit_attention(xb.to(BF), H)[0])
        ref, A = V.vit_attn_ref(xb, H)
        _check(bad, ROUTE_NAME[_route(T, H)], T, 1, H, family, out[None], ref, V.bf16_bound(A), "guard")

        x = V.FAMILIES[family](1, T, H, _seed(T, 1, H, family), bf16=False).cuda()
        ref, A = V.vit_attn_ref(x, H)
        o32 = guarded("unopose_vit_attention_f32", x.reshape(T, 3 * C), C, torch.float32)
        assert bool(torch.isfinite(o32).all()) and torch.equal(o32, ops.vit_attention(x, H)[0])
        _check(bad, "vit_attention_f32", T, 1, H, family, o32[None], ref, V.f32_bound(x, H, A), "guard")
        osp = guarded("unopose_vit_attention_f32_split", x.reshape(T, 3 * C), 2 * C, BF)
        assert bool(torch.isfinite(osp.float()).all()) and torch.equal(osp, ops.vit_attention_f32_split(x, H))
        qs = ops.split_f32(x.reshape(T, 3 * C))
        oss = guarded("unopose_vit_attention_f32_ss", qs, 2 * C, BF)
        assert bool(torch.isfinite(oss.float()).all()) and torch.equal(oss, ops.vit_attention_f32_ss(qs, 1, T, H))
        seen = V.from_split_layout(qs).reshape(1, T, 3 * C)
        ref, A = V.vit_attn_ref(seen, H)
        _check(bad, "vit_attention_f32_ss", T, 1, H, family, V.from_split_layout(oss)[None], ref, V.f32_bound(seen, H, A), "guard")
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------- the 2-GiB dispatch boundary
@torch.no_grad()
@pytest.mark.parametrize("H", [5456, 5457])
def test_two_gib_dispatch_boundary(H):
    """B = 1, T = 1025.  H = 5456: the qkv image is 2 147 481 600 B < 2^31, so vit_attn_kernel_dma runs with its 32-bit offsets at the
    top of their range; H = 5457: the image is >= 2^31, the only way to reach vit_attn_kernel<2,2,8>.  `sharp` drawn on the device as
    bf16 (1.07e9 values, 2.1 GiB; 2.8 GiB with the output); reference and bound on heads 0, 1, 7, 8, H // 2, H - 2, H - 1.
    Wall time of the whole case (input, kernel, reference, comparison), measured 2026-10-20 on an MI355X: 0.04 s (H = 5456) and 0.01 s
    (H = 5457), so the full randn stays: tiling a 64-head block would make heads h and h + 64 indistinguishable for nothing."""
    from unopose_amd import ops

    T = 1025
    t0 = time.perf_counter()
    assert _route(T, H) == (2 if H == 5456 else 3) and (T * 3 * H * 64 * 2 < 2 ** 31) == (H == 5456)
    x = V.sharp_on_device(1, T, H, 5 + H, "cuda")
    out = ops.vit_attention(x, H)
    heads = sorted({0, 1, 7, 8, H // 2, H - 2, H - 1})
    ref, A = V.vit_attn_ref(x, H, heads)
    sel = out.reshape(1, T, H, 64)[:, :, torch.as_tensor(heads, device="cuda")].reshape(1, T, len(heads) * 64)
    bad = []
    _check(bad, ROUTE_NAME[_route(T, H)], T, 1, H, "sharp", sel, ref, V.bf16_bound(A), "heads %s" % heads)
    torch.cuda.synchronize()
    print("PROBE two-GiB case H=%d wall time %.2f s" % (H, time.perf_counter() - t0))
    assert not bad, "\n".join(bad)



# ---------------------------------------------------------------------------------------------------- dispatch guard
def test_dispatch_thresholds_are_where_the_probe_lengths_assume():
    """The T lists above sit on both sides of the launcher's thresholds.  unopose_vit_attention_route is the function the launcher
    itself dispatches on: if 512, 1024 or the 2-GiB rule moves, this fails and the lengths are chosen again."""
    for route, Ts in T_BF16.items():
        for H in (3, 12):
            assert [_route(T, H) for T in Ts] == [route] * len(Ts)
    assert [_route(T, 12) for T in (511, 512, 1023, 1024)] == [0, 1, 1, 2]
    assert _route(1025, 5456) == 2 and _route(1025, 5457) == 3 and _route(1023, 5457) == 1 and _route(511, 5457) == 0
    # every route has lengths on it
    assert set(T_BF16) == {0, 1, 2} and all(len(v) >= 5 for v in T_BF16.values())
