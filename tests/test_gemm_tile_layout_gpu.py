"""Index probes of the 256 x 256-tile GEMM kernel (csrc/gemm_kernel.h): which lane holds which output element.

Exact arithmetic: the operands are small integers, W picks ONE k per output column (W[n][k] = 1 iff k == n mod K), so
C[m][n] = A[m][n mod K] + b[n] with every value and every sum an integer far below 2^8 (bf16) / 2^24 (fp32).  A row, a column or a
lane quarter that the accumulator layout (AccTile) maps to the wrong place is an inequality under `torch.equal`, not noise inside a
tolerance.  The shapes are the smallest the 256-tile kernel takes (gemm.hip hands it launches of at least 5 / 8 of the CUs' worth of
tiles): ragged last row panels, more tiles than CUs (the stream continues into a second tile), one / two / an odd number of K-tiles,
three and nine column tiles.  The LayerNorm forms are not exact and stay with the tolerance tests of test_gemm_gpu.py and
test_layernorm_rows_gpu.py; one ragged case of the algebraic LayerNorm is added here with the bounds of
test_residual_and_layernorm_fold_vs_fp32_composite."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES_768 = [(256 * 90 + r, 768, K) for r in (1, 37, 255) for K in (64, 128, 192)]
SHAPES = SHAPES_768 + [(256 * 20 + 37, 2304, K) for K in (64, 128, 192)]


def _operands(M, N, K, dev="cuda"):
    """A (M, K) bf16, W (N, K) bf16, b (N,) fp32 and the exact C (M, N) fp32."""
    m = torch.arange(M, device=dev)[:, None]
    k = torch.arange(K, device=dev)[None, :]
    n = torch.arange(N, device=dev)
    a = ((7 * m + 3 * k) % 17 - 8).float()
    w = (k == (n % K)[:, None]).float()
    b = ((5 * n) % 7 - 3).float()
    c = a[:, n % K] + b
    return a.bfloat16().contiguous(), w.bfloat16().contiguous(), b.contiguous(), c


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_plain_relu_and_strided_outputs_are_exact(M, N, K):
    from unopose_amd import ops
    from unopose_amd._lib import call, ptr, stream_ptr

    a, w, b, c = _operands(M, N, K)
    assert torch.equal(ops.linear_bf16_hip(a, w, b).float(), c)
    assert torch.equal(ops.linear_bf16_hip(a, w, b, relu=True).float(), c.clamp(min=0))
    # row strides for A, W and C: the pad columns are never read / written
    ap = torch.full((M, K + 64), 7.0, device="cuda").bfloat16()
    ap[:, :K] = a
    wp = torch.full((N, K + 128), -3.0, device="cuda").bfloat16()
    wp[:, :K] = w
    cp = torch.zeros(M, N + 8, device="cuda", dtype=torch.bfloat16)
    call("unopose_linear_bf16_ld", ptr(ap), K + 64, ptr(wp), K + 128, ptr(b), ptr(cp), N + 8, M, N, K, 0, stream_ptr())
    assert torch.equal(cp[:, :N].float(), c) and float(cp[:, N:].abs().max()) == 0.0


@pytest.mark.parametrize("K", [64, 128, 192])
def test_gathered_rows_of_two_groups_are_exact(K):
    """unopose_linear_bf16_gather: output row r of tile t = A[row_list[256 t + r]] times the 256-row weight block of t's group;
    padding rows (-1) compute on row 0 and are nobody's."""
    from unopose_amd._lib import call, ptr, stream_ptr

    M, N = 3001, 512
    a, w, b, c = _operands(M, N, K)
    g = torch.Generator().manual_seed(K)
    tiles = (11, 6)  # tiles of group 0 / 1: 17 tiles on a grid of 24 workgroups
    rows = []
    for cnt, used in zip(tiles, (256 * 10 + 37, 256 * 5 + 255)):  # the last tile of each group is padded
        r = torch.full((cnt * 256,), -1, dtype=torch.int32)
        r[:used] = torch.randint(0, M, (used,), generator=g, dtype=torch.int32)
        rows.append(r)
    row_list = torch.cat(rows).cuda()
    cap_tiles = sum(tiles) + 3  # capacity beyond the tiles in use: never computed
    tile_info = torch.zeros(18, dtype=torch.int32)
    tile_info[0] = sum(tiles)
    tile_info[1], tile_info[2], tile_info[3] = 0, tiles[0], sum(tiles)
    tile_info = tile_info.cuda()
    row_list = torch.cat([row_list, torch.full((3 * 256,), -1, dtype=torch.int32, device="cuda")])
    out = torch.full((cap_tiles * 256, 256), 99.0, dtype=torch.bfloat16, device="cuda")
    call("unopose_linear_bf16_gather", ptr(a), M, K, ptr(w), N, ptr(b), ptr(row_list), ptr(tile_info), cap_tiles, ptr(out), stream_ptr())
    used = row_list[: sum(tiles) * 256]
    grp = (torch.arange(used.numel(), device="cuda") // 256 >= tiles[0]).long()
    valid = used >= 0
    src = used.clamp(min=0).long()
    want = torch.where(grp[:, None] == 0, c[src, :256], c[src, 256:])
    got = out[: used.numel()].float()
    assert torch.equal(got[valid], want[valid])
    assert torch.equal(out[used.numel():], torch.full_like(out[used.numel():], 99.0))  # tiles past tile_info[0] are not touched


@pytest.mark.parametrize("M,N,K", SHAPES_768)
def test_residual_stream_rows_and_partial_sums_are_exact(M, N, K):
    """ops.linear_residual_ with integer-valued x, zero shifts and LayerScale 1: the fp32 stream is x + C, the bf16 rows are
    bf16(x + C), the per-(row, column tile) partial sums and sums of squares are exact integers."""
    import torch.nn as nn
    from unopose_amd import ops

    a, w, b, c = _operands(M, N, K)
    lin = nn.Linear(K, N).cuda()
    with torch.no_grad():
        lin.weight.copy_(w.float())
        lin.bias.copy_(b)
    gamma = nn.Parameter(torch.ones(N, device="cuda"))
    m = torch.arange(M, device="cuda")[:, None]
    n = torch.arange(N, device="cuda")[None, :]
    x0 = ((3 * m + 11 * n) % 23 - 11).float().contiguous()
    x = x0.clone()
    with torch.no_grad():
        xb, stats = ops.linear_residual_(x, a, lin, gamma, None)
    want = x0 + c  # |.| <= 11 + 8 + 3
    assert torch.equal(x, want)
    assert torch.equal(xb.float(), want)
    assert float(ops.fold_shift(stats)[:M].abs().max()) == 0.0
    parts = want.view(M, N // 256, 256)
    assert torch.equal(stats[:M, :, 0], parts.sum(2))
    assert torch.equal(stats[:M, :, 1], (parts * parts).sum(2))


@torch.no_grad()
def test_layernorm_fold_on_a_ragged_row_count_vs_fp32_composite():
    """ops.linear_lnfold at M = 256 * 90 + 37, K = 768, N = 2304 behind ops.linear_residual_, against the fp32 composite: the bounds
    of test_gemm_gpu.test_residual_and_layernorm_fold_vs_fp32_composite."""
    import torch.nn as nn
    from unopose_amd import ops

    dev = torch.device("cuda")
    M, Kp, C, Nc = 256 * 90 + 37, 768, 768, 2304
    g = torch.Generator(device="cuda").manual_seed(M + Nc)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    a = rn(M, Kp).bfloat16()
    lin_p, lin_c, norm = nn.Linear(Kp, C).to(dev), nn.Linear(C, Nc).to(dev), nn.LayerNorm(C, eps=1e-6).to(dev)
    norm.weight.copy_(1 + 0.3 * rn(C))
    norm.bias.copy_(0.2 * rn(C))
    gamma = nn.Parameter(0.05 + 0.45 * torch.rand(C, device=dev, generator=g))
    x0 = (rn(M, C) * 2 + 0.5 * rn(1, C)).contiguous()
    x = x0.clone()
    mean0 = torch.zeros((M + 255) // 256 * 256, device=dev)
    mean0[:M] = x0.double().mean(1).float()
    xb, stats = ops.linear_residual_(x, a, lin_p, gamma, mean0)
    out = ops.linear_lnfold(xb, stats, lin_c, norm, gelu=False)
    xr = x0 + gamma * (a.float() @ lin_p.weight.T + lin_p.bias)
    ref = torch.nn.functional.layer_norm(xr, (C,), norm.weight, norm.bias, 1e-6) @ lin_c.weight.T + lin_c.bias
    assert (x - xr).abs().max().item() < 2e-2 and (x - xr).abs().mean().item() < 1.5e-3
    xc = x - mean0[:M, None]
    assert torch.equal(xb, xc.bfloat16())
    st = stats[:M].sum(1)
    assert (st[:, 0] - xc.sum(1)).abs().max().item() < 1e-2 and ((st[:, 1] - (xc * xc).sum(1)).abs() / (xc * xc).sum(1)).max().item() < 1e-5
    e = (out.float() - ref).abs()
    assert e.max().item() < 8e-2 and e.mean().item() < 5e-3, (e.max().item(), e.mean().item())
