"""GPU: the one-pass fp32 kernels between the GEMMs -- csrc/glue.hip, the three routes of csrc/bmm_f32.hip, add_layernorm and
bilinear_sample of csrc/fused.hip -- through the C ABI against the float64 references of tests/glue_ref.py, on that file's cases.  Every
output is allocated inside a NaN-filled (integers: -7) buffer: every element must lie within its derived bound (a NaN fails), and the guard
elements in front of, behind and beside the output must keep their bits.  tests/test_glue_ref_cpu.py shows that the mutants a kernel could
turn into leave these bounds on these cases.  The worst error / bound per kernel is printed by the last test."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import glue_ref as G  # noqa: E402

pytestmark = pytest.mark.gpu

RATIOS = {}
DEV = "cuda"


def _abi():
    from unopose_amd._lib import call, ptr, stream_ptr

    return call, ptr, stream_ptr


def _note(name, ratio):
    RATIOS[name] = max(RATIOS.get(name, 0.0), ratio)


def _ints(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


class Guarded:
    """An output of `shape` (rows x cols for 2-D placements) inside a buffer filled with NaN (integers: -7): 64 elements in front and behind
    a contiguous one; a row above and below and `col0` / the rest of the pitch `ld` beside a column block."""

    def __init__(self, shape, dtype, ld=None, col0=0):
        fill = float("nan") if dtype.is_floating_point else (171 if dtype == torch.uint8 else -7)
        if ld is None:
            n = 1
            for s in shape:
                n *= s
            self.buf = torch.full((n + 128,), fill, dtype=dtype, device=DEV)
            self.view = self.buf[64:64 + n].view(shape)
        else:
            rows, cols = shape
            self.buf = torch.full((rows + 2, ld), fill, dtype=dtype, device=DEV)
            self.view = self.buf[1:-1, col0:col0 + cols]
        self.fill = fill
        self.pristine = self.buf.clone()

    def take(self):
        """The output on the CPU, after checking that nothing around it was written."""
        torch.cuda.synchronize()
        got = self.view.clone()
        self.view.fill_(self.fill)
        assert torch.equal(_ints(self.buf), _ints(self.pristine)), "a guard element was written"
        return got.cpu()


def _run_all(name, runner, cases=None):
    K = G.KERNELS[name]
    amb, tot = 0.0, 0
    for case in (K.CASES if cases is None else cases):
        inp = K.inputs(case)
        ok, ratio = K.check(inp, runner(inp))
        assert ok, (name, case, ratio)
        a = inp.get("_ambiguous", (0, 0))
        amb, tot = amb + a[0], tot + a[1]
        _note(name, ratio)
    if tot:   # bf16 outputs: either neighbour is accepted on fewer than 1% of the elements
        assert amb / tot < G.AMBIGUOUS_SHARE, (name, amb / tot)


# ================================================================================================================================ bmm_f32
def _bmm_route(a4, b4, n, m):
    """The launcher's conditions (unopose_bmm_f32): both k strides 1, every other stride of both operands a multiple of 4, both base
    pointers on 16 bytes -> the vector route, on 64 x 64 tiles when n and m are both >= 256; anything else -> kernel<false>."""
    strides = [a4.stride(i) for i in (0, 1, 2)] + [b4.stride(i) for i in (0, 1, 2)]
    kvec = a4.stride(3) == 1 and b4.stride(3) == 1 and all(s % 4 == 0 for s in strides) and a4.data_ptr() % 16 == 0 and b4.data_ptr() % 16 == 0
    return ("kernel64" if n >= 256 and m >= 256 else "kernel<true>") if kvec else "kernel<false>"


def _bmm_place(X, layout):
    """The logical (Bo, Bi, rows, K) operand on the device, heads interleaved as the linear attention passes them (the head index between
    the row and the k index of the storage), the storage NaN wherever the kernel has no business reading."""
    Bo, Bi, r, K = X.shape
    P = (K + 3) // 4 * 4
    if layout == "kstride":   # storage (Bo, K, Bi, rows), as k^T v reads its (B, j, heads, 64) tensors: k stride Bi * rows
        st = torch.empty(Bo, K, Bi, r, device=DEV)   # (a fresh tensor: standard strides for dimensions of size 1 too, row stride 1)
        st.copy_(X.permute(0, 3, 1, 2))
        return st.permute(0, 2, 3, 1), st
    if layout == "pitch":   # row pitch P + 1 (odd): the head stride is not a multiple of 4
        P += 1
    flat = torch.full((Bo * r * Bi * P + 1,), float("nan"), device=DEV)
    st = flat[1:] if layout == "base" else flat[:-1]   # "base": the pointer one float into the buffer, every stride a multiple of 4
    st = st.view(Bo, r, Bi, P)
    st[..., :K] = X.permute(0, 2, 1, 3).to(DEV)
    return st[..., :K].permute(0, 2, 1, 3), flat


def _bmm_launch(a4, b4, alpha):
    call, ptr, stream_ptr = _abi()
    Bo, Bi, n, K = a4.shape
    m = b4.shape[2]
    out = Guarded((Bo, Bi, n, m), torch.float32)
    call("unopose_bmm_f32", ptr(a4), *a4.stride(), ptr(b4), *b4.stride(), ptr(out.view), Bo, Bi, n, m, K, float(alpha), stream_ptr())
    return out.take()


@torch.no_grad()
@pytest.mark.parametrize("bo,bi", G.BMM_BATCH)
@pytest.mark.parametrize("n,m", G.BMM_NM32 + G.BMM_NM64)
def test_bmm_f32_routes(n, m, bo, bi):
    """Every K of the list (K < 8: the vector route is all tail; 9, 12, 13, 257: vector steps and a tail, odd K: the last MFMA step half
    empty) on integer-valued (exact) and random operands, alpha 1 and 10.  The same data in four layouts:
      vec      rows padded to a multiple of 4 floats, aligned base: kvec holds -> kernel<true>, or kernel64 when n, m >= 256
      pitch    an odd row pitch: a stride % 4 != 0 -> kernel<false>
      base     the pitch of `vec`, the base pointer one float on: the 16-byte test fails -> kernel<false>
      kstride  k stride != 1 -> kernel<false>
    All routes feed the same (k, k + 1) pairs to the same MFMA chain: equal bits.  For n, m >= 256 the first 255 rows of A go through
    kernel<true> as well (n < 256 takes the 32 x 32 tiles) and must give the first 255 rows of kernel64's result."""
    big = n >= 256 and m >= 256
    for K in (G.BMM_K64 if big else G.BMM_K):
        for kind in ("int", "rand"):
            for alpha in G.BMM_ALPHA:
                inp = G.bmm.inputs((n, m, K, bo, bi, alpha, kind))
                outs = {}
                for layout in ("vec", "pitch", "base", "kstride"):
                    a4, keep_a = _bmm_place(inp["A"], layout)
                    b4, keep_b = _bmm_place(inp["B"], layout)
                    want = ("kernel64" if big else "kernel<true>") if layout == "vec" else "kernel<false>"
                    assert _bmm_route(a4, b4, n, m) == want, (layout, K)
                    outs[layout] = _bmm_launch(a4, b4, alpha)
                    if layout == "vec" and big:
                        assert _bmm_route(a4[:, :, :255], b4, 255, m) == "kernel<true>"
                        outs["vec255"] = _bmm_launch(a4[:, :, :255], b4, alpha)
                    del keep_a, keep_b
                ok, ratio = G.bmm.check(inp, outs["vec"])
                assert ok, ("vec", n, m, K, kind, alpha, ratio)
                _note("bmm_f32", ratio)
                for layout in ("pitch", "base", "kstride"):
                    assert torch.equal(_ints(outs[layout]), _ints(outs["vec"])), (layout, n, m, K, kind, alpha)
                if big:
                    assert torch.equal(_ints(outs["vec255"]), _ints(outs["vec"][:, :, :255].contiguous())), (n, m, K, kind, alpha)


# ================================================================================================== reductions over a cloud or a token list
@torch.no_grad()
def test_cloud_radius():
    """One workgroup per cloud, 256 threads striding over N: N < 256 leaves threads idle (their 0 must not win: radii are >= 0), 255 / 256 /
    257 straddle one full stride, 1000 and 5000 run the loop 4 and 20 times; the outliers sit in the first and last thread's share and at
    index 256 (the first element of the second stride)."""
    call, ptr, stream_ptr = _abi()

    def run(inp):
        p = inp["pts"].to(DEV)
        out = Guarded((p.shape[0],), torch.float32)
        call("unopose_cloud_radius", ptr(p), p.shape[0], p.shape[1], ptr(out.view), stream_ptr())
        return out.take()

    _run_all("cloud_radius", run)


@torch.no_grad()
def test_scale_by_radius():
    """One thread per element, cdiv(n, 256) workgroups per batch row: n = 1, 3, 255 a partly filled workgroup, 257 a second one with one
    element, 6144 = 24 full ones.  Bit-equal to the correctly rounded quotient / product."""
    call, ptr, stream_ptr = _abi()

    def run(inp):
        x, r = inp["x"].to(DEV), inp["radius"].to(DEV)
        out = Guarded(tuple(x.shape), torch.float32)
        call("unopose_scale_by_radius", ptr(x), x.shape[0], x.shape[1], ptr(r), inp["eps"], inp["mode"], ptr(out.view), stream_ptr())
        return out.take()

    _run_all("scale_by_radius", run)


@torch.no_grad()
def test_pose_score():
    """block_sum_256 twice on one LDS array.  The single non-zero weight at 0, N - 1, 255, 256, 257 is lost by a dropped lane, a dropped
    wave or an off-by-one stride; `dis == thr` must not count; all weights zero gives exactly 0."""
    call, ptr, stream_ptr = _abi()

    def run(inp):
        d, w = inp["dis"].to(DEV), inp["w"].to(DEV)
        out = Guarded((d.shape[0],), torch.float32)
        call("unopose_pose_score", ptr(d), ptr(w), d.shape[0], d.shape[1], inp["thr"], ptr(out.view), stream_ptr())
        return out.take()

    _run_all("pose_score", run)


@torch.no_grad()
def test_token_sum_bf16():
    """J < 4: the tail loop alone; 4: the four-chain loop alone; 5, 7, 2049: both (J % 4 = 1, 3, 1); C = 1, 64 a partly filled workgroup,
    300 a second one with 44 columns."""
    call, ptr, stream_ptr = _abi()

    def run(inp):
        x = inp["x"].bfloat16().to(DEV)
        B, J, C = x.shape
        out = Guarded((B, C), torch.float32)
        call("unopose_token_sum_bf16", ptr(x), B, J, C, ptr(out.view), stream_ptr())
        return out.take()

    _run_all("token_sum_bf16", run)


# =========================================================================================================================== 256-wide rows
@torch.no_grad()
def test_row_dot():
    """Four rows per workgroup: rows = 1, 3, 5, 1023 leave waves of the last workgroup without a row.  All four dtype forms."""
    call, ptr, stream_ptr = _abi()

    def run(inp):
        x = (inp["x"].bfloat16() if inp["x_bf16"] else inp["x"]).to(DEV)
        w = inp["w"].to(DEV)
        out = Guarded((x.shape[0],), torch.bfloat16 if inp["out_bf16"] else torch.float32)
        call("unopose_row_dot", ptr(x), inp["x_bf16"], ptr(w), inp["b"], x.shape[0], 256, ptr(out.view), inp["out_bf16"], stream_ptr())
        return out.take().float()

    _run_all("row_dot", run)


@torch.no_grad()
def test_normalize_rows():
    """Both input types, the three output modes (bf16; the bf16 values as fp32; unrounded fp32), temp 0.1 and 1.  Zero rows take the 1e-12
    clamp; the squares of the rows scaled by 1e-20 are subnormal, those of the rows scaled by 1e18 sum to just below FLT_MAX."""
    call, ptr, stream_ptr = _abi()

    def run(inp):
        x = (inp["x"].bfloat16() if inp["x_bf16"] else inp["x"]).to(DEV)
        out = Guarded((x.shape[0], 256), torch.float32 if inp["mode"] else torch.bfloat16)
        call("unopose_normalize_rows_bf16", ptr(x), inp["x_bf16"], x.shape[0], 256, inp["temp"], ptr(out.view), inp["mode"], stream_ptr())
        return out.take().float()

    _run_all("normalize_rows", run)


@torch.no_grad()
def test_overlap_scores():
    """n_out = n1 + n2: 2 (one element per cloud), 346 and 257 (a second workgroup), 513 (a third with one element); the concatenated form
    skips positions 0 and n1 + 1, the two-halves form reads cloud 2 of pair b from batch B + b.  +-100 saturate to exactly 1 and 0."""
    call, ptr, stream_ptr = _abi()

    def run(inp):
        s = (inp["scores"].bfloat16() if inp["x_bf16"] else inp["scores"]).to(DEV)
        n_tot = inp["n1"] + inp["n2"] + 2
        out = Guarded((inp["B"], n_tot - 2), torch.float32)
        call("unopose_overlap_scores", ptr(s), inp["x_bf16"], inp["B"], n_tot, inp["n1"], inp["halves"], ptr(out.view), stream_ptr())
        return out.take()

    _run_all("overlap_scores", run)


@torch.no_grad()
def test_rigid_rows_bf16():
    """One thread per point: N = 1, 255 a partly filled workgroup, 256 a full one, 257 a second with one point.  Bit-equal."""
    call, ptr, stream_ptr = _abi()

    def run(inp):
        p, t, R = inp["p"].to(DEV), inp["t"].to(DEV), inp["R"].to(DEV)
        out = Guarded(tuple(p.shape), torch.bfloat16)
        call("unopose_rigid_rows_bf16", ptr(p), p.shape[0], p.shape[1], ptr(t), ptr(R), ptr(out.view), stream_ptr())
        return out.take().float()

    _run_all("rigid_rows_bf16", run)


@torch.no_grad()
def test_nearest_partner_on_the_lattice():
    """Tiles of 256 points of the reduced cloud in LDS: 1 and 255 a partly filled tile, 256 exactly one, 257 / 513 / 700 a last tile of 1,
    1 and 188; the outputs 1, 255, 256, 300 / 513 / 700 likewise over the workgroups.  Exact distances: dmin bit-equal, the first index
    among the (many) ties, and `<= 0.25` with 0.25 attained."""
    call, ptr, stream_ptr = _abi()

    def run(inp):
        a, b = inp["a"].to(DEV), inp["b"].to(DEV)
        B, n, m = a.shape[0], a.shape[1], b.shape[1]
        nout = n if inp["over_b"] else m
        d, i, c = Guarded((B, nout), torch.float32), Guarded((B, nout), torch.int32), Guarded((B, nout), torch.uint8)
        call("unopose_nearest_partner", ptr(a), ptr(b), B, n, m, inp["over_b"], inp["thr"], ptr(d.view), ptr(i.view), ptr(c.view), stream_ptr())
        return d.take(), i.take(), c.take()

    _run_all("nearest_partner", run)


# ============================================================================================================================ data movement
@torch.no_grad()
def test_gather_rows():
    """The grid is min(cdiv((J + prepend) words, 256), 4096) workgroups: the first case has 4201 * 256 words (4201 > 4096: the grid-stride
    loop runs for the first 105 workgroups), the second 4200 * 256 (one more than the cap as well); the others fit.  idx = N - 1 (off 0),
    idx = N with off 1 (the last row) and idx = 0 with off 1 (the alternative row), int32 and int64 indices, the alternative row per batch
    and one for all (stride 0)."""
    call, ptr, stream_ptr = _abi()

    def run(inp):
        feats, idx = inp["feats"].to(DEV), inp["idx"].to(DEV)
        alt = None if inp["alt"] is None else inp["alt"].to(DEV)
        B, N, words = feats.shape
        J = idx.shape[1]
        out = Guarded((B, J + inp["prepend"], words), torch.int32)
        call("unopose_gather_rows", ptr(feats), B, N, words * 4, ptr(idx), int(idx.dtype == torch.int64), J, inp["off"],
             None if alt is None else ptr(alt), inp["alt_stride"] * 4, inp["prepend"], ptr(out.view), stream_ptr())
        return out.take()

    _run_all("gather_rows", run)


@torch.no_grad()
def test_copy_rows():
    """The grid is min(cdiv(words, 256), 64) workgroups per row: 1 word = one thread; 16384 words = exactly the capped grid, no second trip;
    16385 words: thread 0 of workgroup 0 takes a second trip of the grid-stride loop.  Source stride 0 (one row for all) and words + 3; the
    destination pitch is words + 5, and the 5 words between the rows stay untouched."""
    call, ptr, stream_ptr = _abi()

    def run(inp):
        src = inp["src"].to(DEV)
        out = Guarded((inp["rows"], inp["words"]), torch.int32, ld=inp["dst_pitch"])
        call("unopose_copy_rows", ptr(src), inp["src_pitch"] * 4, ptr(out.view), inp["dst_pitch"] * 4, inp["rows"], inp["words"] * 4, stream_ptr())
        return out.take()

    _run_all("copy_rows", run)


@torch.no_grad()
def test_nan_to_num_multi():
    """A table of five tensors in one launch, grid (min(cdiv(max_size, 256), 64) = 64, 5): the tensors of 1, 255 and 256 elements use part
    of one workgroup, 64 * 256 + 1 takes one element into the second trip of the grid-stride loop, 100000 runs it 7 times.  Every finite
    bit pattern stays; the guards (NaN: a kernel that strayed would replace them) keep theirs."""
    call, ptr, stream_ptr = _abi()

    def run(inp):
        gs = [Guarded((x.numel(),), torch.float32) for x in inp["tensors"]]
        for g, x in zip(gs, inp["tensors"]):
            g.view.copy_(x.to(DEV))
        table = torch.tensor([g.view.data_ptr() for g in gs] + [x.numel() for x in inp["tensors"]], dtype=torch.int64, device=DEV)
        n = len(gs)
        call("unopose_nan_to_num_multi", ptr(table), ptr(table[n:]), n, max(G.NAN_SIZES), *inp["repl"], stream_ptr())
        return [g.take() for g in gs]

    _run_all("nan_to_num_multi", run)


@torch.no_grad()
@pytest.mark.parametrize("S", (14, 224, 518))
def test_patchify(S):
    """g = S / 14 patches per side: 1 (one workgroup per crop, 294 to 352 column pairs over 256 threads), 16 and 37 (the production crop);
    (na, nb) = (1, 0) without a second tensor, (2, 3) with the crop index crossing from a to b.  Kp = 588 no padding, 640 / 704 zero columns;
    the split form (Kp = 608, 640) equals ops.split_f32 of the fp32 patch matrix bit for bit, and the CPU's split layout."""
    from unopose_amd import ops

    call, ptr, stream_ptr = _abi()

    def run(inp):
        a = inp["a"].to(DEV)
        b = None if inp["b"] is None else inp["b"].to(DEV)
        na, nb = a.shape[0], 0 if b is None else b.shape[0]
        rows = (na + nb) * (S // 14) ** 2
        out = Guarded((rows, inp["Kp"] * (2 if inp["split"] else 1)), torch.bfloat16)
        call("unopose_patchify_split" if inp["split"] else "unopose_patchify_bf16", ptr(a), na, None if b is None else ptr(b), nb, S, inp["Kp"],
             ptr(out.view), stream_ptr())
        got = out.take()
        if inp["split"]:
            want = ops.split_f32(G.patch_matrix_64(inp["a"], inp["b"], inp["Kp"]).to(DEV)).cpu()
            assert torch.equal(_ints(got), _ints(want)), "patchify_split differs from split_f32 of the patch matrix"
        return got

    _run_all("patchify", run, [c for c in G.patchify.CASES if c[0] == S])


# ============================================================================================================================ fused.hip
def _ln_launch(inp, ld_extra=8, col0=4):
    call, ptr, stream_ptr = _abi()
    a = (inp["a"].bfloat16() if inp["a_bf16"] else inp["a"]).to(DEV)
    b = None if inp["b"] is None else (inp["b"].bfloat16() if inp["b_bf16"] else inp["b"]).to(DEV)
    w, bias = inp["w"].to(DEV), inp["bias"].to(DEV)
    rows, C = a.shape
    out = Guarded((rows, C), torch.bfloat16 if inp["out_bf16"] else torch.float32, ld=C + ld_extra, col0=col0)
    call("unopose_add_layernorm_strided", ptr(a), inp["a_bf16"], None if b is None else ptr(b), inp["b_bf16"], ptr(w), ptr(bias), rows, C,
         inp["eps"], ptr(out.view), inp["out_bf16"], C + ld_extra, stream_ptr())
    return out, out.take().float()


def _ln_vec4(C, out):
    """The launcher's condition: C and the output pitch multiples of 4, and the base pointers of a, b (fresh allocations) and out on four
    elements."""
    v = out.view
    return C % 4 == 0 and v.stride(0) % 4 == 0 and v.data_ptr() % (4 * v.element_size()) == 0


@torch.no_grad()
@pytest.mark.parametrize("C", G.LN_C)
def test_add_layernorm(C):
    """C = 4, 100, 256, 1000, 1024 with the output block at column 4 of a pitch of C + 8: add_layernorm_vec4_kernel (C % 4 == 0,
    ld_out % 4 == 0, aligned bases) -- 4: one lane; 100: 25 lanes of the first group; 1000: the fourth lane group partly filled; 1024: all
    four full, the ABI's maximum.  C = 30, 257: add_layernorm_kernel (C % 4 != 0), 257 with one channel in the fifth of its 16 steps.
    rows = 1, 5, 777: the last workgroup has waves without a row.  All twelve dtype forms, the row families of test_layernorm_rows_gpu.py."""
    for case in G.add_layernorm.CASES:
        if case[0] != C:
            continue
        inp = G.add_layernorm.inputs(case)
        out, got = _ln_launch(inp)
        assert _ln_vec4(C, out) == (C % 4 == 0), case
        ok, ratio = G.add_layernorm.check(inp, got)
        assert ok, (case, ratio)
        _note("add_layernorm", ratio)


@torch.no_grad()
@pytest.mark.parametrize("C", (4, 256, 1024))
def test_add_layernorm_block_at_an_unaligned_column(C):
    """C % 4 == 0 and ld_out % 4 == 0, but the output block starts at column 3: its base pointer is not on four elements, so the launcher
    must take add_layernorm_kernel (it used to choose from C and ld_out alone and issue 16-byte stores at 12-byte offsets).  Same bound."""
    for case in G.add_layernorm.CASES:
        if case[0] != C or case[1] == 1:
            continue
        inp = G.add_layernorm.inputs(case)
        out, got = _ln_launch(inp, col0=3)
        assert not _ln_vec4(C, out) and out.view.stride(0) % 4 == 0
        ok, ratio = G.add_layernorm.check(inp, got)
        assert ok, (case, ratio)
        _note("add_layernorm", ratio)


@torch.no_grad()
@pytest.mark.parametrize("side,H,W", G.BILINEAR_GEOM)
def test_bilinear_sample(side, H, W):
    """One wavefront per pixel, four per workgroup.  (16, 224, 224) and (37, 518, 518): the model's crops, scale 2 / 7; (1, 14, 14): one
    token, every cell of the 4 x 4 map on a border; (4, 56, 42) and (16, 224, 160): H != W, so a row / column mix-up or the wrong scale on
    an axis shows; (5, 70, 70): an odd side.  Every border pixel (the clamp to the first tap, y1 = y0 at the far edge) and 2000 random ones;
    fp32 and bf16 maps; with tok_offset = 5 the prefix tokens hold 1e9, which any read of them would show."""
    call, ptr, stream_ptr = _abi()

    def run(inp):
        z = (inp["z"].bfloat16() if inp["z_bf16"] else inp["z"]).to(DEV)
        ch = inp["choose"].to(DEV)
        out = Guarded((1, ch.shape[1], 256), torch.float32)
        call("unopose_bilinear_sample_tokens", ptr(z), inp["z_bf16"], ptr(ch), 1, side, ch.shape[1], H, W, inp["off"], inp["off"] + side * side,
             ptr(out.view), stream_ptr())
        return out.take()

    _run_all("bilinear_sample", run, [c for c in G.bilinear_sample.CASES if c[:3] == (side, H, W)])


def test_zz_print_the_ratio_table():
    if RATIOS:
        print("\n" + G.ratio_table(RATIOS, "MI355X"))
