"""GPU: the correspondence transformer's token attention -- csrc/attn.hip (bf16: the LDS-DMA RPE kernel, the fragment-load RPE kernel,
the cross kernel), csrc/attn_f32.hip (fp32 class, RPE and cross) and `ops.token_attention` -- and the producers of its zero-padded V^T
operand (csrc/gemm_small.hip EPI 4, csrc/glue.hip transpose_pad), against a plain float64 reference, across key counts, query counts,
batches, row strides and adversarial values.

Reference: P = softmax(0.125 (q_h . k_j + qp_h . E[n, j])), out = P v per head h (q_h, k_j, v_j: 64 channels of head h; qp_h: the
folded RPE query, 256 channels).  Each element of a result is checked against a bound derived from the arithmetic (`reference`):
  * score error D_j (per query row, head and key): fp32 accumulation of the MFMA products, c_s * 0.125 * (sum |q_h||k_j| + sum
    |qp_h||E_j|) with c_s = 2^-16 (bf16 operands: exact products, ~2 x 32 accumulator roundings) or 2^-15 (fp32 class: the hi / lo split
    drops lo.lo, ~3 x 2^-18 per product, plus 3 x the roundings), plus whatever uncertainty the operands themselves carry (op level);
  * a score error moves P_j by P_j (D_j + sum_i P_i D_i): sum_j P_j |v_j| D_j + (sum_j P_j |v_j|) (sum_i P_i D_i), counted twice;
  * P.v: bf16 P (2^-9 per weight) and bf16 output (2^-9 of the value), each counted twice: 2^-8 sum_j P_j |v_j| + 2^-8 |out|, plus
    m 2^-23 sum_j P_j |v_j| of fp32 accumulation; fp32 class: 2^-15 sum_j P_j |v_j| + 2^-20 |out|.
The mean error is checked as well on random data: it must stay well inside the mean bound (a systematic error -- a key miscounted, a
dropped lo term -- moves every element, independent roundings do not)."""
import ctypes
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
KP = 224  # padded key count of both kernels (TA_MP / AF_MP) = unopose_token_attention_key_pad()
MEAN_FRAC = 0.3  # mean |error| / mean bound (independent roundings on random data: ~0.2 in bf16)


def _lib():
    from unopose_amd import _lib

    return _lib


def vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _call(name, *args):
    L = _lib()
    L.call(name, *args)


# ------------------------------------------------------------------------------------------ float64 reference and its bound
CONST = {  # c_s, P.v relative (without the m term), output relative
    BF: (2.0 ** -16, 2.0 ** -8, 2.0 ** -8),
    F32: (2.0 ** -15, 2.0 ** -15, 2.0 ** -20),
}


def reference(q, k, v, qp=None, E=None, *, dt, dq=None, dk=None, dv=None, dqp=None, dE=None, rs=0.0, chunk=1 << 24):
    """q (B,n,256), k / v (B,m,256), qp (B,n,1024) = 4 heads x 256, E (B,n,m,256): any dtype, used exactly (float64).
    d*: optional per-element uncertainty of an operand (op level: the projections' rounding); rs: relative rounding of the scores
    themselves (the torch composite rounds them to its dtype).  Returns (out, bound), both (B,n,256) float64."""
    c_s, pv_rel, out_rel = CONST[dt]
    B, n, _ = q.shape
    m = k.shape[1]
    d = lambda t: None if t is None else t.double()  # noqa: E731
    k4, v4 = d(k).reshape(B, m, 4, 64), d(v).reshape(B, m, 4, 64)
    ka, va = k4.abs(), v4.abs()
    dk4 = None if dk is None else d(dk).reshape(B, m, 4, 64)
    dv4 = None if dv is None else d(dv).reshape(B, m, 4, 64)
    if dk4 is not None:
        ka = ka + dk4
    rows = max(1, chunk // max(1, B * m * 256))
    outs, bounds = [], []
    for r0 in range(0, n, rows):
        r1 = min(n, r0 + rows)
        q4 = d(q[:, r0:r1]).reshape(B, r1 - r0, 4, 64)
        qa = q4.abs() if dq is None else q4.abs() + d(dq[:, r0:r1]).reshape(B, r1 - r0, 4, 64)
        s = torch.einsum("bnhc,bmhc->bhnm", q4, k4)
        sa = torch.einsum("bnhc,bmhc->bhnm", qa, ka)
        u = torch.zeros_like(s)
        if dq is not None:
            u += torch.einsum("bnhc,bmhc->bhnm", d(dq[:, r0:r1]).reshape(B, r1 - r0, 4, 64), k4.abs())
        if dk4 is not None:
            u += torch.einsum("bnhc,bmhc->bhnm", qa, dk4)
        if qp is not None:
            p4 = d(qp[:, r0:r1]).reshape(B, r1 - r0, 4, 256)
            Ec = d(E[:, r0:r1])
            pa = p4.abs() if dqp is None else p4.abs() + d(dqp[:, r0:r1]).reshape(B, r1 - r0, 4, 256)
            Ea = Ec.abs() if dE is None else Ec.abs() + d(dE[:, r0:r1])
            s += torch.einsum("bnhd,bnmd->bhnm", p4, Ec)
            sa += torch.einsum("bnhd,bnmd->bhnm", pa, Ea)
            if dqp is not None:
                u += torch.einsum("bnhd,bnmd->bhnm", d(dqp[:, r0:r1]).reshape(B, r1 - r0, 4, 256), Ec.abs())
            if dE is not None:
                u += torch.einsum("bnhd,bnmd->bhnm", pa, d(dE[:, r0:r1]))
        P = torch.softmax(0.125 * s, dim=-1)
        D = 0.125 * (c_s * sa + u + rs * sa) + c_s  # (+ c_s: the exponential's own rounding)
        o = torch.einsum("bhnm,bmhc->bnhc", P, v4)
        A = torch.einsum("bhnm,bmhc->bnhc", P, va)
        PD = P * D
        T = torch.einsum("bhnm,bmhc->bnhc", PD, va) + A * PD.sum(-1).permute(0, 2, 1).unsqueeze(-1)
        bound = (pv_rel + (m * 2.0 ** -23 if dt == BF else 0.0)) * A + out_rel * o.abs() + 2 * T + 2.0 ** -120
        if dv4 is not None:
            bound += 2 * torch.einsum("bhnm,bmhc->bnhc", P, dv4)
        outs.append(o.reshape(B, r1 - r0, 256))
        bounds.append(bound.reshape(B, r1 - r0, 256))
    return torch.cat(outs, 1), torch.cat(bounds, 1)


def check(out, ref, bound, what="", mean=True):
    e = (out.double() - ref).abs()
    bad = ~(e <= bound)  # (NaN fails)
    if bad.any():
        idx = tuple(int(i) for i in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {e.numel()} elements outside the bound; first at {idx}: got "
                             f"{out[idx].item()!r}, want {ref[idx].item()!r} +- {bound[idx].item():.3e}")
    em, bm = e.mean().item(), bound.mean().item()
    assert not mean or em <= MEAN_FRAC * bm, f"{what}: mean error {em:.3e} vs mean bound {bm:.3e}"


# ------------------------------------------------------------------------------------------ kernel-level calls
def pack(layout, q, qp, k, v):
    """Lay the operands out as the wrapper passes them, return the views the kernel reads and their row strides:
    dense: separate tensors (ld 256, qp ld 1024); split: q | qp (ld 1280) and k | v (ld 512), as the cross layers' projections;
    self: q | qp | k | v (ld 1792; without RPE q | k | v, ld 768), the self layer's one projection (n == m)."""
    rpe = qp is not None
    if layout == "dense":
        return dict(q=q.contiguous(), ldq=256, qp=qp.contiguous() if rpe else None, ldqp=1024 if rpe else 0, k=k.contiguous(), ldk=256)
    if layout == "split":
        yq = torch.cat([q, qp], -1) if rpe else q.contiguous()
        ykv = torch.cat([k, v], -1)
        return dict(q=yq, ldq=yq.shape[-1], qp=yq[..., 256:] if rpe else None, ldqp=yq.shape[-1] if rpe else 0, k=ykv, ldk=512)
    assert layout == "self" and q.shape[1] == k.shape[1]
    y = torch.cat([q, qp, k, v] if rpe else [q, k, v], -1)
    W = y.shape[-1]
    return dict(q=y, ldq=W, qp=y[..., 256:1280] if rpe else None, ldqp=W if rpe else 0, k=y[..., W - 512:], ldk=W)


def vt_of(v):
    """The kernels' V^T operand: (B, 256, 224), keys >= m exactly zero."""
    B, m, C = v.shape
    vt = torch.zeros(B, C, KP, dtype=v.dtype, device=v.device)
    vt[:, :, :m] = v.transpose(1, 2)
    return vt


def attend(o, vt, E, B, n, m, dt):
    out = torch.full((B, n, 256), float("nan"), dtype=dt, device="cuda")  # every element must be written
    name = "unopose_token_attention" if dt == BF else "unopose_token_attention_f32"
    _call(name, vp(o["q"]), o["ldq"], vp(o["k"]), o["ldk"], vp(vt), vp(o["qp"]), o["ldqp"], vp(E), B, n, m, 0.125, vp(out),
          _lib().stream_ptr())
    return out


def operands(dt, B, n, m, rpe, seed, qs=1.0, ks=1.0, vs=1.0, ps=0.25, es=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s, sc: (torch.randn(*s, generator=g, device="cuda") * sc).to(dt)  # noqa: E731
    q, k, v = r(B, n, 256, sc=qs), r(B, m, 256, sc=ks), r(B, m, 256, sc=vs)
    qp = r(B, n, 1024, sc=ps) if rpe else None
    E = r(B, n, m, 256, sc=es) if rpe else None
    return q, qp, k, v, E


KERNELS = [pytest.param(dt, rpe, id=f"{'bf16' if dt == BF else 'f32'}-{'rpe' if rpe else 'cross'}") for dt in (BF, F32) for rpe in (True, False)]
SWEEP_M = [1, 2, 15, 16, 17, 31, 33, 100, 159, 160, 161, 196, 197, 208, 223, 224]
SWEEP_N = [1, 2, 3, 4, 5, 15, 16, 17, 197, 300, 2049]
SHAPES = sorted({(n, m) for m in SWEEP_M for n in (m, 197)} | {(n, m) for m in (17, 197, 224) for n in SWEEP_N})


@torch.no_grad()
@pytest.mark.parametrize("n,m", SHAPES, ids=[f"n{n}-m{m}" for n, m in SHAPES])
@pytest.mark.parametrize("dt,rpe", KERNELS)
def test_token_attention_kernel_shapes(dt, rpe, n, m):
    """Every key count of the last 16-key tile, query counts around the 4-row wave and 16-row workgroup tiles, 1 and 3 clouds, the
    row strides the wrapper passes (self layout when n == m) and dense operands."""
    for B, layout in ((1, "dense"), (3, "self" if n == m else "split")):
        q, qp, k, v, E = operands(dt, B, n, m, rpe, seed=1000 * n + m + B)
        out = attend(pack(layout, q, qp, k, v), vt_of(v), E, B, n, m, dt)
        ref, bound = reference(q, k, v, qp, E, dt=dt)
        check(out, ref, bound, f"B={B} {layout}")


# ------------------------------------------------------------------------------------------ adversarial values
ADV_M = [1, 17, 100, 197, 224]


@torch.no_grad()
@pytest.mark.parametrize("m", ADV_M)
@pytest.mark.parametrize("dt,rpe", KERNELS)
def test_one_dominant_key(dt, rpe, m):
    """q > 0 and one key k_j* = 4 (score ~ +29 over the others' ~0): the output is that key's v row, for j* the first and the last key."""
    B, n = 2, 21
    for js in sorted({0, m - 1}):
        q, qp, k, v, E = operands(dt, B, n, m, rpe, seed=m + 7 * js, ks=0.05, ps=0.05)
        q = (q.float().abs() * 0.5 + 0.5).to(dt)
        k[:, js] = 4.0
        out = attend(pack("split", q, qp, k, v), vt_of(v), E, B, n, m, dt)
        ref, bound = reference(q, k, v, qp, E, dt=dt)
        want = v[:, js].double().unsqueeze(1).expand(B, n, 256)
        assert ((ref - want).abs() <= 1e-4 * bound).all()  # (the other keys' weight: e^-29 each)
        check(out, want, bound, f"j*={js}", mean=False)


@torch.no_grad()
@pytest.mark.parametrize("m", ADV_M)
@pytest.mark.parametrize("dt,rpe", KERNELS)
def test_uniform_scores_average_exactly_m_keys(dt, rpe, m):
    """q = qp = 0: every score is 0 and the output is the mean of v over exactly m keys (v has a nonzero mean, so one key too many or
    too few moves every output by ~1/m)."""
    B, n = 3, 9
    q, qp, k, v, E = operands(dt, B, n, m, rpe, seed=300 + m, vs=0.25)
    q.zero_()
    if rpe:
        qp.zero_()
    v = (v.float() + 1.0).to(dt)
    out = attend(pack("split", q, qp, k, v), vt_of(v), E, B, n, m, dt)
    want = v.double().mean(1, keepdim=True).expand(B, n, 256)
    ref, bound = reference(q, k, v, qp, E, dt=dt)
    assert (ref - want).abs().max().item() < 1e-12
    check(out, want, bound, "uniform", mean=False)  # (every weight is the same bf16(1/m): its rounding error does not average out)


@torch.no_grad()
@pytest.mark.parametrize("m", ADV_M)
@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
def test_rpe_dominated_scores(dt, m):
    """qp . E >> q . k (scaled scores ~ N(0, 6^2) from the embedding term, ~0.01 from q k)."""
    B, n = 2, 37
    q, qp, k, v, E = operands(dt, B, n, m, True, seed=500 + m, qs=0.01, ps=3.0)
    out = attend(pack("split", q, qp, k, v), vt_of(v), E, B, n, m, dt)
    ref, bound = reference(q, k, v, qp, E, dt=dt)
    check(out, ref, bound, "rpe-dominated")


def _in_pool(t, tail, fill):
    """t copied to the front of a larger allocation whose `tail` elements after it hold `fill` (a tensor or a scalar)."""
    pool = torch.empty(t.numel() + tail, dtype=t.dtype, device=t.device)
    pool[t.numel():] = fill
    view = pool[: t.numel()].view(t.shape)
    view.copy_(t)
    return view


@torch.no_grad()
@pytest.mark.parametrize("m", ADV_M + [33])
@pytest.mark.parametrize("dt,rpe", KERNELS)
def test_poisoned_overread_is_masked(dt, rpe, m):
    """The last key tile reads up to 15 keys past m: the next query row's first keys (E), or past the end of the operands.  The next
    row's first keys are made large and aligned with the previous row's qp (a softmax that counted them would be dominated by them: the
    bound catches it); the allocations' tails after E, k | v and q | qp hold NaN or values aligned with the last row's qp: the output must
    equal, bit for bit, the run with a benign tail."""
    B, n = 3, 7
    q, qp, k, v, E = operands(dt, B, n, m, rpe, seed=700 + m)
    if rpe:
        Er = E.float().reshape(B * n, m, 256)
        al = torch.sign(qp.float().reshape(B * n, 4, 256).sum(1))  # direction of the previous row's qp, all heads
        Er[1:, : min(16, m)] = 10.0 * al[:-1].unsqueeze(1)
        E = Er.reshape(B, n, m, 256).to(dt)
    o = pack("split", q, qp, k, v)
    vt = vt_of(v)
    ref, bound = reference(q, k, v, qp, E, dt=dt)
    tail = 64 * 256
    huge = None
    if rpe:
        huge = (1e4 * torch.sign(qp[-1, -1].float().reshape(4, 256).sum(0))).to(dt).repeat(64)
    outs = []
    for fill in ("benign", "nan", "huge"):
        if fill == "huge" and not rpe:
            continue
        f = {"benign": 0.5, "nan": float("nan"), "huge": huge}[fill]
        oq = _in_pool(o["q"], tail, f)
        ok = _in_pool(o["k"], tail, f)
        ov = dict(q=oq, ldq=o["ldq"], qp=oq[..., 256:] if rpe else None, ldqp=o["ldqp"], k=ok, ldk=o["ldk"])
        Ep = _in_pool(E, tail, f) if rpe else None
        outs.append((fill, attend(ov, vt, Ep, B, n, m, dt)))
    check(outs[0][1], ref, bound, "benign tail")
    for fill, out in outs[1:]:
        assert torch.equal(out, outs[0][1]), f"{fill} tail changed the output"


# ------------------------------------------------------------------------------------------ batch and route invariance at scale
@torch.no_grad()
@pytest.mark.parametrize("n,m", [(197, 197), (197, 17), (197, 224)])
def test_rpe_routes_and_batch_invariance_near_4gib(n, m):
    """bf16 RPE: the smallest cloud count whose embedding reaches 2^32 bytes runs the fragment-load kernel (token_attn_kernel<true>,
    n = m = 197: B = 217, E = 4 311 835 136 B), one cloud fewer the LDS-DMA kernel with its 32-bit offsets just below the limit
    (B = 216, 4 291 964 928 B).  Clouds 0, B / 2 and B - 1 must equal the same cloud run alone (B = 1: the DMA kernel) bit for bit --
    both kernels issue the same MFMAs in the same order -- and stay inside the float64 bound."""
    per = n * m * 512
    B_frag = -(-(1 << 32) // per)
    for B, route in ((B_frag, "fragment"), (B_frag - 1, "dma")):
        assert (B * per >= 1 << 32) == (route == "fragment")
        g = torch.Generator(device="cuda").manual_seed(B)
        E = torch.randn(B, n, m, 256, generator=g, device="cuda", dtype=BF)
        y = torch.cat([torch.randn(B, n, 256, generator=g, device="cuda", dtype=BF),
                       0.25 * torch.randn(B, n, 1024, generator=g, device="cuda", dtype=BF)], -1)
        kv = torch.randn(B, m, 512, generator=g, device="cuda", dtype=BF)
        vt = vt_of(kv[..., 256:])
        full = attend(dict(q=y, ldq=1280, qp=y[..., 256:], ldqp=1280, k=kv, ldk=512), vt, E, B, n, m, BF)
        for b in (0, B // 2, B - 1):
            s = slice(b, b + 1)
            alone = attend(dict(q=y[s], ldq=1280, qp=y[s, :, 256:], ldqp=1280, k=kv[s], ldk=512), vt[s], E[s], 1, n, m, BF)
            assert torch.equal(full[s], alone), f"{route} B={B}: cloud {b} differs from the same cloud alone"
            ref, bound = reference(y[s, :, :256], kv[s, :, :256], kv[s, :, 256:], y[s, :, 256:], E[s], dt=BF)
            check(full[s], ref, bound, f"{route} B={B} cloud {b}")
        del E, y, kv, vt, full
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------ V^T producers
def _kv_vt(B, tokens, key_pad, N, seed):
    """unopose_linear_bf16_kv_vt vs unopose_linear_bf16 on the same operands, vt and C prefilled with NaN."""
    M, K = B * tokens, 256
    g = torch.Generator(device="cuda").manual_seed(seed)
    A = torch.randn(M, K, generator=g, device="cuda").to(BF)
    W = (0.06 * torch.randn(N, K, generator=g, device="cuda")).to(BF)
    bias = torch.randn(N, generator=g, device="cuda")
    C = torch.full((M, N), float("nan"), dtype=BF, device="cuda")
    vt = torch.full((B, 256, key_pad), float("nan"), dtype=BF, device="cuda")
    s = _lib().stream_ptr()
    _call("unopose_linear_bf16_kv_vt", vp(A), vp(W), vp(bias), vp(C), vp(vt), M, N, K, tokens, key_pad, s)
    want = torch.empty(M, N, dtype=BF, device="cuda")
    _call("unopose_linear_bf16", vp(A), vp(W), vp(bias), vp(want), M, N, K, 0, s)
    assert torch.equal(C[:, : N - 256], want[:, : N - 256]), "k columns differ from linear_bf16"
    assert torch.equal(vt[:, :, :tokens], want[:, N - 256:].reshape(B, tokens, 256).transpose(1, 2)), "V^T body is not the transpose of V"
    assert (vt[:, :, tokens:] == 0).all(), "V^T pad keys are not exactly zero"


@torch.no_grad()
@pytest.mark.parametrize("B", [1, 2, 3, 7, 64])
@pytest.mark.parametrize("m", [160, 161, 196, 197, 208, 223, 224])
def test_kv_vt_epilogue(m, B):
    """csrc/gemm_small.hip EPI 4 at every key count the wrapper sends it (224 - m <= 64): clouds ending anywhere in a 64-row block."""
    _kv_vt(B, m, KP, 512, seed=m * 100 + B)
    if B in (1, 3):
        _kv_vt(B, m, KP, 1792, seed=m * 100 + B + 1)  # the self layer's q | qp | k | v projection


@torch.no_grad()
@pytest.mark.parametrize("tokens,extra", list(itertools.product([1, 7, 33], [0, 1, 64])))
def test_kv_vt_epilogue_small_clouds(tokens, extra):
    """ABI-legal small clouds: several clouds end inside one 64-row block (and key_pad = tokens: no pad at all)."""
    _kv_vt(300 // tokens + 1, tokens, tokens + extra, 512, seed=tokens * 10 + extra)


@torch.no_grad()
def test_kv_vt_abi_rejects_bad_shapes():
    A = torch.zeros(14, 256, dtype=BF, device="cuda")
    W = torch.zeros(512, 256, dtype=BF, device="cuda")
    bias = torch.zeros(512, device="cuda")
    C = torch.zeros(14, 512, dtype=BF, device="cuda")
    vt = torch.zeros(2, 256, 80, dtype=BF, device="cuda")
    s = _lib().stream_ptr()
    with pytest.raises(RuntimeError, match="key_pad"):
        _call("unopose_linear_bf16_kv_vt", vp(A), vp(W), vp(bias), vp(C), vp(vt), 14, 512, 256, 7, 7 + 65, s)
    with pytest.raises(RuntimeError, match="whole clouds"):
        _call("unopose_linear_bf16_kv_vt", vp(A), vp(W), vp(bias), vp(C), vp(vt), 14, 512, 256, 5, 40, s)


@torch.no_grad()
@pytest.mark.parametrize("m", [1, 17, 100, 159, 224])
@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
def test_transpose_pad(dt, m):
    """csrc/glue.hip transpose_pad from the k | v projection (v read in place, row stride 512) into a NaN-prefilled V^T."""
    s = _lib().stream_ptr()
    for B in (1, 3):
        y = torch.randn(B, m, 512, device="cuda").to(dt)
        vt = torch.full((B, 256, KP), float("nan"), dtype=dt, device="cuda")
        name = "unopose_transpose_pad_bf16" if dt == BF else "unopose_transpose_pad_f32"
        _call(name, ctypes.c_void_p(y.data_ptr() + 256 * y.element_size()), y.stride(1), B, m, 256, KP, vp(vt), s)
        assert torch.equal(vt[:, :, :m], y[..., 256:].transpose(1, 2)), "V^T body is not the transpose of V"
        assert (vt[:, :, m:] == 0).all(), "V^T pad keys are not exactly zero"


# ------------------------------------------------------------------------------------------ op level
def _mha(rpe, seed):
    from unopose_amd.model.modules import _MHA

    torch.manual_seed(seed)
    att = _MHA(256, rpe).cuda().eval()
    with torch.no_grad():
        for p in att.parameters():
            p.normal_(0, 0.1)
        if rpe:
            att.proj_p.weight.mul_(0.5)  # (qp . E then ~ as large as q . k)
    return att


def _poison_allocator(B, dt):
    """Hand the caching allocator a few freed blocks of V^T's size full of NaN: a pad column left unwritten then shows up."""
    blocks = [torch.full((B, 256, KP), float("nan"), dtype=dt, device="cuda") for _ in range(4)]
    del blocks


def rounded(y, eps):
    """bf16(y) and its uncertainty when the path computes y to within eps before rounding: 0 unless y - eps or y + eps rounds to
    another bf16 value (then the farther of those)."""
    yr = y.to(BF).double()
    return yr, torch.maximum(((y - eps).to(BF).double() - yr).abs(), ((y + eps).to(BF).double() - yr).abs())


def op_reference(x, mem, att, embed, prec, composite):
    """float64 reference from the module's weights (proj_q / k / v / p), with the path's rounding points modelled.
    bf16 (autocast): x, E, the weights and biases enter as bf16 values (taken exactly); each projection is one fp32-accumulated GEMM
    rounded to bf16: the reference rounds the float64 value, and where the fp32 sum (16 k-steps of 16 products: within 2^-18 of
    |x| |W| + |b|) may fall on the other side of a rounding boundary, the neighbour is allowed (`rounded`; the library GEMMs of the
    composite may round once more before the bias: 2^-9 |y|).  The RPE query qp_h = q_h W_p,h is,
    on the kernel path, one GEMM with the folded weight W_p,h^T W_q,h (the fold is fp32 arithmetic of the path, rounded to bf16: taken
    as the path forms it); the composite computes bf16(q W_p).
    fp32: exact operands; each projection within 2^-15 of its absolute sum (the hi / lo split GEMMs: ~3 x 2^-18 per product), the
    folded RPE weight formed in fp32.
    The composite fall-back (m > 224) rounds its scores as well (three roundings to its dtype).  The proj_p bias adds q_h . b_p to every
    key of a row: a constant the softmax removes."""
    B, n, _ = x.shape
    bf = prec == "bf16"
    r = (lambda t: t.detach().to(BF).double()) if bf else (lambda t: t.detach().double())  # noqa: E731
    xd, md = r(x), r(mem)

    def proj(a, lin):
        w, b = r(lin.weight), r(lin.bias)
        y, ya = a @ w.T + b, a.abs() @ w.abs().T + b.abs()
        return rounded(y, 2.0 ** -18 * ya) if bf else (y, 2.0 ** -15 * ya)

    q, dq = proj(xd, att.proj_q)
    k, dk = proj(md, att.proj_k)
    v, dv = proj(md, att.proj_v)
    qp = dqp = E = None
    if embed is not None:
        if bf and not composite:
            wq, bq = att.proj_q.weight.detach().float(), att.proj_q.bias.detach().float()
            wp32 = att.proj_p.weight.detach().float().reshape(4, 64, 256)
            wf = torch.einsum("hcd,hci->hdi", wp32, wq.reshape(4, 64, 256)).reshape(1024, 256).to(BF).double()
            bfold = torch.einsum("hcd,hc->hd", wp32, bq.reshape(4, 64)).reshape(1024).to(BF).double()
            qp, dqp = rounded(xd @ wf.T + bfold, 2.0 ** -18 * (xd.abs() @ wf.abs().T + bfold.abs()))
        elif not composite:  # fp32 kernel path: one GEMM with the fold (fp32 sums of 64 products: 2^-18 of the chained absolute sums)
            wq, bq = att.proj_q.weight.double().reshape(4, 64, 256), att.proj_q.bias.double().reshape(4, 64)
            wp = att.proj_p.weight.double().reshape(4, 64, 256)
            wf = torch.einsum("hcd,hci->hdi", wp, wq).reshape(1024, 256)
            bfold = torch.einsum("hcd,hc->hd", wp, bq).reshape(1024)
            qp = xd @ wf.T + bfold
            chained = torch.einsum("bnhc,hcd->bnhd", (xd.abs() @ wq.abs().reshape(256, 256).T + bq.abs().reshape(256)).reshape(B, n, 4, 64),
                                   wp.abs()).reshape(B, n, 1024)
            dqp = 2.0 ** -15 * (xd.abs() @ wf.abs().T + bfold.abs()) + 2.0 ** -18 * chained
        else:
            wp = r(att.proj_p.weight).reshape(4, 64, 256)
            q4, dq4 = q.reshape(B, n, 4, 64), dq.reshape(B, n, 4, 64)
            qp = torch.einsum("bnhc,hcd->bnhd", q4, wp).reshape(B, n, 1024)
            qa = torch.einsum("bnhc,hcd->bnhd", q4.abs(), wp.abs()).reshape(B, n, 1024)
            carried = torch.einsum("bnhc,hcd->bnhd", dq4, wp.abs()).reshape(B, n, 1024)
            if bf:
                qp, dqp = rounded(qp, 2.0 ** -18 * qa + carried)
                dqp = dqp + carried
            else:
                dqp = 2.0 ** -15 * qa + carried
        E = r(embed)
    rs = (3 * 2.0 ** -9 if bf else 2.0 ** -15) if composite else 0.0
    return reference(q, k, v, qp, E, dt=BF if bf else F32, dq=dq, dk=dk, dv=dv, dqp=dqp, rs=rs)


OP_M = [17, 159, 160, 224, 225]


@torch.no_grad()
@pytest.mark.parametrize("m", OP_M)
@pytest.mark.parametrize("kind", ["self-rpe", "self", "cross"])
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_op_token_attention(prec, kind, m, monkeypatch):
    """ops.token_attention under autocast(bf16) and in fp32: RPE self-attention, self-attention without embedding, cross-attention of
    2049 queries over m keys.  m = 225 exceeds the kernels' key tile: the torch composite runs, with its RuntimeWarning."""
    from unopose_amd import ops
    from unopose_amd.ops import common

    B = 2
    att = _mha(kind == "self-rpe", seed=m)
    g = torch.Generator(device="cuda").manual_seed(m + 1)
    n = m if kind.startswith("self") else 2049
    x = torch.randn(B, n, 256, generator=g, device="cuda")
    mem = x if kind.startswith("self") else torch.randn(B, m, 256, generator=g, device="cuda")
    E = torch.randn(B, n, m, 256, generator=g, device="cuda") if kind == "self-rpe" else None
    dt = BF if prec == "bf16" else F32
    monkeypatch.setattr(common, "_fallbacks_seen", set())
    _poison_allocator(B, dt)
    with torch.autocast("cuda", dtype=BF, enabled=prec == "bf16"):
        if m > KP:
            with pytest.warns(RuntimeWarning, match="token_attention"):
                out = ops.token_attention(x, mem, att, 4, E)
        else:
            out = ops.token_attention(x, mem, att, 4, E)
    assert out.dtype == dt and out.shape == (B, n, 256)
    ref, bound = op_reference(x, mem, att, E, prec, composite=m > KP)
    check(out, ref, bound, f"{prec} {kind} m={m}")


@torch.no_grad()
@pytest.mark.parametrize("m", [160, 197, 224])
def test_kv_vt_route_equals_transpose_route(m):
    """USE_KV_VT on / off (V^T from the projection's epilogue or from the transpose launch) give the same bits, self and cross, on a
    NaN-poisoned allocator (extends the m = 197 check of test_model_gpu.py::test_token_attention_kernel_bf16)."""
    from unopose_amd import ops

    B = 3
    att0, att1 = _mha(True, seed=11), _mha(False, seed=12)
    g = torch.Generator(device="cuda").manual_seed(m)
    x = torch.randn(B, m, 256, generator=g, device="cuda")
    y = torch.randn(B, m, 256, generator=g, device="cuda")
    E = torch.randn(B, m, m, 256, generator=g, device="cuda")
    got = {}
    for fused in (True, False):
        ops.USE_KV_VT = fused
        try:
            with torch.autocast("cuda", dtype=BF):
                _poison_allocator(B, BF)
                a = ops.token_attention(x, x, att0, 4, E)
                _poison_allocator(B, BF)
                b = ops.token_attention(x, y, att1, 4, None)
            got[fused] = (a, b)
        finally:
            ops.USE_KV_VT = True
    assert torch.equal(got[True][0], got[False][0]) and torch.equal(got[True][1], got[False][1])
    assert not got[True][0].isnan().any() and not got[True][1].isnan().any()
