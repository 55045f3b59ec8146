"""Attention cores: timm ViT attention (csrc/vit_attn*.hip), the correspondence transformer's RPE / cross token attention (csrc/attn*.hip) and the
focused linear attention (csrc/linattn.hip), each with its op-by-op torch composite (training path, fall-back)."""
import ctypes

import torch
import torch.nn.functional as F

from .._lib import call, lib, on_device, ptr, stream_ptr
from . import _state as st
from .common import _c, _own_f32, _own_glue, _params_key, note_fallback
from .dense import _lin, bf16_linear_2d, bmm_nt_f32, linear, linear_f32_raw


def vit_attention(qkv, heads):
    """timm Attention core: qkv (B,T,3C) -> (B,T,C).  bf16 (autocast) inputs run the flash-style HIP
    kernel (csrc/vit_attn.hip, head dim 64); fp32 inputs the op-by-op composite."""
    if st._DIFF:
        return vit_attention_torch(qkv, heads)
    if qkv.dtype == torch.bfloat16 and qkv.shape[-1] == 3 * heads * 64:
        B, T, C3 = qkv.shape
        qkv = _c(qkv)
        out = torch.empty(B, T, C3 // 3, dtype=torch.bfloat16, device=qkv.device)
        with on_device(qkv.device):
            call("unopose_vit_attention", ptr(qkv), B, T, heads, ptr(out), stream_ptr())
        return out
    if qkv.dtype == torch.float32 and qkv.is_cuda and qkv.shape[-1] == 3 * heads * 64:
        B, T, C3 = qkv.shape
        qkv = _c(qkv)
        out = torch.empty(B, T, C3 // 3, dtype=torch.float32, device=qkv.device)
        with on_device(qkv.device):
            call("unopose_vit_attention_f32", ptr(qkv), B, T, heads, ptr(out), stream_ptr())
        return out
    note_fallback("vit_attention", f"head dim {qkv.shape[-1] // (3 * heads)} / dtype {qkv.dtype} (kernels: head dim 64, bf16 or fp32)")
    return vit_attention_torch(qkv, heads)


def vit_attention_f32_split(qkv, heads):
    """fp32 qkv (B,T,3C) -> the attention output in the split layout of csrc/gemm_f32.hip, a (B*T, 2C) bf16 tensor: the operand of
    the projection GEMM, written by the attention kernel itself (no fp32 round trip, no split pass)."""
    B, T, C3 = qkv.shape
    assert qkv.dtype == torch.float32 and qkv.is_cuda and C3 == 3 * heads * 64
    qkv = _c(qkv)
    out = torch.empty(B * T, 2 * (C3 // 3), dtype=torch.bfloat16, device=qkv.device)
    with on_device(qkv.device):
        call("unopose_vit_attention_f32_split", ptr(qkv), B, T, heads, ptr(out), stream_ptr())
    return out


def vit_attention_f32_ss(qkv_split, B, T, heads):
    """qkv in the split layout ((B*T, 2 * 3C) bf16, as `linear_f32x3(..., out="split")` writes it) -> the attention output in the
    split layout ((B*T, 2C) bf16): csrc/vit_attn_f32s.hip, the fp32 ViT block's attention core (no fp32 tensor in between)."""
    C3 = qkv_split.shape[-1] // 2
    assert qkv_split.dtype == torch.bfloat16 and qkv_split.is_cuda and qkv_split.is_contiguous() and C3 == 3 * heads * 64
    out = torch.empty(B * T, 2 * (C3 // 3), dtype=torch.bfloat16, device=qkv_split.device)
    with on_device(qkv_split.device):
        call("unopose_vit_attention_f32_ss", ptr(qkv_split), B, T, heads, ptr(out), stream_ptr())
    return out


def vit_attention_torch(qkv, heads):
    """Op-by-op composite of the same function."""
    B, T, C3 = qkv.shape
    C = C3 // 3
    hd = C // heads
    q, k, v = qkv.reshape(B, T, 3, heads, hd).permute(2, 0, 3, 1, 4)
    # (softmax in fp32 for 16-bit inputs; float64 inputs stay float64 throughout -- tests/test_vit_attn_ref_cpu.py compares at 1e-12)
    sm = torch.float64 if qkv.dtype == torch.float64 else torch.float32
    a = torch.softmax((q * hd ** -0.5) @ k.transpose(-2, -1), dim=-1, dtype=sm).to(v.dtype) @ v
    return a.transpose(1, 2).reshape(B, T, C)


_KEY_PAD = None


def _key_pad():
    """The kernels' padded key count KP (unopose_token_attention_key_pad())."""
    global _KEY_PAD
    if _KEY_PAD is None:
        _KEY_PAD = lib().unopose_token_attention_key_pad()
    return _KEY_PAD


def token_attention(x, mem, att, heads, embed=None):
    """MultiHeadAttention / RPEMultiHeadAttention core (transformer.py:130-148, 386-405): returns the
    concatenated heads (B,n,C) before the output Linear.  The RPE term q.proj_p(E) is folded:
    q.(W_p e + b_p) = (q W_p).e + q.b_p  (SURVEY.md App-F), so no (B,4,n,m,64) tensor exists.
    Under autocast(bf16) the whole core (q k^T, folded RPE term, softmax, P v) is ONE HIP kernel on the
    bf16 matrix cores (csrc/attn.hip) that streams E once; in fp32 the same scheme with hi/lo-split operands
    (csrc/attn_f32.hip).  Under autograd (differentiable mode, fp32) the core is `_TokenAttnFn` on the projections'
    outputs; shapes outside the kernels take the op-by-op composite below."""
    if st._DIFF and torch.is_grad_enabled() and token_attention_train_ok(x, mem, att, heads, embed):
        return _token_attention_train(x, mem, att, embed)
    if not st._DIFF and x.is_cuda and heads == 4 and x.shape[-1] == 256:
        if mem.shape[1] <= _key_pad():
            if torch.is_autocast_enabled():
                return _token_attention_hip(x, mem, att, embed)
            if x.dtype == torch.float32:
                return _token_attention_hip_f32(x, mem, att, embed)
    if not st._DIFF and x.is_cuda:
        note_fallback("token_attention", f"heads {heads} x width {x.shape[-1]}, {mem.shape[1]} keys, dtype {x.dtype} (kernels: 4 x 64, up to the padded key count)")
    return token_attention_torch(x, mem, att, heads, embed)


def _token_attention_hip_f32(x, mem, att, embed):
    """fp32 path: same kernel scheme with hi/lo-split bf16 MFMAs (csrc/attn_f32.hip); projections in
    fp32 with the RPE fold baked into the weights (exact algebra, fp32 rounding)."""

    B, n, C = x.shape
    kp = _key_pad()
    m = mem.shape[1]
    rpe = embed is not None
    key = _params_key(att, rpe, "f32")
    cache = getattr(att, "_hip_cache_f32", None)
    if cache is None or cache[0] != key:
        with torch.no_grad():
            wq, bq = att.proj_q.weight.float(), att.proj_q.bias.float()
            pw, pb = [wq], [bq]
            if rpe:
                wp = att.proj_p.weight.float().reshape(4, 64, 256)
                pw.append(torch.einsum("hcd,hci->hdi", wp, wq.reshape(4, 64, 256)).reshape(1024, 256))
                pb.append(torch.einsum("hcd,hc->hd", wp, bq.reshape(4, 64)).reshape(1024))
            cache = (key, torch.cat(pw, 0).contiguous(), torch.cat(pb, 0).contiguous(),
                     torch.cat([att.proj_k.weight.float(), att.proj_v.weight.float()], 0).contiguous(),
                     torch.cat([att.proj_k.bias.float(), att.proj_v.bias.float()], 0).contiguous())
        att._hip_cache_f32 = cache
    _, w_q, b_q, w_kv, b_kv = cache
    yq = linear_f32_raw(x, w_q, b_q, att, "q")
    ykv = linear_f32_raw(mem, w_kv, b_kv, att, "kv")
    if ykv.is_contiguous() and C % 32 == 0 and m <= kp:  # V^T, zero-padded to the kernel's key count: one launch (csrc/glue.hip)
        vt = torch.empty(B, C, kp, dtype=torch.float32, device=x.device)
        with on_device(x.device):
            call("unopose_transpose_pad_f32", ctypes.c_void_p(ykv.data_ptr() + C * 4), ykv.stride(1), B, m, C, kp, ptr(vt), stream_ptr())
    else:
        vt = torch.zeros(B, C, kp, dtype=torch.float32, device=x.device)
        vt[:, :, :m] = ykv[..., C:].transpose(1, 2)
    E = _c(embed.float()) if rpe else None
    out = torch.empty(B, n, C, dtype=torch.float32, device=x.device)
    qptr, kptr = yq.data_ptr(), ykv.data_ptr()
    with on_device(x.device):
        call("unopose_token_attention_f32", ctypes.c_void_p(qptr), yq.stride(1), ctypes.c_void_p(kptr), ykv.stride(1),
             ptr(vt), ctypes.c_void_p(qptr + C * 4) if rpe else None, yq.stride(1), ptr(E) if rpe else None, B, n, m,
             0.125, ptr(out), stream_ptr())
    return out


def _attn_weights(att, rpe):
    """bf16 projection weights of one attention module, concatenated so that q | k | v (| the folded
    RPE query q W_p, 4 x 256) come out of as few GEMMs as possible.  Folding in fp32:
    (x Wq_h^T + bq_h) Wp_h = x (Wp_h^T Wq_h)^T + bq_h Wp_h."""
    key = _params_key(att, rpe)
    cache = getattr(att, "_hip_cache", None)
    if cache is not None and cache[0] == key:
        return cache[1]
    with torch.no_grad(), torch.autocast("cuda", enabled=False):  # (the caller runs under autocast: its einsum would fold in bf16)
        bf = torch.bfloat16
        wq, bq = att.proj_q.weight.float(), att.proj_q.bias.float()
        parts_w, parts_b = [wq], [bq]
        if rpe:
            wp = att.proj_p.weight.float().reshape(4, 64, 256)  # [h][c][d]
            wqh = wq.reshape(4, 64, 256)                         # [h][c][in]
            parts_w.append(torch.einsum("hcd,hci->hdi", wp, wqh).reshape(1024, 256))
            parts_b.append(torch.einsum("hcd,hc->hd", wp, bq.reshape(4, 64)).reshape(1024))
        w_q = torch.cat(parts_w, 0).to(bf).contiguous()
        b_q = torch.cat(parts_b, 0).to(bf).contiguous()
        w_kv = torch.cat([att.proj_k.weight.float(), att.proj_v.weight.float()], 0).to(bf).contiguous()
        b_kv = torch.cat([att.proj_k.bias.float(), att.proj_v.bias.float()], 0).to(bf).contiguous()
        w_all = torch.cat([w_q, w_kv], 0).contiguous()
        b_all = torch.cat([b_q, b_kv], 0).contiguous()
    val = (w_q, b_q, w_kv, b_kv, w_all, b_all, b_q.float(), b_kv.float(), b_all.float())
    att._hip_cache = (key, val)
    return val


def _token_attention_hip(x, mem, att, embed):
    B, n, C = x.shape
    kp = _key_pad()
    m = mem.shape[1]
    bf = torch.bfloat16
    rpe = embed is not None
    w_q, b_q, w_kv, b_kv, w_all, b_all, bq32, bkv32, ball32 = _attn_weights(att, rpe)
    nq = w_q.shape[0]
    xb = x.to(bf)
    vt = torch.empty(B, C, kp, dtype=bf, device=x.device)

    def project_kv(a2, w, b32, rows):
        """a2 @ w^T + b with the V columns (the last 256) written straight into `vt` (csrc/gemm_small.hip EPI 4): no transpose launch"""
        y = torch.empty(rows, w.shape[0], dtype=bf, device=x.device)
        with on_device(x.device):
            call("unopose_linear_bf16_kv_vt", ptr(a2), ptr(w), ptr(b32), ptr(y), ptr(vt), rows, w.shape[0], C, m, kp, stream_ptr())
        return y

    fused_vt = st.USE_KV_VT and C == 256 and kp - m <= 64 and st.USE_HIP_GEMM and st.HIP_GEMM_ALL
    with torch.autocast("cuda", enabled=False):
        if mem is x:  # self-attention: one GEMM for q | qp | k | v
            if fused_vt:
                y = project_kv(_c(xb).reshape(B * n, C), w_all, ball32, B * n).reshape(B, n, -1)
            else:
                y = bf16_linear_2d(xb.reshape(B * n, C), w_all, ball32, b_all).reshape(B, n, -1)
            yq, ykv = y[..., :nq], y[..., nq:]
        else:
            yq = bf16_linear_2d(xb.reshape(B * n, C), w_q, bq32, b_q).reshape(B, n, -1)
            if fused_vt:
                ykv = project_kv(_c(mem.to(bf)).reshape(B * m, C), w_kv, bkv32, B * m).reshape(B, m, -1)
            else:
                ykv = bf16_linear_2d(mem.to(bf).reshape(B * m, C), w_kv, bkv32, b_kv).reshape(B, m, -1)
    # q | qp and k | v are consumed in place from the projection outputs (row strides passed to the kernel)
    if not fused_vt:
        with on_device(x.device):
            call("unopose_transpose_pad_bf16", ctypes.c_void_p(ykv.data_ptr() + C * 2), ykv.stride(1), B, m, C, kp, ptr(vt), stream_ptr())
    E = _c(embed.to(bf)) if rpe else None
    out = torch.empty(B, n, C, dtype=bf, device=x.device)
    esz = 2
    q_ptr = yq.data_ptr()
    k_ptr = ykv.data_ptr()
    with on_device(x.device):
        call("unopose_token_attention", ctypes.c_void_p(q_ptr), yq.stride(1), ctypes.c_void_p(k_ptr), ykv.stride(1),
             ptr(vt), ctypes.c_void_p(q_ptr + C * esz) if rpe else None, yq.stride(1),
             ptr(E) if E is not None else None, B, n, m, 0.125, ptr(out), stream_ptr())
    return out


def _transpose_pad_f32(t):
    """(B,m,256) fp32 rows -> (B,256,KP) channel-major, zero-padded to the kernels' key count (csrc/glue.hip)."""
    B, m, C = t.shape
    out = torch.empty(B, C, _key_pad(), dtype=torch.float32, device=t.device)
    with on_device(t.device):
        call("unopose_transpose_pad_f32", ptr(t), t.stride(1), B, m, C, _key_pad(), ptr(out), stream_ptr())
    return out


class _TokenAttnFn(torch.autograd.Function):
    """The attention core of `token_attention_torch` under autograd, from the projections' outputs: q (B,n,256), k / v (B,m,256),
    RPE: qp (B,n,4,256) = q_h W_p,h (the folded proj_p) and E (B,n,m,256), else None.  Forward = the fp32 eval kernel, which also
    stores the softmax weights P (B,4,n,KP); backward = csrc/attn_f32.hip's three kernels (dq and dS; dk, dv; dqp and dE with E
    streamed once).  `bp` (proj_p.bias or None) only receives its gradient: q.b_p is constant along every softmax row, so it
    changes nothing and its gradient is zero (every trainable parameter still gets one, as DDP expects)."""

    @staticmethod
    def forward(ctx, q, k, v, qp, E, bp):
        B, n, C = q.shape
        m = k.shape[1]
        q, k, v = _c(q), _c(k), _c(v)
        rpe = qp is not None
        if rpe:
            qp, E = _c(qp), _c(E)
        vt = _transpose_pad_f32(v)
        out = torch.empty(B, n, C, dtype=torch.float32, device=q.device)
        P = torch.empty(B, 4, n, _key_pad(), dtype=torch.float32, device=q.device)
        with on_device(q.device):
            call("unopose_token_attention_f32_train", ptr(q), C, ptr(k), C, ptr(vt), ptr(qp) if rpe else None, 4 * C,
                 ptr(E) if rpe else None, B, n, m, 0.125, ptr(out), ptr(P), stream_ptr())
        ctx.save_for_backward(q, k, v, qp, E, P)
        ctx.bp_like = None if bp is None else (bp.shape, bp.dtype, bp.device)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, qp, E, P = ctx.saved_tensors
        B, n, C = q.shape
        m = k.shape[1]
        rpe = qp is not None
        dout = _c(dout.float())
        kt = _transpose_pad_f32(k)
        dS = torch.empty_like(P)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        dqp = torch.empty_like(qp) if rpe else None
        dE = torch.empty_like(E) if rpe and ctx.needs_input_grad[4] else None
        with on_device(q.device):
            call("unopose_token_attention_f32_backward", ptr(dout), ptr(q), C, ptr(v), C, ptr(kt), ptr(qp) if rpe else None, 4 * C,
                 ptr(E) if rpe else None, ptr(P), B, n, m, 0.125, ptr(dS), ptr(dq), ptr(dk), ptr(dv), ptr(dqp) if rpe else None,
                 ptr(dE) if dE is not None else None, stream_ptr())
        dbp = None if ctx.bp_like is None else torch.zeros(ctx.bp_like[0], dtype=ctx.bp_like[1], device=ctx.bp_like[2])
        return dq, dk, dv, dqp, dE, dbp


def token_attention_train_ok(x, mem, att, heads, embed=None):
    """`_TokenAttnFn` applies: switch on, CUDA, fp32 outside autocast, 4 heads x 64, 1 <= m <= KP keys."""
    f32 = torch.float32
    return (st.TRAIN_OWN_ATTN and x.is_cuda and heads == 4 and x.shape[-1] == 256 and mem.shape[-1] == 256 and x.shape[1] >= 1
            and 1 <= mem.shape[1] <= _key_pad() and x.shape[0] <= 65535 and not torch.is_autocast_enabled()
            and x.dtype == f32 and mem.dtype == f32 and att.proj_q.weight.dtype == f32 and (embed is None or embed.dtype == f32))


def _token_attention_train(x, mem, att, embed):
    """The projections as in the composite (trainable linears, qp = q W_p a torch op: dW_p and its share of dq come from autograd), the
    core on `_TokenAttnFn`."""
    B, n, C = x.shape
    q, k, v = _lin(x, att.proj_q), _lin(mem, att.proj_k), _lin(mem, att.proj_v)
    if embed is None:
        return _TokenAttnFn.apply(q, k, v, None, None, None)
    qp = torch.einsum("bnhc,hcd->bnhd", q.reshape(B, n, 4, 64), att.proj_p.weight.reshape(4, 64, C))
    return _TokenAttnFn.apply(q, k, v, qp, embed, att.proj_p.bias)


def token_attention_torch(x, mem, att, heads, embed=None):
    """Op-by-op composite of the same function (fp32 path; A/B reference for the HIP kernel)."""
    B, n, C = x.shape
    hd = C // heads
    q = _lin(x, att.proj_q).reshape(B, n, heads, hd)
    k = _lin(mem, att.proj_k).reshape(B, -1, heads, hd)
    v = _lin(mem, att.proj_v).reshape(B, -1, heads, hd)
    s = torch.einsum("bnhc,bmhc->bhnm", q, k)
    if embed is not None:
        wp = att.proj_p.weight.reshape(heads, hd, C)  # rows of W_p grouped by head
        qp = torch.einsum("bnhc,hcd->bnhd", q, wp.to(q.dtype))  # (B,n,h,C)
        s = s + torch.einsum("bnhd,bnmd->bhnm", qp, embed.to(q.dtype))
        s = s + torch.einsum("bnhc,hc->bhn", q, att.proj_p.bias.reshape(heads, hd).to(q.dtype)).unsqueeze(-1)
    p = torch.softmax(s.float() / hd ** 0.5, dim=-1).to(v.dtype)
    return torch.einsum("bhnm,bmhc->bnhc", p, v).reshape(B, n, C)


def focused_linear_attention(xq, xkv, att, heads, focusing, kv_skip=0):
    """LinearAttention.forward (transformer.py:533-568).  With 4 heads x 64 the focusing + per-head
    contraction + z scaling run in ONE HIP kernel per side (csrc/linattn.hip): bf16 MFMAs under autocast,
    hi/lo-split (fp32-class) MFMAs on fp32 data; other shapes take the op-by-op composite.
    `kv_skip`: leading rows of every batch of xkv that are not keys / values (xkv[:, kv_skip:] is meant; the bf16 kernels read the
    window in place, the other paths slice).  Under autograd (differentiable mode, fp32) the core is `_LinearAttnFn` on the
    projections' outputs (csrc/linattn_train.hip: forward and backward kernels); shapes outside it take the op-by-op composite."""
    if st._DIFF and torch.is_grad_enabled() and linear_attention_train_ok(xq, xkv, att, heads, focusing):
        return _focused_linear_attention_train(xq, xkv, att, kv_skip)
    if not st._DIFF and heads == 4 and xq.shape[-1] == 256 and xq.is_cuda and float(focusing) == 3.0:
        if torch.is_autocast_enabled():
            if kv_skip and not (st.USE_LA_KV_STATE and xkv.is_contiguous()):
                xkv, kv_skip = xkv[:, kv_skip:], 0
            return _focused_linear_attention_hip(xq, xkv, att, int(focusing), kv_skip)
    if kv_skip:
        xkv = xkv[:, kv_skip:]
    if not st._DIFF and heads == 4 and xq.shape[-1] == 256 and xq.is_cuda and float(focusing) == 3.0:
        if xq.dtype == torch.float32 and xkv.dtype == torch.float32:
            return _focused_linear_attention_hip_f32(xq, xkv, att, int(focusing))
    if not st._DIFF and xq.is_cuda:
        note_fallback("focused_linear_attention", f"heads {heads} x width {xq.shape[-1]}, focusing {focusing} (kernels: 4 x 64, 3)")
    return focused_linear_attention_torch(xq, xkv, att, heads, focusing)


_LA_PARTIAL_FLOATS = None


def _la_workspace(B, N, J, device):
    """The partial-sum workspace of the linear attention's training kernels at this size (records of a fixed number of floats)."""
    global _LA_PARTIAL_FLOATS
    if _LA_PARTIAL_FLOATS is None:
        _LA_PARTIAL_FLOATS = lib().unopose_linear_attention_f32_partial_floats()
    n = lib().unopose_linear_attention_f32_partials(B, N, J)
    if n < 0:
        raise RuntimeError(f"unopose_linear_attention_f32_partials: B={B} N={N} J={J} outside the contract")
    return torch.empty(max(n, 1), _LA_PARTIAL_FLOATS, dtype=torch.float32, device=device), n


class _LinearAttnFn(torch.autograd.Function):
    """The core of `focused_linear_attention_torch` under autograd, from the projections' outputs: yq (B,N,256), yk / v (B,J,256) and
    s (256) = 1 / softplus(scale) (a torch op of the caller's: the gradient of `scale` itself comes from autograd).  Forward =
    csrc/linattn_train.hip's key state (K = k^T v per head, its transpose, S = sum_j k_j) and query pass, which keeps den (B,N,4);
    backward = one pass over the query rows (dyq, per-workgroup partials of dK, dS, ds), one over the key rows (dyk, dv) and the
    fixed-order sums of the partials.  The focused rows are recomputed, not stored: besides its inputs the function saves only
    K, K^T, S and den.  Without a gradient for yk, v and s the backward is the query pass alone."""

    @staticmethod
    def forward(ctx, yq, yk, v, s):
        B, N, C = yq.shape
        J = yk.shape[1]
        yq, yk, v, s = _c(yq), _c(yk), _c(v), _c(s)
        dev = yq.device
        out = torch.empty(B, N, C, dtype=torch.float32, device=dev)
        K = torch.empty(B, 4, 64, 64, dtype=torch.float32, device=dev)
        Kt = torch.empty_like(K)
        S = torch.empty(B, C, dtype=torch.float32, device=dev)
        den = torch.empty(B, N, 4, dtype=torch.float32, device=dev)
        ws, n = _la_workspace(B, N, J, dev)
        with on_device(dev):
            call("unopose_linear_attention_f32_train", ptr(yq), ptr(yk), ptr(v), ptr(s), B, N, J, 3, ptr(out), ptr(K), ptr(Kt), ptr(S),
                 ptr(den), ptr(ws), n, stream_ptr())
        ctx.save_for_backward(yq, yk, v, s, K, Kt, S, den)
        return out

    @staticmethod
    def backward(ctx, dout):
        yq, yk, v, s, K, Kt, S, den = ctx.saved_tensors
        B, N, C = yq.shape
        J = yk.shape[1]
        dev = yq.device
        dout = _c(dout.float())
        keys = any(ctx.needs_input_grad[1:])
        dyq = torch.empty_like(yq)
        dyk = dv = ds = ws = None
        n = 0
        if keys:
            dyk, dv, ds = torch.empty_like(yk), torch.empty_like(v), torch.empty_like(s)
            ws, n = _la_workspace(B, N, J, dev)
        with on_device(dev):
            call("unopose_linear_attention_f32_backward", ptr(dout), ptr(yq), ptr(yk), ptr(v), ptr(s), ptr(K), ptr(Kt), ptr(S), ptr(den),
                 B, N, J, 3, ptr(dyq), ptr(dyk) if keys else None, ptr(dv) if keys else None, ptr(ds) if keys else None,
                 ptr(ws) if keys else None, n, stream_ptr())
        need = ctx.needs_input_grad
        return dyq if need[0] else None, dyk if need[1] else None, dv if need[2] else None, ds if need[3] else None


def linear_attention_train_ok(xq, xkv, att, heads, focusing):
    """`_LinearAttnFn` applies: switch on, CUDA, fp32 outside autocast, 4 heads x 64, focusing factor 3, at least one query and key."""
    f32 = torch.float32
    return (st.TRAIN_OWN_LINATTN and xq.is_cuda and heads == 4 and xq.shape[-1] == 256 and xkv.shape[-1] == 256 and float(focusing) == 3.0
            and xq.shape[0] <= 65535 and xq.shape[1] >= 1 and xkv.shape[1] >= 1 and not torch.is_autocast_enabled()
            and xq.dtype == f32 and xkv.dtype == f32 and att.proj_q.weight.dtype == f32 and att.scale.dtype == f32 and att.scale.numel() == 256)


def _focused_linear_attention_train(xq, xkv, att, kv_skip=0):
    """The projections as in the composite (trainable linears), s = 1 / softplus(scale) a torch op, the core on `_LinearAttnFn`;
    `kv_skip` by slicing (autograd gives the skipped rows a zero gradient)."""
    if kv_skip:
        xkv = xkv[:, kv_skip:]
    q, k, v = _lin(xq, att.proj_q), _lin(xkv, att.proj_k), _lin(xkv, att.proj_v)
    s = (1.0 / F.softplus(att.scale)).reshape(-1)
    return _LinearAttnFn.apply(q, k, v, s)


def _focused_linear_attention_hip_f32(xq, xkv, att, focusing):
    """fp32 configuration: same two launches on fp32 data (csrc/linattn.hip linear_attn_f32_kernel: hi/lo-split
    MFMAs); projections are plain fp32 GEMMs, kv / k-sum tiny fp32 contractions."""
    B, N, C = xq.shape
    j = xkv.shape[1]
    key = (att.scale._version, att.scale.data_ptr(), "f32")
    cache = getattr(att, "_hip_cache_f32", None)
    if cache is None or cache[0] != key:
        with torch.no_grad():
            cache = (key, (1.0 / F.softplus(att.scale.float())).reshape(-1).contiguous())
        att._hip_cache_f32 = cache
    inv_sp = cache[1]
    q = _c(linear(xq, att.proj_q))
    kproj = _c(linear(xkv, att.proj_k))
    v = linear(xkv, att.proj_v)
    kf = torch.empty(B, j, C, dtype=torch.float32, device=xq.device)
    out = torch.empty(B, N, C, dtype=torch.float32, device=xq.device)
    with on_device(xq.device):
        call("unopose_linear_attention_f32", ptr(kproj), ptr(inv_sp), None, None, B, j, focusing, 1, ptr(kf), stream_ptr())
        ksum = _c(kf.sum(dim=1))
        if _own_f32(v) and v.dtype == torch.float32:
            # kv_h^T[d][c] = sum_j v[j,h,d] k[j,h,c]: (pair, head) batches, both operands read in place (j strided)
            kvt = bmm_nt_f32(v.reshape(B, j, 4, 64).permute(0, 2, 3, 1), kf.reshape(B, j, 4, 64).permute(0, 2, 3, 1))
        else:
            kvt = _c(torch.einsum("bjhd,bjhc->bhdc", v.reshape(B, j, 4, 64), kf.reshape(B, j, 4, 64)))
        call("unopose_linear_attention_f32", ptr(q), ptr(inv_sp), ptr(kvt), ptr(ksum), B, N, focusing, 0, ptr(out),
             stream_ptr())
    return out


def _focused_linear_attention_hip(xq, xkv, att, focusing, kv_skip=0):
    bf = torch.bfloat16
    B, N, C = xq.shape
    jr = xkv.shape[1]  # rows per pair in memory: the projection runs over all of them, the state over [kv_skip, jr)
    j = jr - kv_skip
    key = _params_key(att)
    cache = getattr(att, "_hip_cache", None)
    if cache is None or cache[0] != key:
        with torch.no_grad():
            w_kv = torch.cat([att.proj_k.weight.float(), att.proj_v.weight.float()], 0).to(bf).contiguous()
            b_kv = torch.cat([att.proj_k.bias.float(), att.proj_v.bias.float()], 0).to(bf).contiguous()
            inv_sp = (1.0 / F.softplus(att.scale.float())).reshape(-1).contiguous()
        cache = (key, w_kv, b_kv, inv_sp, b_kv.float())
        att._hip_cache = cache
    _, w_kv, b_kv, inv_sp, bkv32 = cache
    q = _c(linear(xq, att.proj_q))
    with torch.autocast("cuda", enabled=False):
        ykv = bf16_linear_2d(xkv.to(bf).reshape(B * jr, C), w_kv, bkv32, b_kv).reshape(B, jr, -1)
    out = torch.empty(B, N, C, dtype=bf, device=xq.device)
    if st.USE_LA_KV_STATE and C == 256:
        # focused keys, their sum and k^T v in one launch, read from the projection's rows in place (csrc/linattn.hip)
        kvt = torch.empty(B, 4, 64, 64, dtype=bf, device=xq.device)
        ksum = torch.empty(B, C, dtype=torch.float32, device=xq.device)
        with on_device(xq.device):
            call("unopose_linear_attention_kv_state", ptr(ykv), ptr(inv_sp), B, j, jr, kv_skip, focusing, ptr(kvt), ptr(ksum), stream_ptr())
            call("unopose_linear_attention", ptr(q), ptr(inv_sp), ptr(kvt), ptr(ksum), B, N, focusing, 0, ptr(out), stream_ptr())
        return out
    assert kv_skip == 0
    kproj, v = _c(ykv[..., :C]), ykv[..., C:]
    kf = torch.empty(B, j, C, dtype=bf, device=xq.device)
    with on_device(xq.device):
        call("unopose_linear_attention", ptr(kproj), ptr(inv_sp), None, None, B, j, focusing, 1, ptr(kf),
             stream_ptr())
        kf32 = kf.float()
        if _own_glue(kf):
            ksum = torch.empty(B, C, dtype=torch.float32, device=kf.device)  # (B,256): sum over the tokens
            call("unopose_token_sum_bf16", ptr(kf), B, j, C, ptr(ksum), stream_ptr())
        else:
            ksum = _c(kf32.sum(dim=1))
        # kv_h^T[d][c] = sum_j v[j,h,d] k[j,h,c]   (fp32 contraction: autocast would turn it into a library bf16 GEMM)
        with torch.autocast("cuda", enabled=False):
            if _own_f32(v):
                kvt = bmm_nt_f32(v.float().reshape(B, j, 4, 64).permute(0, 2, 3, 1), kf32.reshape(B, j, 4, 64).permute(0, 2, 3, 1)).to(bf)
            else:
                kvt = _c(torch.einsum("bjhd,bjhc->bhdc", v.float().reshape(B, j, 4, 64), kf32.reshape(B, j, 4, 64)).to(bf))
        call("unopose_linear_attention", ptr(q), ptr(inv_sp), ptr(kvt), ptr(ksum), B, N, focusing, 0, ptr(out),
             stream_ptr())
    return out


def focused_linear_attention_torch(xq, xkv, att, heads, focusing):
    """Op-by-op composite, kv branch (the shape test at transformer.py:560 is static)."""
    q, k, v = _lin(xq, att.proj_q), _lin(xkv, att.proj_k), _lin(xkv, att.proj_v)
    dt = v.dtype
    q, k = q.float(), k.float()
    scale = F.softplus(att.scale.float())
    q = (F.relu(q) + 1e-6) / scale
    k = (F.relu(k) + 1e-6) / scale
    qn, kn = q.norm(dim=-1, keepdim=True), k.norm(dim=-1, keepdim=True)
    q, k = q ** focusing, k ** focusing
    q = q / q.norm(dim=-1, keepdim=True) * qn
    k = k / k.norm(dim=-1, keepdim=True) * kn
    B, i, C = q.shape
    j = k.shape[1]
    hd = C // heads
    q = q.reshape(B, i, heads, hd)
    k = k.reshape(B, j, heads, hd)
    v = v.reshape(B, j, heads, hd)
    z = 1 / (torch.einsum("bihc,bhc->bih", q, k.sum(dim=1)) + 1e-6)
    if i * j * (hd + hd) > hd * hd * (i + j):
        kv = torch.einsum("bjhc,bjhd->bhcd", k.to(dt), v)
        x = torch.einsum("bihc,bhcd->bihd", q.to(dt), kv).float() * z.unsqueeze(-1)
    else:
        qk = torch.einsum("bihc,bjhc->bhij", q.to(dt), k.to(dt))
        x = torch.einsum("bhij,bjhd->bihd", qk, v).float() * z.unsqueeze(-1)
    return x.reshape(B, i, C).to(dt)
