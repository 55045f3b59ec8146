"""GPU: the correspondence transformer's token attention under autograd (the fp32 training step): `ops._TokenAttnFn` (csrc/attn_f32.hip:
the eval kernel storing P, then the dq / dS, dk / dv and RPE backward kernels) against torch autograd over the op-by-op composite in
float64, its route inside `ops.differentiable()`, and its determinism.

Bounds: every tensor is compared against float64 relative to its own max|ref|, element-wise and in the Frobenius norm.  The fp32
composite's own error is printed next to the kernels'.  The kernels' products are hi / lo-split bf16 MFMAs where the forward uses them
(scores, P v; in the backward dO v^T and dS k): ~2^-16 relative per product, so a score of magnitude |S| carries ~|S| 2^-16, which moves P,
and everything after it, by that much relative: measured 1.4e-5 element-wise and 8e-6 Frobenius at most over the shapes below, 10-20x the
fp32 composite's error.  The rest (dk, dv, dqp, dE) is exact fp32 FMA.  EL / FRO are those largest errors times a margin of ~3.5."""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
KP = 224
EL, FRO = 5e-5, 3e-5  # element-wise (of max|ref|) and Frobenius bounds of the kernels' results
SHAPES = [(2, 197, 197), (16, 197, 197), (3, 64, 80), (1, 5, 5), (2, 1, 224), (2, 197, 1)]
NAMES = ("out", "dq", "dk", "dv", "dqp", "dE")


def _inputs(B, n, m, rpe, seed, dev="cuda"):
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(B, r, 256, generator=g) for r in (n, m, m))
    qp = 0.05 * torch.randn(B, n, 4, 256, generator=g) if rpe else None
    E = torch.randn(B, n, m, 256, generator=g) if rpe else None
    dO = torch.randn(B, n, 256, generator=g)
    t = [q, k, v, qp, E, dO]
    return [None if x is None else x.to(dev) for x in t]


def core_torch(q, k, v, qp=None, E=None):
    """The attention core of ops.token_attention_torch from the projections' outputs (q.b_p dropped: constant along every row)."""
    B, n, _ = q.shape
    q4, k4, v4 = q.reshape(B, n, 4, 64), k.reshape(B, -1, 4, 64), v.reshape(B, -1, 4, 64)
    s = torch.einsum("bnhc,bmhc->bhnm", q4, k4)
    if qp is not None:
        s = s + torch.einsum("bnhd,bnmd->bhnm", qp, E)
    p = torch.softmax(s * 0.125, dim=-1)
    return torch.einsum("bhnm,bmhc->bnhc", p, v4).reshape(B, n, 256)


def _grads(fn, q, k, v, qp, E, dO, dt):
    leaves = [None if x is None else x.detach().to(dt).requires_grad_(True) for x in (q, k, v, qp, E)]
    out = fn(*leaves)
    out.backward(dO.to(dt))
    return [out.detach()] + [None if x is None else x.grad for x in leaves]


def _kernel(q, k, v, qp, E):
    from unopose_amd import ops

    return ops._TokenAttnFn.apply(q, k, v, qp, E, None)


def _errs(got, ref):
    scale = ref.abs().max().item()
    e = (got.double() - ref).abs().max().item()
    fro = (got.double() - ref).norm().item() / max(ref.norm().item(), 1e-300)
    return e, scale, fro


def _check(label, got, ref, comp=None, atol=1e-6):
    """got / comp (fp32) against ref (float64): element-wise within EL of max|ref| (+ atol for tensors that are ~0), Frobenius within FRO."""
    for name, g, r, c in zip(NAMES, got, ref, comp or [None] * len(got)):
        if r is None:
            assert g is None, (label, name)
            continue
        assert torch.isfinite(g).all(), (label, name)
        e, scale, fro = _errs(g, r)
        line = f"{label} {name}: kernel {e / max(scale, 1e-300):.2e} (fro {fro:.2e})"
        if c is not None:
            ec, _, froc = _errs(c, r)
            line += f", fp32 composite {ec / max(scale, 1e-300):.2e} (fro {froc:.2e})"
        print(line)
        assert e <= EL * scale + atol, (label, name, e, scale)
        if r.norm().item() > 1e3 * atol:
            assert fro <= FRO, (label, name, fro)


@pytest.mark.parametrize("rpe", [True, False])
@pytest.mark.parametrize("B,n,m", SHAPES)
def test_token_attn_fn_matches_float64_autograd(B, n, m, rpe):
    q, k, v, qp, E, dO = _inputs(B, n, m, rpe, seed=B * 10007 + n * 31 + m)
    got = _grads(_kernel, q, k, v, qp, E, dO, torch.float32)
    ref = _grads(core_torch, q, k, v, qp, E, dO, torch.float64)
    comp = _grads(core_torch, q, k, v, qp, E, dO, torch.float32)
    _check(f"B={B} n={n} m={m} rpe={rpe}", got, ref, comp)
    if m == 1:  # P == 1: dS == 0, so no gradient reaches q, k, qp or E
        for name, g in zip(NAMES, got):
            if g is not None and name in ("dq", "dk", "dqp", "dE"):
                assert torch.count_nonzero(g) == 0, name


@pytest.mark.parametrize("case", ["one_hot", "uniform", "zero_rows"])
def test_token_attn_fn_adversarial_rows(case):
    """Scores near +-80 (one-hot P), identical keys (uniform P), zero query rows and zero output gradients."""
    B, n, m = 2, 37, 150
    q, k, v, qp, E, dO = _inputs(B, n, m, True, seed=7)
    if case == "one_hot":  # every query row aligns with one key: score 0.125 * 640 = 80 for it, about -80 / 0 for the rest
        key = torch.randint(0, m, (B, n), generator=torch.Generator().manual_seed(3)).cuda()
        k = torch.sign(torch.randn(B, m, 256, device="cuda"))
        q = 10 * torch.gather(k, 1, key.unsqueeze(-1).expand(B, n, 256))
        qp = torch.zeros_like(qp)
    elif case == "uniform":
        k = k[:, :1].expand(B, m, 256).contiguous()
        E = E[:, :, :1].expand(B, n, m, 256).contiguous()
    else:
        q[:, ::3] = 0
        qp[:, ::3] = 0
        dO[:, 1::4] = 0
    got = _grads(_kernel, q, k, v, qp, E, dO, torch.float32)
    ref = _grads(core_torch, q, k, v, qp, E, dO, torch.float64)
    _check(case, got, ref, atol=1e-5)


def _layer_ref(layer, x, mem, embed):
    """TransformerLayer.forward in float64 with plain torch ops (transformer.py:196-227 / 444-466, the q.b_p term included)."""
    a = layer.attention
    att = a.attention
    B, n, C = x.shape
    mem = x if mem is None else mem
    q = F.linear(x, att.proj_q.weight, att.proj_q.bias).reshape(B, n, 4, 64)
    k = F.linear(mem, att.proj_k.weight, att.proj_k.bias).reshape(B, -1, 4, 64)
    v = F.linear(mem, att.proj_v.weight, att.proj_v.bias).reshape(B, -1, 4, 64)
    s = torch.einsum("bnhc,bmhc->bhnm", q, k)
    if embed is not None:
        pe = F.linear(embed, att.proj_p.weight, att.proj_p.bias).reshape(B, n, -1, 4, 64)
        s = s + torch.einsum("bnhc,bnmhc->bhnm", q, pe)
    h = torch.einsum("bhnm,bmhc->bnhc", torch.softmax(s * 0.125, dim=-1), v).reshape(B, n, C)
    y = F.layer_norm(F.linear(h, a.linear.weight, a.linear.bias) + x, (C,), a.norm.weight, a.norm.bias, a.norm.eps)
    o = layer.output
    z = F.linear(F.relu(F.linear(y, o.expand.weight, o.expand.bias)), o.squeeze.weight, o.squeeze.bias)
    return F.layer_norm(y + z, (C,), o.norm.weight, o.norm.bias, o.norm.eps)


@pytest.mark.parametrize("rpe", [True, False])
def test_transformer_layer_under_autograd_matches_float64(rpe):
    """TransformerLayer inside ops.differentiable(): every parameter gradient plus dx, dmem and dE against float64; proj_p.bias gets
    its gradient, zero."""
    from unopose_amd import ops
    from unopose_amd.model.modules import TransformerLayer

    torch.manual_seed(11 + rpe)
    layer = TransformerLayer(256, rpe).cuda()
    B, n, m = 4, 197, 197 if rpe else 150
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, n, 256, generator=g).cuda()
    mem = None if rpe else torch.randn(B, m, 256, generator=g).cuda()
    embed = torch.randn(B, n, m, 256, generator=g).cuda() if rpe else None
    dy = torch.randn(B, n, 256, generator=g).cuda()

    def run(mod, dt, fn):
        ins = [None if t is None else t.detach().to(dt).requires_grad_(True) for t in (x, mem, embed)]
        for p in mod.parameters():
            p.grad = None
        fn(mod, *ins).backward(dy.to(dt))
        return {"x": ins[0].grad, "mem": None if mem is None else ins[1].grad, "E": None if embed is None else ins[2].grad,
                **{k: p.grad for k, p in mod.named_parameters()}}

    def own(mod, xi, mi, ei):
        with ops.differentiable():
            return mod(xi, mi, ei)

    got = run(layer, torch.float32, own)
    ref = run(copy.deepcopy(layer).double(), torch.float64, _layer_ref)
    assert got.keys() == ref.keys()
    top = max(r.abs().max().item() for r in ref.values() if r is not None)
    for key in got:
        if ref[key] is None:
            continue
        assert got[key] is not None, key
        if key.endswith("proj_p.bias"):
            assert torch.count_nonzero(got[key]) == 0 and ref[key].abs().max().item() < 1e-9, key
            continue
        e, scale, fro = _errs(got[key], ref[key])
        print(f"rpe={rpe} {key}: {e / top:.2e} of the largest gradient, {e / scale:.2e} of its own (fro {fro:.2e})")
        if scale < 1e-9 * top:  # a gradient that is zero in exact arithmetic (proj_k.bias: q.b_k is constant along every row)
            assert e <= EL * top, (key, e, top)
            continue
        assert e <= EL * scale and fro <= FRO, (key, e, scale, fro)


def test_deterministic_and_forward_equals_the_eval_kernel():
    """Two forward + backward runs give the same bits; the training forward's O is unopose_token_attention_f32's."""
    from unopose_amd import ops
    from unopose_amd._lib import call, ptr, stream_ptr

    B, n, m = 3, 197, 197
    q, k, v, qp, E, dO = _inputs(B, n, m, True, seed=99)
    a = _grads(_kernel, q, k, v, qp, E, dO, torch.float32)
    b = _grads(_kernel, q, k, v, qp, E, dO, torch.float32)
    for name, x, y in zip(NAMES, a, b):
        assert torch.equal(x, y), name
    vt = ops._transpose_pad_f32(v)
    for rpe in (True, False):
        out = torch.empty(B, n, 256, device="cuda")
        call("unopose_token_attention_f32", ptr(q), 256, ptr(k), 256, ptr(vt), ptr(qp) if rpe else None, 1024, ptr(E) if rpe else None,
             B, n, m, 0.125, ptr(out), stream_ptr())
        with torch.no_grad():
            train = _kernel(q, k, v, qp if rpe else None, E if rpe else None)
        assert torch.equal(out, train), rpe


def _model():
    from oracle.unopose_ref import default_cfg, random_state_dict  # weights only
    from unopose_amd.model import UNOPose, default_model_cfg
    from unopose_amd.train import freeze_backbone

    m = UNOPose(default_model_cfg(fine_npoint=512))
    m.load_state_dict(random_state_dict(default_cfg(), seed=0, tame=0.1), strict=True)
    return freeze_backbone(m.cuda())


def test_training_step_runs_token_attention_on_the_kernels(monkeypatch):
    """Route guard: in a training forward + backward of the small model the new kernels run, and no bmm / softmax of the composite's
    core shapes ([B.4, n, 64] x [B.4, 64, m], [B.n, 4, 256] x [B.n, 256, m], their backward siblings, softmax over (B, 4, n, m)) is left
    at the sizes the token attention layers see.  Self-checking: with ops.TRAIN_OWN_ATTN = False they come back."""
    from torch.profiler import ProfilerActivity, profile
    from train_case import make_train_batch

    from unopose_amd import ops
    from unopose_amd.losses import process_loss

    model = _model().train()
    batch, aug = make_train_batch()
    sizes = set()
    inner = ops.token_attention

    def spy(x, mem, att, heads, embed=None):
        if mem.shape[1] <= KP:
            sizes.add((x.shape[0], x.shape[1], mem.shape[1]))
        return inner(x, mem, att, heads, embed)

    monkeypatch.setattr(ops, "token_attention", spy)

    def step():
        ep = {k: v.cuda() for k, v in batch.items()}
        ep["aug_pose"] = (aug[0].cuda(), aug[1].cuda())
        model.zero_grad(set_to_none=True)
        process_loss(model(ep))["loss"].backward()
        torch.cuda.synchronize()

    def composite_like(shapes):
        if len(shapes) < 2 or any(len(s) != 3 for s in shapes[:2]):
            return False
        (a, x, y), (a2, y2, z) = shapes[0], shapes[1]
        if a != a2 or y != y2:
            return False
        dims = sorted((x, y, z))
        return any((a == B * 4 and dims == sorted((n, m, 64))) or (a == B * n and dims == sorted((4, 256, m))) for B, n, m in sizes)

    def census():
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA], record_shapes=True) as prof:
            step()
        names = [e.key for e in prof.key_averages()]
        bad = []
        for e in prof.key_averages(group_by_input_shape=True):
            shapes = [list(s) for s in e.input_shapes if isinstance(s, (list, tuple))]
            if e.key == "aten::bmm" and composite_like(shapes):
                bad.append((e.key, shapes))
            if "softmax" in e.key and shapes and len(shapes[0]) == 4 and any(shapes[0] == [B, 4, n, m] for B, n, m in sizes):
                bad.append((e.key, shapes))
        return names, bad

    step()  # caches
    assert sizes, "the model ran no token attention within the kernels' key count"
    names, bad = census()
    assert bad == [], bad
    for kname in ("token_attn_f32_kernel", "token_attn_f32_bwd_dq_kernel", "token_attn_f32_bwd_dkv_kernel", "token_attn_f32_bwd_rpe_kernel"):
        assert any(kname in x for x in names), kname
    ops.TRAIN_OWN_ATTN = False
    try:
        names, bad = census()
    finally:
        ops.TRAIN_OWN_ATTN = True
    assert len(bad) >= 3, bad
    assert not any("token_attn_f32_bwd" in x for x in names)
