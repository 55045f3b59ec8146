"""GPU: the dense layers' focused linear attention under autograd (the fp32 training step): `ops._LinearAttnFn`
(csrc/linattn_train.hip: key state, query forward, query-side and key-side backward, fixed-order partial sums) and the route
`ops.focused_linear_attention` takes inside `ops.differentiable()` (switch `ops.TRAIN_OWN_LINATTN`).

Reference: torch autograd over the composite core in float64 -- the body of `focused_linear_attention_torch` from the projections'
outputs, with s = 1 / softplus(scale) as a leaf -- on the same inputs.  The same composite also runs in fp32 on the GPU.  For each
of out, dyq, dyk, dv, ds, relative to that tensor's max|ref|, element-wise and in the Frobenius norm:
    kernel error <= max(4 x the fp32 composite's error, 1e-6)
(the rule of tests/test_add_layernorm_train_gpu.py for an fp32 route against an fp32 composite: two summation orders, and the
~16-ulp floor where the composite happens to be exact; it applies because every product of the kernels is an fp32 FMA).  Where
max|ref| is 0 the kernel's tensor must be exactly 0.  Both errors and their ratio are printed per tensor and case.

Measured on an MI355X over every tensor and case of this file: the largest ratio of the kernel's error to the composite's is 1.50
element-wise (ds, dead_keys: 1.70e-6 against 1.14e-6) and 1.48 in the Frobenius norm, the largest error above the floor 2.54e-4 of
max|ref| (ds, cancel; composite 2.99e-4) -- except at (1, 1, 1), where out ~ v and the query / key gradients are what rounding
leaves of a cancelled difference: dyq 0.252 (composite 0.0725, ratio 3.48, Frobenius 2.19), dyk 0.687 (0.572), ds 0.087 (0.063)."""
import copy
import ctypes

import pytest
import torch
import torch.nn.functional as F

from test_linear_attention_gpu import ADV, _att, _clean, _pool, adversarial, check, op_reference, wide_scale

pytestmark = pytest.mark.gpu
F32 = torch.float32
NAMES = ("out", "dyq", "dyk", "dv", "ds")
FACTOR, FLOOR = 4.0, 1e-6
SHAPES = [(1, 1, 1), (3, 33, 7), (2, 129, 196), (1, 257, 129), (3, 31, 257), (2, 4097, 196), (16, 130, 196)]


def core_torch(yq, yk, v, s):
    """The core of ops.focused_linear_attention_torch from the projections' outputs (kv form), in the dtype of its inputs."""
    q, k = (F.relu(yq) + 1e-6) * s, (F.relu(yk) + 1e-6) * s
    qn, kn = q.norm(dim=-1, keepdim=True), k.norm(dim=-1, keepdim=True)
    q, k = q ** 3, k ** 3
    q = q / q.norm(dim=-1, keepdim=True) * qn
    k = k / k.norm(dim=-1, keepdim=True) * kn
    B, N, _ = q.shape
    q, k, v = q.reshape(B, N, 4, 64), k.reshape(B, -1, 4, 64), v.reshape(B, -1, 4, 64)
    z = 1 / (torch.einsum("bihc,bhc->bih", q, k.sum(dim=1)) + 1e-6)
    kv = torch.einsum("bjhc,bjhd->bhcd", k, v)
    return (torch.einsum("bihc,bhcd->bihd", q, kv) * z.unsqueeze(-1)).reshape(B, N, 256)


def _kernel(yq, yk, v, s):
    from unopose_amd import ops

    return ops._LinearAttnFn.apply(yq, yk, v, s)


def _grads(fn, yq, yk, v, s, dO, dt):
    leaves = [x.detach().to(dt).requires_grad_(True) for x in (yq, yk, v, s)]
    out = fn(*leaves)
    out.backward(dO.to(dt))
    return [out.detach()] + [x.grad for x in leaves]


def _err(got, ref):
    scale = ref.abs().max().item()
    if scale == 0:
        return 0.0, 0.0, scale
    return ((got.double() - ref).abs().max().item() / scale, (got.double() - ref).norm().item() / ref.norm().item(), scale)


WORST = {"ratio": 0.0, "err": 0.0}


def _compare(label, got, ref, comp, names=NAMES):
    """The module docstring's rule for every tensor; prints the figures first."""
    fails = []
    for name, g, r, c in zip(names, got, ref, comp):
        assert torch.isfinite(g).all(), (label, name)
        e, fro, scale = _err(g, r)
        ec, froc, _ = _err(c, r)
        if scale == 0:
            print(f"{label} {name}: reference identically 0, kernel max {g.abs().max().item():.1e}")
            if torch.count_nonzero(g) != 0:
                fails.append((name, "not exactly 0"))
            continue
        ratio, rfro = e / max(ec, 1e-300), fro / max(froc, 1e-300)
        print(f"{label} {name}: kernel {e:.2e} (fro {fro:.2e}), fp32 composite {ec:.2e} (fro {froc:.2e}), ratio {ratio:.2f} (fro {rfro:.2f})")
        if e > FLOOR:
            WORST["ratio"] = max(WORST["ratio"], ratio)
        WORST["err"] = max(WORST["err"], e)
        if not e <= max(FACTOR * ec, FLOOR):
            fails.append((name, "element", e, ec))
        if not fro <= max(FACTOR * froc, FLOOR):
            fails.append((name, "frobenius", fro, froc))
    print(f"worst so far: ratio {WORST['ratio']:.2f} (above the floor), error {WORST['err']:.2e}")
    assert not fails, (label, fails)


def _inputs(B, N, J, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    yq, yk, v, dO = (torch.randn(B, r, 256, generator=g, device="cuda") for r in (N, J, J, N))
    _, s = wide_scale(g)
    return yq, yk, v, s, dO


def _three(yq, yk, v, s, dO):
    got = _grads(_kernel, yq, yk, v, s, dO, torch.float32)
    ref = _grads(core_torch, yq, yk, v, s, dO, torch.float64)
    comp = _grads(core_torch, yq, yk, v, s, dO, torch.float32)
    return got, ref, comp


@pytest.mark.parametrize("B,N,J", SHAPES)
def test_linear_attn_fn_matches_float64_autograd(B, N, J):
    """The ends of the kernels' row steps and workgroups, several workgroups' partials, one and many batches, one key."""
    yq, yk, v, s, dO = _inputs(B, N, J, seed=B * 10007 + N * 31 + J)
    _compare(f"B={B} N={N} J={J}", *_three(yq, yk, v, s, dO))


@pytest.mark.parametrize("case", ADV)
def test_linear_attn_fn_adversarial_values(case):
    """The six families of the forward tests; rows whose 256 inputs are all <= 0 get a gradient of exactly 0."""
    B, N, J = 2, 129, 196
    g, yq, yk, v = adversarial(case, torch.float32, B, N, J, seed=ADV.index(case))
    _, s = wide_scale(g)
    dO = torch.randn(B, N, 256, generator=g, device="cuda")
    got, ref, comp = _three(yq, yk, v, s, dO)
    _compare(case, got, ref, comp)
    for name, y, dy in (("dyq", yq, got[1]), ("dyk", yk, got[2])):
        dead = (y <= 0).all(dim=-1)
        assert torch.count_nonzero(dy[dead]) == 0, f"{case} {name}: a dead row has a gradient"
    if case == "dead_rows":
        assert (yq <= 0).all(dim=-1).any() and (yk <= 0).all(dim=-1).any()
    if case == "dead_keys":
        assert torch.count_nonzero(got[2]) == 0, "dyk must be exactly 0 when every key is dead"


@pytest.mark.parametrize("N,J", [(2049, 196), (33, 1)])
def test_training_route_forward_within_the_eval_bound(N, J):
    """Op level: the training route's output within the derived fp32 bound of tests/test_linear_attention_gpu.py, unchanged."""
    from unopose_amd import ops

    att = _att(N + J)
    g = torch.Generator(device="cuda").manual_seed(N * 7 + J)
    xq = torch.randn(2, N, 256, generator=g, device="cuda")
    xkv = torch.randn(2, J, 256, generator=g, device="cuda")
    old = ops.TRAIN_OWN_LINATTN
    ops.TRAIN_OWN_LINATTN = True
    try:
        assert ops.linear_attention_train_ok(xq, xkv, att, 4, 3)
        with ops.differentiable():
            out = ops.focused_linear_attention(xq, xkv, att, 4, 3)
    finally:
        ops.TRAIN_OWN_LINATTN = old
    assert out.grad_fn is not None and "LinearAttnFn" in type(out.grad_fn).__name__
    check(out.detach(), *op_reference(xq, xkv, att, "fp32"), f"train route N={N} J={J}")


def _layer_ref(layer, x, mem):
    """LinearTransformerLayer.forward with plain torch ops, in the dtype of the layer."""
    a, o = layer.attention, layer.output
    att = a.attention
    C = x.shape[-1]
    lin = lambda t, m: F.linear(t, m.weight, m.bias)  # noqa: E731
    s = (1.0 / F.softplus(att.scale)).reshape(-1)
    h = core_torch(lin(x, att.proj_q), lin(mem, att.proj_k), lin(mem, att.proj_v), s)
    y = F.layer_norm(lin(h, a.linear) + x, (C,), a.norm.weight, a.norm.bias, a.norm.eps)
    z = lin(F.relu(lin(y, o.expand)), o.squeeze)
    return F.layer_norm(y + z, (C,), o.norm.weight, o.norm.bias, o.norm.eps)


def _layer_run(mod, x, mem, dy, dt, fn):
    ins = [t.detach().to(dt).requires_grad_(True) for t in (x, mem)]
    for p in mod.parameters():
        p.grad = None
    fn(mod, *ins).backward(dy.to(dt))
    return {"x": ins[0].grad, "mem": ins[1].grad, **{k: p.grad.clone() for k, p in mod.named_parameters()}}


def _own(switch, kv_skip=0):
    from unopose_amd import ops

    def fn(mod, xi, mi):
        old = ops.TRAIN_OWN_LINATTN
        ops.TRAIN_OWN_LINATTN = switch
        try:
            with ops.differentiable():
                return mod(xi, mi, kv_skip=kv_skip)
        finally:
            ops.TRAIN_OWN_LINATTN = old

    return fn


def test_linear_transformer_layer_under_autograd_matches_float64():
    """LinearTransformerLayer inside ops.differentiable(): dx, dmem and every parameter gradient (proj_q/k/v, scale, linear, norm, the
    output block) against a float64 restatement of the layer; the fp32 composite is the same layer with the switch off.  Then
    kv_skip = 1 on a block whose first row is NaN: bit-equal to the sliced call, the NaN row's gradient exactly 0."""
    from unopose_amd.model.modules import LinearTransformerLayer

    torch.manual_seed(21)
    layer = LinearTransformerLayer(256).cuda()
    g = torch.Generator(device="cuda").manual_seed(6)
    with torch.no_grad():
        layer.attention.attention.scale.copy_(wide_scale(g)[0].reshape(1, 1, 256))
    B, N, J = 4, 300, 196
    x, mem, dy = (torch.randn(B, r, 256, generator=g, device="cuda") for r in (N, J, N))
    got = _layer_run(layer, x, mem, dy, torch.float32, _own(True))
    comp = _layer_run(layer, x, mem, dy, torch.float32, _own(False))
    ref = _layer_run(copy.deepcopy(layer).double(), x, mem, dy, torch.float64, _layer_ref)
    assert got.keys() == ref.keys() and "attention.attention.scale" in got
    keys = sorted(got)
    _compare("layer", [got[k] for k in keys], [ref[k] for k in keys], [comp[k] for k in keys], names=keys)

    blk = torch.cat([torch.full((B, 1, 256), float("nan"), device="cuda"), mem], 1)
    skip = _layer_run(layer, x, blk, dy, torch.float32, _own(True, kv_skip=1))
    for k in keys:
        want = got[k]
        have = skip[k][:, 1:] if k == "mem" else skip[k]
        assert torch.equal(have, want), f"kv_skip = 1: {k} differs from the sliced call"
    assert torch.count_nonzero(skip["mem"][:, 0]) == 0, "the skipped row has a gradient"


def test_deterministic():
    """Two forward + backward runs give equal bits for all five tensors."""
    yq, yk, v, s, dO = _inputs(3, 1301, 196, seed=99)
    a = _grads(_kernel, yq, yk, v, s, dO, torch.float32)
    b = _grads(_kernel, yq, yk, v, s, dO, torch.float32)
    for name, x, y in zip(NAMES, a, b):
        assert torch.equal(x, y), name


def _lib():
    from unopose_amd import _lib

    return _lib


def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _workspace(B, N, J):
    L = _lib().lib()
    n = L.unopose_linear_attention_f32_partials(B, N, J)
    assert n > 0
    return torch.empty(n, L.unopose_linear_attention_f32_partial_floats(), device="cuda"), n


@torch.no_grad()
def test_output_hygiene():
    """Every output of both entry points into NaN-payload-prefilled buffers with guard elements after them: every element written
    and finite, every guard element untouched."""
    B, N, J = 2, 129, 197
    yq, yk, v, s, dO = _inputs(B, N, J, seed=5)
    lib = _lib()
    ws, n = _workspace(B, N, J)
    outs = {"out": _pool((B, N, 256), F32, 32 * 256), "K": _pool((B, 4, 64, 64), F32, 4096), "Kt": _pool((B, 4, 64, 64), F32, 4096),
            "S": _pool((B, 256), F32, 256), "den": _pool((B, N, 4), F32, 128)}
    o = {k: t[0] for k, t in outs.items()}
    lib.call("unopose_linear_attention_f32_train", _vp(yq), _vp(yk), _vp(v), _vp(s), B, N, J, 3, _vp(o["out"]), _vp(o["K"]), _vp(o["Kt"]),
             _vp(o["S"]), _vp(o["den"]), _vp(ws), n, lib.stream_ptr())
    torch.cuda.synchronize()
    for k, (view, tail) in outs.items():
        _clean(view, tail, k)
    assert torch.equal(o["Kt"], o["K"].transpose(2, 3))
    grads = {"dyq": _pool((B, N, 256), F32, 32 * 256), "dyk": _pool((B, J, 256), F32, 32 * 256), "dv": _pool((B, J, 256), F32, 32 * 256),
             "ds": _pool((256,), F32, 256)}
    d = {k: t[0] for k, t in grads.items()}
    lib.call("unopose_linear_attention_f32_backward", _vp(dO), _vp(yq), _vp(yk), _vp(v), _vp(s), _vp(o["K"]), _vp(o["Kt"]), _vp(o["S"]),
             _vp(o["den"]), B, N, J, 3, _vp(d["dyq"]), _vp(d["dyk"]), _vp(d["dv"]), _vp(d["ds"]), _vp(ws), n, lib.stream_ptr())
    torch.cuda.synchronize()
    for k, (view, tail) in grads.items():
        _clean(view, tail, k)
    # the query pass alone (no gradient for keys, values and scale): the same dyq, nothing else touched
    q_only, tail = _pool((B, N, 256), F32, 32 * 256)
    lib.call("unopose_linear_attention_f32_backward", _vp(dO), _vp(yq), _vp(yk), _vp(v), _vp(s), _vp(o["K"]), _vp(o["Kt"]), _vp(o["S"]),
             _vp(o["den"]), B, N, J, 3, _vp(q_only), None, None, None, None, 0, lib.stream_ptr())
    torch.cuda.synchronize()
    _clean(q_only, tail, "dyq alone")
    assert torch.equal(q_only, d["dyq"])


@torch.no_grad()
def test_abi_rejects_bad_arguments():
    """Null pointer, N = 0, J = 0, focus = 2, a workspace that is too small: an error, and the NaN-prefilled outputs keep their bits."""
    B, N, J = 2, 40, 9
    yq, yk, v, s, dO = _inputs(B, N, J, seed=1)
    lib = _lib()
    ws, n = _workspace(B, N, J)
    nan = lambda *sh: torch.full(sh, float("nan"), device="cuda")  # noqa: E731
    out, K, Kt, S, den = nan(B, N, 256), nan(B, 4, 64, 64), nan(B, 4, 64, 64), nan(B, 256), nan(B, N, 4)
    dyq, dyk, dv, ds = nan(B, N, 256), nan(B, J, 256), nan(B, J, 256), nan(256)

    def train(yq_=yq, N_=N, J_=J, focus=3, K_=K, n_=n):
        lib.call("unopose_linear_attention_f32_train", _vp(yq_), _vp(yk), _vp(v), _vp(s), B, N_, J_, focus, _vp(out), _vp(K_), _vp(Kt), _vp(S),
                 _vp(den), _vp(ws), n_, lib.stream_ptr())

    def backward(dO_=dO, N_=N, J_=J, focus=3, dv_=dv, n_=n):
        lib.call("unopose_linear_attention_f32_backward", _vp(dO_), _vp(yq), _vp(yk), _vp(v), _vp(s), _vp(K), _vp(Kt), _vp(S), _vp(den),
                 B, N_, J_, focus, _vp(dyq), _vp(dyk), _vp(dv_), _vp(ds), _vp(ws), n_, lib.stream_ptr())

    for fn in (train, backward):
        with pytest.raises(RuntimeError, match="bad sizes"):
            fn(N_=0)
        with pytest.raises(RuntimeError, match="bad sizes"):
            fn(J_=0)
        with pytest.raises(RuntimeError, match="focusing_factor"):
            fn(focus=2)
    with pytest.raises(RuntimeError, match="null pointer"):
        train(yq_=None)
    with pytest.raises(RuntimeError, match="null pointer"):
        train(K_=None)
    with pytest.raises(RuntimeError, match="null pointer"):
        backward(dO_=None)
    with pytest.raises(RuntimeError, match="go together"):
        backward(dv_=None)
    with pytest.raises(RuntimeError, match="workspace"):
        train(n_=0)
    with pytest.raises(RuntimeError, match="workspace"):
        backward(n_=n - 1)
    assert lib.lib().unopose_linear_attention_f32_partials(B, 0, J) < 0 and lib.lib().unopose_linear_attention_f32_partials(70000, N, J) < 0
    torch.cuda.synchronize()
    for name, t in (("out", out), ("K", K), ("Kt", Kt), ("S", S), ("den", den), ("dyq", dyq), ("dyk", dyk), ("dv", dv), ("ds", ds)):
        assert t.isnan().all(), f"a rejected call wrote {name}"


def test_saved_tensors_hold_one_query_sized_tensor():
    """The function saves no tensor of B N 256 elements other than yq: the focused rows are recomputed, and the workspace stays below
    one such tensor."""
    B, N, J = 2, 4097, 196
    yq, yk, v, s, dO = _inputs(B, N, J, seed=3)
    saved = []
    leaves = [x.requires_grad_(True) for x in (yq, yk, v, s)]
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        out = _kernel(*leaves)
    big = [t for t in saved if t.numel() >= B * N * 256]
    assert len(big) == 1 and big[0].data_ptr() == yq.data_ptr(), [tuple(t.shape) for t in saved]
    assert sum(t.numel() for t in saved if t.data_ptr() not in {x.data_ptr() for x in leaves}) < B * N * 256 // 8
    ws, _ = _workspace(B, N, J)
    assert ws.numel() < B * N * 256
    out.backward(dO)
    assert all(x.grad is not None for x in leaves)


def test_needs_input_grad_skips_the_key_pass():
    """Without a gradient for keys, values and scale the backward is the query pass alone and gives the same dyq."""
    from torch.profiler import ProfilerActivity, profile

    yq, yk, v, s, dO = _inputs(2, 300, 196, seed=8)
    full = _grads(_kernel, yq, yk, v, s, dO, torch.float32)
    q = yq.detach().requires_grad_(True)
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        _kernel(q, yk, v, s).backward(dO)
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages()]
    assert any("la_query_bwd_kernel" in x for x in names) and not any("la_key_bwd_kernel" in x for x in names), names
    assert torch.equal(q.grad, full[1])


def _model():
    from oracle.unopose_ref import default_cfg, random_state_dict  # weights only
    from unopose_amd.model import UNOPose, default_model_cfg
    from unopose_amd.train import freeze_backbone

    m = UNOPose(default_model_cfg(fine_npoint=512))
    m.load_state_dict(random_state_dict(default_cfg(), seed=0, tame=0.1), strict=True)
    return freeze_backbone(m.cuda())


def test_training_step_runs_linear_attention_on_the_kernels(monkeypatch):
    """Route guard: in a training forward + backward of the small model, with the switch on, the new forward and backward kernels run
    and no aten::pow is left on a 3-D input of a dense-layer query tensor's shape.  Self-checking: with the switch off the pow
    entries come back and the new kernels are gone."""
    from torch.profiler import ProfilerActivity, profile
    from train_case import make_train_batch

    from unopose_amd import ops
    from unopose_amd.losses import process_loss

    model = _model().train()
    batch, aug = make_train_batch()
    shapes = set()
    inner = ops.focused_linear_attention

    def spy(xq, xkv, att, heads, focusing, kv_skip=0):
        shapes.add(tuple(xq.shape))
        return inner(xq, xkv, att, heads, focusing, kv_skip=kv_skip)

    monkeypatch.setattr(ops, "focused_linear_attention", spy)

    def step():
        ep = {k: v.cuda() for k, v in batch.items()}
        ep["aug_pose"] = (aug[0].cuda(), aug[1].cuda())
        model.zero_grad(set_to_none=True)
        process_loss(model(ep))["loss"].backward()
        torch.cuda.synchronize()

    def census():
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA], record_shapes=True) as prof:
            step()
        names = [e.key for e in prof.key_averages()]
        pows = []
        for e in prof.key_averages(group_by_input_shape=True):
            sh = [list(x) for x in e.input_shapes if isinstance(x, (list, tuple))]
            if e.key == "aten::pow" and sh and len(sh[0]) == 3 and tuple(sh[0]) in shapes:
                pows.append(sh[0])
        return names, pows

    kernels = ("la_key_state_kernel", "la_query_fwd_kernel", "la_query_bwd_kernel", "la_key_bwd_kernel", "la_reduce_state_kernel",
               "la_reduce_ds_kernel")
    old = ops.TRAIN_OWN_LINATTN
    try:
        ops.TRAIN_OWN_LINATTN = True
        step()  # caches
        assert shapes, "the model ran no focused linear attention"
        names, pows = census()
        assert pows == [], pows
        for k in kernels:
            assert any(k in x for x in names), k
        ops.TRAIN_OWN_LINATTN = False
        names, pows = census()
        assert pows, "the composite's pow did not come back with the switch off"
        assert not any(k in x for k in kernels for x in names)
    finally:
        ops.TRAIN_OWN_LINATTN = old
