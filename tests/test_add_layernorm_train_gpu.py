"""GPU: residual add + LayerNorm under autograd (the training step's post-LN glue): `ops._AddLayerNormFn` / `ops.add_layernorm_train`
(csrc/ln_train.hip: forward keeping the sum and the row statistics, backward writing dx and per-slab partials of dweight / dbias, the launch
that adds the partials) against torch autograd over `F.layer_norm(a + b, ...)` in float64 on the same inputs, its route inside
`ops.differentiable()`, its contract and its determinism.

Bound, on every tensor (y, da, db, dweight, dbias), element-wise relative to that tensor's max|ref|: the kernels' error <= max(4 x the
error of the fp32 torch composite on the GPU, 1e-6).  The factor allows for the different summation orders of two fp32 routes (neither is the more accurate
one by construction); the floor, ~16 fp32 ulps, for the cases where the composite happens to be exact (dbias at one row: a copy).  Both errors are printed per case.
Measured on an MI355X over the cases of this file: the largest kernel / composite ratio is 2.3 (dbias of the single-input case at
788 x 256: 1.5e-7 against 6.4e-8), every other tensor stays below 1.6; the kernels' largest error is 3.2e-6 (dweight on the rows shifted by
+100, composite 3.3e-6), everything else is below 2e-7."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
EPS = 1e-5
FACTOR, FLOOR = 4.0, 1e-6
NAMES = ("y", "da", "db", "dweight", "dbias")
SHAPES = [(1, 256), (5, 256), (788, 256), (4099, 256), (67, 4), (130, 768), (67, 1024)]


def _inputs(rows, C, family="normal", seed=0):
    """a, b, weight, bias, dy (fp32, on the GPU).  Families: standard normal rows; rows shifted by +100 (mean / sigma ~ 70: where a
    one-pass variance fails); rows shifted by +3 with two channels at +-50."""
    g = torch.Generator().manual_seed(seed * 1000003 + rows * 1031 + C)
    a, b, dy = (torch.randn(rows, C, generator=g) for _ in range(3))
    if family == "shift100":
        a = a + 100.0
    elif family == "outliers":
        a = a + 3.0
        a[:, 1 % C] = 50.0
        a[:, C - 1] = -50.0
        b[:, 1 % C] = 0.0
        b[:, C - 1] = 0.0
    else:
        assert family == "normal"
    w = 1.0 + 0.5 * torch.randn(C, generator=g)
    bias = 0.3 * torch.randn(C, generator=g)
    return [t.cuda() for t in (a, b, w, bias, dy)]


def _composite(a, b, w, bias):
    return F.layer_norm(a if b is None else a + b, (a.shape[-1],), w, bias, EPS)


def _kernel(a, b, w, bias):
    from unopose_amd import ops

    return ops._AddLayerNormFn.apply(a, b, w, bias, EPS)


def _grads(fn, a, b, w, bias, dy, dt=None, param_grads=True):
    """y and the gradients of fresh leaves (cast to `dt` when given), in the order of NAMES; None where there is no such input."""
    cast = (lambda t: t.detach().clone()) if dt is None else (lambda t: t.detach().to(dt))
    la, lb = cast(a).requires_grad_(True), None if b is None else cast(b).requires_grad_(True)
    lw, lbias = cast(w).requires_grad_(param_grads), cast(bias).requires_grad_(param_grads)
    y = fn(la, lb, lw, lbias)
    y.backward(dy if dt is None else dy.to(dt))
    return [y.detach(), la.grad, None if lb is None else lb.grad, lw.grad, lbias.grad]


def _check(label, got, ref, comp, names=NAMES):
    """Every tensor of `got` (the kernels) within max(FACTOR x the composite's error, FLOOR) of `ref` (float64), relative to max|ref|."""
    worst = 0.0
    for name, g, r, c in zip(NAMES, got, ref, comp):
        if name not in names:
            continue
        if r is None:
            assert g is None, (label, name)
            continue
        assert g is not None and g.dtype == torch.float32 and g.shape == r.shape and torch.isfinite(g).all(), (label, name)
        scale = max(r.abs().max().item(), 1e-300)
        ek = (g.double() - r).abs().max().item() / scale
        ec = (c.double() - r).abs().max().item() / scale
        if ec > 0:
            worst = max(worst, ek / ec)
        print(f"{label} {name}: kernel {ek:.2e}, fp32 composite {ec:.2e} of max|ref| = {scale:.3g}")
        assert ek <= max(FACTOR * ec, FLOOR), (label, name, ek, ec)
    print(f"{label}: largest kernel / composite ratio {worst:.2f}")


def _three_way(a, b, w, bias, dy):
    return (_grads(_kernel, a, b, w, bias, dy), _grads(_composite, a, b, w, bias, dy, torch.float64), _grads(_composite, a, b, w, bias, dy))


@pytest.mark.parametrize("rows,C", SHAPES)
def test_kernels_match_float64_autograd(rows, C):
    a, b, w, bias, dy = _inputs(rows, C)
    _check(f"rows={rows} C={C}", *_three_way(a, b, w, bias, dy))


@pytest.mark.parametrize("family", ["normal", "shift100", "outliers"])
def test_kernels_match_float64_autograd_on_off_centre_rows(family):
    a, b, w, bias, dy = _inputs(788, 256, family, seed=1)
    _check(family, *_three_way(a, b, w, bias, dy))


def test_bf16_addend_with_fp32_residual():
    """What `train.amp` with bf16 hands over: linear's bf16 output + the fp32 residual.  da is db rounded to bf16."""
    a, b, w, bias, dy = _inputs(788, 256, seed=2)
    a = a.to(torch.bfloat16)
    got = _grads(_kernel, a, b, w, bias, dy)
    ref = _grads(_composite, a, b, w, bias, dy, torch.float64)
    comp = _grads(_composite, a, b, w, bias, dy)  # a + b promotes to fp32, as in the composite route
    assert got[1].dtype == torch.bfloat16 and torch.equal(got[1], got[2].to(torch.bfloat16))
    _check("bf16 + fp32", got, ref, comp, names=("y", "db", "dweight", "dbias"))
    both = _grads(_kernel, a, b.to(torch.bfloat16), w, bias, dy)
    assert both[1].dtype == both[2].dtype == torch.bfloat16 and torch.equal(both[1], both[2])


def test_single_input():
    a, _, w, bias, dy = _inputs(788, 256, seed=3)
    _check("b=None", *_three_way(a, None, w, bias, dy))


def test_same_leaf_as_both_inputs_gets_twice_dx():
    a, _, w, bias, dy = _inputs(130, 256, seed=4)
    x = a.clone().requires_grad_(True)
    _kernel(x, x, w, bias).backward(dy)
    sep = _grads(_kernel, a, a.clone(), w, bias, dy)
    assert torch.equal(sep[1], sep[2]) and torch.equal(x.grad, 2 * sep[1])


def test_non_contiguous_output_gradient():
    a, b, w, bias, dy = _inputs(788, 256, seed=5)
    wide = torch.zeros(788, 257, device="cuda")
    wide[:, 1:] = dy
    assert not wide[:, 1:].is_contiguous()
    got = _grads(_kernel, a, b, w, bias, wide[:, 1:])
    _check("strided dy", got, _grads(_composite, a, b, w, bias, dy, torch.float64), _grads(_composite, a, b, w, bias, dy))
    for name, x, y in zip(NAMES, got, _grads(_kernel, a, b, w, bias, dy)):
        assert torch.equal(x, y), name


def test_frozen_parameters_get_no_gradient_and_dx_keeps_its_bits():
    a, b, w, bias, dy = _inputs(4099, 256, seed=6)
    full = _grads(_kernel, a, b, w, bias, dy)
    frozen = _grads(_kernel, a, b, w, bias, dy, param_grads=False)
    assert frozen[3] is None and frozen[4] is None
    for i in (0, 1, 2):
        assert torch.equal(full[i], frozen[i]), NAMES[i]


def test_backward_is_deterministic():
    a, b, w, bias, dy = _inputs(4099, 256, seed=7)
    one, two = _grads(_kernel, a, b, w, bias, dy), _grads(_kernel, a, b, w, bias, dy)
    for name, x, y in zip(NAMES, one, two):
        assert torch.equal(x, y), name


@pytest.mark.parametrize("C", [6, 1028])
def test_contract_on_the_channel_count(C):
    """Outside C % 4 == 0, 4 <= C <= 1024 both entry points return an error, `add_layernorm_train_ok` says no and `add_layernorm_train`
    is the composite."""
    from unopose_amd import ops
    from unopose_amd._lib import lib, ptr, stream_ptr

    rows = 9
    g = torch.Generator().manual_seed(C)
    a, b = torch.randn(rows, C, generator=g).cuda(), torch.randn(rows, C, generator=g).cuda()
    norm = torch.nn.LayerNorm(C).cuda()
    y, s, dx = torch.empty_like(a), torch.empty_like(a), torch.empty_like(a)
    mean, rstd = torch.zeros(rows, device="cuda"), torch.ones(rows, device="cuda")
    part, dw, db = torch.empty(4, 2, C, device="cuda"), torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    L = lib()
    assert L.unopose_add_layernorm_train(ptr(a), 0, ptr(b), 0, ptr(norm.weight), ptr(norm.bias), rows, C, EPS, ptr(y), ptr(s), ptr(mean), ptr(rstd),
                                         stream_ptr()) != 0
    assert b"unsupported" in L.unopose_last_error()
    assert L.unopose_add_layernorm_backward(ptr(a), ptr(s), ptr(mean), ptr(rstd), ptr(norm.weight), rows, C, ptr(dx), ptr(dw), ptr(db), ptr(part), 4,
                                            stream_ptr()) != 0
    assert L.unopose_add_layernorm_backward_slabs(rows, C) < 0
    assert not ops.add_layernorm_train_ok(a, b, norm)
    assert torch.equal(ops.add_layernorm_train(a, b, norm), norm(a + b))


def test_layernorm_without_affine_parameters_takes_the_composite():
    from unopose_amd import ops

    a, b, _, _, _ = _inputs(67, 256, seed=8)
    norm = torch.nn.LayerNorm(256, elementwise_affine=False).cuda()
    assert not ops.add_layernorm_train_ok(a, b, norm)
    assert torch.equal(ops.add_layernorm_train(a, b, norm), norm(a + b))
    affine = torch.nn.LayerNorm(256).cuda()
    assert ops.add_layernorm_train_ok(a, b, affine) and ops.add_layernorm_train_ok(a, None, affine)
    assert not ops.add_layernorm_train_ok(a, b, torch.nn.LayerNorm(256).cuda().double())
    assert not ops.add_layernorm_train_ok(a.double(), b.double(), affine)
    ops.TRAIN_OWN_LN = False
    try:
        assert not ops.add_layernorm_train_ok(a, b, affine)
    finally:
        ops.TRAIN_OWN_LN = True


def _model():
    from oracle.unopose_ref import default_cfg, random_state_dict  # weights only
    from unopose_amd.model import UNOPose, default_model_cfg
    from unopose_amd.train import freeze_backbone

    m = UNOPose(default_model_cfg(fine_npoint=512))
    m.load_state_dict(random_state_dict(default_cfg(), seed=0, tame=0.1), strict=True)
    return freeze_backbone(m.cuda())


def _stepper(model):
    from train_case import make_train_batch

    from unopose_amd.losses import process_loss

    batch, aug = make_train_batch()

    def step():
        ep = {k: v.cuda() for k, v in batch.items()}
        ep["aug_pose"] = (aug[0].cuda(), aug[1].cuda())
        model.zero_grad(set_to_none=True)
        loss = process_loss(model(ep))["loss"]
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach()

    return step


FWD_KERNEL, BWD_KERNELS = "add_layernorm_train_kernel", ("add_layernorm_bwd_kernel", "add_layernorm_bwd_params_kernel")


def test_training_step_runs_add_layernorm_on_the_kernels():
    """Route guard: in a training forward + backward of the small model no aten layer norm (forward or backward) over 256 channels is
    left and the new kernels run.  Self-checking: with ops.TRAIN_OWN_LN = False the aten ops come back and the kernels are gone."""
    from torch.profiler import ProfilerActivity, profile

    from unopose_amd import ops

    step = _stepper(_model().train())

    def census():
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA], record_shapes=True) as prof:
            step()
        names = [e.key for e in prof.key_averages()]
        aten = set()
        for e in prof.key_averages(group_by_input_shape=True):
            if e.key in ("aten::native_layer_norm", "aten::native_layer_norm_backward"):
                shapes = [list(s) for s in e.input_shapes if isinstance(s, (list, tuple))]
                if [256] in shapes:  # the weight (and bias) of a LayerNorm over 256 channels
                    aten.add(e.key)
        return names, aten

    step()  # caches
    names, aten = census()
    assert aten == set(), aten
    for k in (FWD_KERNEL,) + BWD_KERNELS:
        assert any(k in n for n in names), k
    ops.TRAIN_OWN_LN = False
    try:
        names, aten = census()
    finally:
        ops.TRAIN_OWN_LN = True
    assert aten == {"aten::native_layer_norm", "aten::native_layer_norm_backward"}, aten
    assert not any(k in n for n in names for k in (FWD_KERNEL,) + BWD_KERNELS)


def test_training_step_matches_the_composite_route():
    """The small model's loss with the switch on and off agrees to 1e-5 relative; every trainable parameter has a gradient, and it agrees
    within the bound test_train_gpu.py::test_training_forward_backward_matches_reference puts on gradients (norm within 3 %, 10 % for the
    positional-encoding MLP; the first 16 entries within 5 % + a tenth of the largest of them)."""
    from unopose_amd import ops

    model = _model().train()
    step = _stepper(model)

    def run():
        loss = float(step())
        return loss, {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.named_parameters() if p.requires_grad}

    loss_on, g_on = run()
    ops.TRAIN_OWN_LN = False
    try:
        loss_off, g_off = run()
    finally:
        ops.TRAIN_OWN_LN = True
    print(f"loss: kernels {loss_on:.8f}, composite {loss_off:.8f}")
    assert abs(loss_on - loss_off) <= 1e-5 * abs(loss_off), (loss_on, loss_off)
    assert [k for k, g in g_on.items() if g is None] == []
    assert g_on.keys() == g_off.keys() and len(g_on) > 100
    worst = 0.0
    for k, g in g_on.items():
        want = g_off[k]
        assert want is not None and torch.isfinite(g).all(), k
        tol = 0.1 if ".PE." in k else 3e-2
        nw = float(want.norm())
        if nw > 1e-5:  # (gradients that are zero in exact arithmetic, such as proj_k.bias, only meet the absolute term)
            worst = max(worst, abs(float(g.norm()) - nw) / nw)
        assert abs(float(g.norm()) - nw) < tol * nw + 1e-7, (k, float(g.norm()), nw)
        head, hw = g.flatten()[:16], want.flatten()[:16]
        assert torch.all((head - hw).abs() <= 5e-2 * hw.abs() + 0.1 * hw.abs().max() + 1e-8), k
    print(f"largest relative difference of a gradient norm: {worst:.2e}")
