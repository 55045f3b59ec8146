"""GPU: the small trainable linears of the matcher's 197-token layers under autograd: `ops._SmallLinearFn` (csrc/linear_small_train.hip:
forward, dX, dW + db, each straight from the fp32 tensors as stored) and the route `ops.linear` takes inside `ops.differentiable()` (switch
`ops.TRAIN_OWN_SMALL_LINEAR`).  The switch ships off (the measured gain of the training step did not clear the rule for its default, DESIGN.md
section 7), so every test of this file that exercises the kernels turns it on for its own duration (`switch_on`); the default itself is pinned by
`test_route_everything_else_as_before`.

Reference: torch.nn.functional.linear (+ relu) under autograd in float64 on the same inputs.  y, dx, dW and db are compared element-wise,
each relative to max|ref| of that tensor:
    y, dx   3e-5   fp32 class: bf16 hi / lo split, three MFMAs per product (the bound of tests/test_train_gpu.py, fp32 branch of
                   test_trainable_linear_on_own_gemm_matches_torch_autograd)
    dW, db  2e-6   exact fp32 products, row slices combined in double (the bound of test_own_linear_weight_gradient_matches_float64)
ReLU: where the float64 pre-activation lies within 1e-4 of its own max|.| the gradients are checked with the kernel's mask (y > 0 of the
forward's own output), everywhere else the kernel's mask must equal the reference's; such unclear elements stay under 1 % in every case.
Inputs are drawn on the CPU from seeded generators, so the unclear share can be (and was) confirmed without a GPU: at most 1.95e-3
(one element of 512 at rows 1, K 256, N 512), 4e-4 at the model's shapes; on the GPU no mask differed outside the unclear elements.

Measured on an MI355X, the largest error per tensor and input family over every shape of this file (relu off and on):
    family      y         dx        dW        db
    normal      6.36e-06  5.61e-06  5.40e-07  3.40e-07
    offcentre   8.07e-06  5.77e-06  4.41e-07  1.44e-07
    sparse_g    5.77e-06  5.85e-06  1.56e-07  1.47e-07
    scaled      6.58e-06  6.22e-06  5.45e-07  3.09e-07"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROWS = (1, 63, 64, 65, 197, 591, 1576, 3152)
KN = ((64, 64), (256, 256), (256, 512), (512, 256))
FAMILIES = ("normal", "offcentre", "sparse_g", "scaled")
TOL = {"y": 3e-5, "dx": 3e-5, "dw": 2e-6, "db": 2e-6}
NAMES = ("y", "dx", "dw", "db")
UNCLEAR, UNCLEAR_SHARE = 1e-4, 0.01
WORST = {}


@pytest.fixture(autouse=True)
def switch_on(monkeypatch):
    """The position under test: the kernels' route (the switch ships off).  -> the value the switch had before, i.e. its default."""
    from unopose_amd import ops

    default = ops.TRAIN_OWN_SMALL_LINEAR
    monkeypatch.setattr(ops, "TRAIN_OWN_SMALL_LINEAR", True)
    return default


def make_case(rows, K, N, family, bias=True):
    """(nn.Linear with its default initialisation, x (rows, K), g (rows, N)) on the CPU, fp32, seeded by the case."""
    seed = 1000003 * FAMILIES.index(family) + rows * 4099 + K * 7 + N
    torch.manual_seed(seed)
    lin = torch.nn.Linear(K, N, bias=bias)
    gen = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(rows, K, generator=gen)
    g = torch.randn(rows, N, generator=gen)
    if family == "offcentre":  # cancellation in dW, a large db
        x = x + 4.0
        g = g + 0.5
    elif family == "sparse_g":  # 90 % of the rows of g are zero
        keep = torch.rand(rows, generator=gen) < 0.1
        g = g * keep[:, None]
    elif family == "scaled":
        x, g = x * 1e3, g * 1e3
    return lin, x, g


def reference(lin, x, g, relu, kernel_y=None):
    """float64 autograd of F.linear (+ relu); with `kernel_y` the ReLU's mask is the kernel's on the unclear elements (module docstring).
    -> (y, dx, dw, db or None), the unclear share, the mask mismatches outside the unclear elements."""
    xd = x.detach().double().requires_grad_(True)
    wd = lin.weight.detach().double().requires_grad_(True)
    bd = None if lin.bias is None else lin.bias.detach().double().requires_grad_(True)
    pre = F.linear(xd, wd, bd)
    share = mismatch = 0.0
    if relu:
        y = torch.relu(pre)
        mask = pre.detach() > 0
        unclear = pre.detach().abs() <= UNCLEAR * pre.detach().abs().max()
        share = unclear.double().mean().item()
        if kernel_y is not None:
            kmask = kernel_y.reshape(mask.shape) > 0
            mismatch = int(((kmask != mask) & ~unclear).sum())
            mask = torch.where(unclear, kmask, mask)
        out = pre * mask
    else:
        y = out = pre
    out.backward(g.double().reshape(out.shape))
    return (y.detach(), xd.grad, wd.grad, None if bd is None else bd.grad), share, mismatch


def own(x, lin, relu, g):
    """ops.linear inside ops.differentiable() on fresh leaves -> (y, dx, dw, db or None); asserts the route."""
    from unopose_amd import ops

    xi = x.detach().requires_grad_(True)
    lin.zero_grad(set_to_none=True)
    with ops.differentiable():
        y = ops.linear(xi, lin, relu=relu)
    assert type(y.grad_fn).__name__ == "_SmallLinearFnBackward", type(y.grad_fn).__name__
    y.backward(g.reshape(y.shape))
    return y.detach(), xi.grad, lin.weight.grad.clone(), None if lin.bias is None else lin.bias.grad.clone()


def compare(label, family, got, ref):
    fails = []
    for name, a, r in zip(NAMES, got, ref):
        if r is None:
            assert a is None
            continue
        assert a.dtype == torch.float32 and a.shape == r.shape and torch.isfinite(a).all(), (label, name)
        scale = r.abs().max().item()
        err = (a.double() - r).abs().max().item() / scale if scale > 0 else float(a.abs().max().item())
        WORST[(family, name)] = max(WORST.get((family, name), 0.0), err)
        print(f"{label} {name}: {err:.2e} of max|ref| {scale:.3e} (bound {TOL[name]:.0e}); worst of {family} so far {WORST[(family, name)]:.2e}")
        if not err <= TOL[name]:
            fails.append((name, err))
    assert not fails, (label, fails)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("K,N", KN)
@pytest.mark.parametrize("rows", ROWS)
def test_values_and_gradients_match_float64(rows, K, N, relu):
    """Every row count around the 64-row tile and the 16-row wave strip, one and many workgroups and row slices, the model's 197 / 1576 /
    3152, the four width pairs; the four input families."""
    for family in FAMILIES:
        lin, x, g = make_case(rows, K, N, family)
        lin, x, g = lin.cuda(), x.cuda(), g.cuda()
        got = own(x, lin, relu, g)
        ref, share, mismatch = reference(lin, x, g, relu, kernel_y=got[0])
        label = f"rows={rows} K={K} N={N} relu={int(relu)} {family}"
        if relu:
            print(f"{label}: unclear share {share:.2e}, mask mismatches outside {mismatch}")
            assert share < UNCLEAR_SHARE, (label, share)
            assert mismatch == 0, (label, mismatch)
        compare(label, family, got, ref)


@pytest.mark.parametrize("shape,N", [((8, 197, 256), 256), ((8, 197, 256), 512), ((16, 197, 512), 256)])
def test_route_small_linears_run_on_the_kernels(shape, N):
    """Fails without the feature: with the switch on and every other switch at its default the 197-token shapes take `_SmallLinearFn`."""
    from unopose_amd import ops

    assert ops.TRAIN_OWN_SMALL_LINEAR is True and ops.TRAIN_OWN_GEMM_MIN_FLOP == 4e9 and ops.TRAIN_OWN_GEMM is True
    torch.manual_seed(0)
    lin = torch.nn.Linear(shape[-1], N).cuda()
    x = torch.randn(*shape, device="cuda", requires_grad=True)
    for relu in (False, True):
        assert ops.small_linear_train_ok(x, lin)
        with ops.differentiable():
            y = ops.linear(x, lin, relu=relu)
        assert type(y.grad_fn).__name__ == "_SmallLinearFnBackward"
        assert y.shape == (*shape[:-1], N) and y.dtype == torch.float32


def test_route_everything_else_as_before(monkeypatch, switch_on):
    """Switch off (the shipped default), bf16 autocast and a 256 -> 1 head: nn.Linear; TRAIN_OWN_GEMM_MIN_FLOP = 0: `_LinearFn` first, as before."""
    from unopose_amd import ops

    assert switch_on is False  # the default that ships (profiles/small_linear_train_ab.txt)
    torch.manual_seed(0)
    lin, head = torch.nn.Linear(256, 256).cuda(), torch.nn.Linear(256, 1).cuda()
    x = torch.randn(8 * 197, 256, device="cuda", requires_grad=True)  # (2-D: nn.Linear on a 3-D input ends in a view)

    def name(layer, relu, amp=False):
        with ops.differentiable(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            return type(ops.linear(x, layer, relu=relu).grad_fn).__name__

    for relu, want in ((False, "AddmmBackward0"), (True, "ReluBackward0")):
        assert name(head, relu) == want
        assert name(lin, relu, amp=True) == want
        monkeypatch.setattr(ops, "TRAIN_OWN_SMALL_LINEAR", False)
        assert not ops.small_linear_train_ok(x, lin)
        assert name(lin, relu) == want
        monkeypatch.setattr(ops, "TRAIN_OWN_SMALL_LINEAR", True)
        assert name(lin, relu) == "_SmallLinearFnBackward"
    monkeypatch.setattr(ops, "TRAIN_OWN_GEMM_MIN_FLOP", 0.0)
    assert name(lin, False) == "_LinearFnBackward" and name(lin, True) == "_LinearFnBackward"


def test_which_gradients_are_asked_for():
    """x without requires_grad: no dx (the weight-gradient launch alone); frozen parameters: dx only (the dx launch alone) -- both with the
    bits of the joint launch that serves the full case; no bias; 3-D input and a strided view give the numbers of their contiguous copies."""
    from torch.profiler import ProfilerActivity, profile

    from unopose_amd import ops

    rows, K, N = 197, 256, 512
    lin, x, g = (t.cuda() for t in make_case(rows, K, N, "normal"))
    full = own(x, lin, True, g)

    lin.zero_grad(set_to_none=True)
    with ops.differentiable():
        y = ops.linear(x, lin, relu=True)  # x is no leaf that asks for a gradient
    assert type(y.grad_fn).__name__ == "_SmallLinearFnBackward"
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        y.backward(g)
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages()]
    assert x.grad is None and any("small_wgrad_kernel" in n for n in names), names
    assert not any("small_linear_dx_kernel" in n or "small_backward_kernel" in n for n in names), names
    assert torch.equal(lin.weight.grad, full[2]) and torch.equal(lin.bias.grad, full[3])

    for p in lin.parameters():
        p.requires_grad_(False)
    lin.zero_grad(set_to_none=True)
    xi = x.detach().requires_grad_(True)
    with ops.differentiable():
        y = ops.linear(xi, lin, relu=True)
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        y.backward(g)
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages()]
    assert any("small_linear_dx_kernel" in n for n in names) and not any("small_wgrad" in n or "small_backward_kernel" in n for n in names), names
    assert lin.weight.grad is None and lin.bias.grad is None and torch.equal(xi.grad, full[1])

    nb, x, g = (t.cuda() for t in make_case(rows, K, N, "normal", bias=False))
    got = own(x, nb, True, g)
    ref, _, mismatch = reference(nb, x, g, True, kernel_y=got[0])
    assert mismatch == 0 and got[3] is None
    compare("no bias", "normal", got, ref)

    lin, x, g = (t.cuda() for t in make_case(4 * 50, K, N, "normal"))
    flat = own(x, lin, True, g)
    cube = own(x.reshape(4, 50, K), lin, True, g)
    assert cube[0].shape == (4, 50, N) and cube[1].shape == (4, 50, K)
    for a, b in zip(flat, cube):
        assert torch.equal(a.reshape(b.shape), b)
    big = torch.zeros(2 * 200, K, device="cuda")
    big[::2] = x
    view = big[::2]
    assert not view.is_contiguous()
    strided = own(view, lin, True, g)
    for a, b in zip(flat, strided):
        assert torch.equal(a, b)


def test_no_stale_state_after_in_place_parameter_edits():
    """`.data` edits bump no version counter: the second run must follow the new parameters all the same."""
    lin, x, g = (t.cuda() for t in make_case(197, 256, 256, "normal"))
    own(x, lin, True, g)
    v = (lin.weight._version, lin.bias._version)
    lin.weight.data.mul_(2)
    lin.bias.data.add_(1)
    assert (lin.weight._version, lin.bias._version) == v
    got = own(x, lin, True, g)
    ref, _, mismatch = reference(lin, x, g, True, kernel_y=got[0])
    assert mismatch == 0
    compare("after the edit", "normal", got, ref)


def test_two_runs_give_equal_bits():
    lin, x, g = (t.cuda() for t in make_case(1576, 256, 512, "normal"))
    a = own(x, lin, True, g)
    b = own(x, lin, True, g)
    for name, s, t in zip(NAMES, a, b):
        assert torch.equal(s, t), name


def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@torch.no_grad()
def test_raw_entry_points_refuse_bad_arguments():
    """Null pointer, rows = 0, rows = 16384, N = 96, K = 576, a workspace one float short: a non-zero return, the NaN-prefilled outputs keep
    their bits, and a valid call afterwards still works (forward, dx, dwdb and the joint backward launch)."""
    from unopose_amd import _lib

    L = _lib.lib()
    rows, N, K = 65, 128, 192
    gen = torch.Generator().manual_seed(3)
    x, w, b, g = (torch.randn(*s, generator=gen).cuda() for s in ((rows, K), (N, K), (N,), (rows, N)))
    n_ws = L.unopose_linear_small_train_ws_floats(rows, N, K)
    assert n_ws > 0
    for bad in ((0, N, K), (16384, N, K), (rows, 96, K), (rows, N, 576), (rows, 0, K), (rows, N, 32)):
        assert L.unopose_linear_small_train_ws_floats(*bad) < 0, bad
    assert L.unopose_linear_small_train_ws_floats(16383, 512, 512) > 0
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")  # noqa: E731
    y, dx, dw, db, ws = nan(rows, N), nan(rows, K), nan(N, K), nan(N), nan(n_ws)
    st = _lib.stream_ptr()

    def fwd(x_=x, w_=w, y_=y, rows_=rows, N_=N, K_=K):
        return L.unopose_linear_small_train_forward(_vp(x_), _vp(w_), _vp(b), rows_, N_, K_, 1, _vp(y_), st)

    def bdx(g_=g, w_=w, dx_=dx, rows_=rows, N_=N, K_=K):
        return L.unopose_linear_small_train_dx(_vp(g_), None, _vp(w_), rows_, N_, K_, _vp(dx_), st)

    def bdw(g_=g, x_=x, ws_=ws, dw_=dw, n_=n_ws, rows_=rows, N_=N, K_=K):
        return L.unopose_linear_small_train_dwdb(_vp(g_), None, _vp(x_), rows_, N_, K_, _vp(ws_), n_, _vp(dw_), _vp(db), st)

    def bwd(g_=g, x_=x, w_=w, ws_=ws, dx_=dx, dw_=dw, n_=n_ws, rows_=rows, N_=N, K_=K):
        return L.unopose_linear_small_train_backward(_vp(g_), None, _vp(x_), _vp(w_), rows_, N_, K_, _vp(ws_), n_, _vp(dx_), _vp(dw_), _vp(db), st)

    for fn, first in ((fwd, "x_"), (bdx, "g_"), (bdw, "g_"), (bwd, "g_")):
        assert fn(**{first: None}) != 0
        for kw in ({"rows_": 0}, {"rows_": 16384}, {"N_": 96}, {"K_": 576}):
            assert fn(**kw) != 0, (fn.__name__, kw)
    assert fwd(w_=None) != 0 and fwd(y_=None) != 0 and bdx(w_=None) != 0 and bdx(dx_=None) != 0
    assert bdw(x_=None) != 0 and bdw(ws_=None) != 0 and bdw(dw_=None) != 0
    assert bwd(x_=None) != 0 and bwd(w_=None) != 0 and bwd(ws_=None) != 0 and bwd(dx_=None) != 0 and bwd(dw_=None) != 0
    assert bdw(n_=n_ws - 1) != 0 and bwd(n_=n_ws - 1) != 0
    assert b"workspace" in L.unopose_last_error()
    torch.cuda.synchronize()
    for name, t in (("y", y), ("dx", dx), ("dw", dw), ("db", db), ("workspace", ws)):
        assert t.isnan().all(), f"a refused call wrote {name}"
    assert fwd() == 0 and bdx() == 0 and bdw() == 0
    torch.cuda.synchronize()
    want = torch.relu(x.double() @ w.double().t() + b.double())
    assert (y.double() - want).abs().max().item() <= 3e-5 * want.abs().max().item()
    for got, ref, tol in ((dx, g.double() @ w.double(), 3e-5), (dw, g.double().t() @ x.double(), 2e-6), (db, g.double().sum(0), 2e-6)):
        assert (got.double() - ref).abs().max().item() <= tol * ref.abs().max().item()
    dx2, dw2, db2 = nan(rows, K), nan(N, K), nan(N)
    assert L.unopose_linear_small_train_backward(_vp(g), None, _vp(x), _vp(w), rows, N, K, _vp(ws), n_ws, _vp(dx2), _vp(dw2), _vp(db2), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(dx2, dx) and torch.equal(dw2, dw) and torch.equal(db2, db)  # the joint launch: the bits of the two single ones


def _model():
    from oracle.unopose_ref import default_cfg, random_state_dict  # weights only
    from unopose_amd.model import UNOPose, default_model_cfg
    from unopose_amd.train import freeze_backbone

    m = UNOPose(default_model_cfg(fine_npoint=512))
    m.load_state_dict(random_state_dict(default_cfg(), seed=0, tame=0.1), strict=True)
    return freeze_backbone(m.cuda())


def test_training_step_runs_the_small_linears_on_the_kernels():
    """One training forward + backward of the small test model under the profiler: the new kernels run; with the switch off they do not."""
    from torch.profiler import ProfilerActivity, profile
    from train_case import make_train_batch

    from unopose_amd import ops
    from unopose_amd.losses import process_loss

    model = _model().train()
    batch, aug = make_train_batch()

    def census():
        ep = {k: v.cuda() for k, v in batch.items()}
        ep["aug_pose"] = (aug[0].cuda(), aug[1].cuda())
        model.zero_grad(set_to_none=True)
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            process_loss(model(ep))["loss"].backward()
            torch.cuda.synchronize()
        return [e.key for e in prof.key_averages()]

    kernels = ("small_linear_fwd_kernel", "small_backward_kernel", "small_wgrad_combine_kernel")  # forward, dX with dW + db, the combine
    old = ops.TRAIN_OWN_SMALL_LINEAR
    try:
        ops.TRAIN_OWN_SMALL_LINEAR = True
        names = census()
        for k in kernels:
            assert any(k in n for n in names), k
        ops.TRAIN_OWN_SMALL_LINEAR = False
        names = census()
        assert not any(k in n for k in kernels for n in names)
    finally:
        ops.TRAIN_OWN_SMALL_LINEAR = old
