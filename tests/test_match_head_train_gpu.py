"""GPU: the match head under autograd (ops.match_head on csrc/match_train.hip: InfoNCE + saliency pair + row arg max of one transformer
block from the unit features, no (B, R, C) similarity) against the float64 reference tests/match_head_ref.py.

Error measure: every tensor relative to its own max|ref|, element-wise (EL, plus ATOL for tensors that are ~0) and in the Frobenius norm
(FRO), as tests/test_token_attention_train_gpu.py.  Largest errors measured on the MI355X over the cases below (kernel / fp32 composite =
the switch-off route on the materialised fp32 similarity):
    loss      1.0e-6 (fro 1.0e-6) / 6.9e-7 (6.9e-7)     worst case (1,1,1) early_max
    m1, m2    9.8e-6 (fro 6.3e-6) / 1.1e-6 (8.2e-7)     (1,32,31) random
    da, db    6.3e-5 (fro 3.6e-5) / 9.7e-6 (4.9e-6)     (1,65,15) flat: the rows of G nearly cancel, max|ref| is small
    ds1, ds2  5.8e-6 (fro 5.4e-6) / 1.1e-6 (6.0e-7)     (2,130,257) random
    pred      the reference logit at pred equals the row maximum in every case (0 below it)
BOUNDS holds those maxima times 3-4 (box-to-box MFMA summation order); all stay under the 2e-4 that the 3-product split allows in a
logit (3 * 2^-18 * tau = 1.2e-4 at tau = 10 on unit rows)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import match_head_ref as ref

pytestmark = pytest.mark.gpu

TAU = 10.0
ATOL = 1e-6
BOUNDS = {"loss": (4e-6, 4e-6), "m1": (4e-5, 2.5e-5), "m2": (4e-5, 2.5e-5), "da": (2e-4, 1.4e-4), "db": (2e-4, 1.4e-4),  # name -> (EL, FRO)
          "ds1": (2e-5, 2e-5), "ds2": (2e-5, 2e-5)}
LOGIT_BOUND = 3 * 2.0 ** -18 * TAU
# (B, n1, n2).  The kernels own 64 rows per workgroup (16 per wave; the forward from row 1, the backward from row 0) and stream 32-column
# tiles (two 16-column MFMA tiles): the last four shapes put R - 1, R and C one below / on / above those edges.
SHAPES = [(1, 1, 1), (2, 5, 7), (2, 63, 64), (1, 64, 63), (3, 196, 196), (2, 130, 257), (1, 1030, 515),
          (1, 31, 32), (1, 32, 31), (1, 65, 15), (1, 16, 65)]
FAMILIES = ["random", "peaked", "late_max", "early_max", "flat"]
NAMES = ("loss", "m1", "m2", "da", "db", "ds1", "ds2")


def _labels(g, B, n, hi):
    """(B, n) in [0, hi]: >= a third background, the values 0 and hi present, duplicates."""
    lab = torch.randint(0, hi + 1, (B, n), generator=g)
    lab[torch.rand(B, n, generator=g) < 0.4] = 0
    lab[:, 0] = 0
    if n >= 2:
        lab[:, -1] = hi
    if n >= 4:
        lab[:, 1] = hi
        lab[:, 2] = lab[:, 3]
    return lab


def _features(g, B, n1, n2, family):
    R, C = n1 + 1, n2 + 1
    a = F.normalize(torch.randn(B, R, 256, generator=g), dim=2)
    b = F.normalize(torch.randn(B, C, 256, generator=g), dim=2)
    if family == "flat":
        u = F.normalize(torch.randn(256, generator=g), dim=0)
        return u.expand(B, R, 256).contiguous(), u.expand(B, C, 256).contiguous()
    if family == "random":
        return a, b
    for bi in range(B):
        if family == "peaked":
            k = max(min(R, C) // 2, 1)
            rows, cols = torch.randperm(R, generator=g)[:k], torch.randperm(C, generator=g)[:k]
        else:  # partners inside the last / first 32-row tile of either side: the online rescale fires at the end / never
            wr, wc = min(32, R), min(32, C)
            k = max(min(wr, wc) // 2, 1)
            rows, cols = torch.randperm(wr, generator=g)[:k], torch.randperm(wc, generator=g)[:k]
            if family == "late_max":
                rows, cols = R - 1 - rows, C - 1 - cols
        b[bi, cols] = F.normalize(a[bi, rows] + 0.02 * torch.randn(k, 256, generator=g), dim=1)
    return a, b


@functools.lru_cache(maxsize=None)
def _case(B, n1, n2, family, all_background=False):
    """Inputs (fp32, cuda), upstream gradients and the float64 reference, computed once per case."""
    g = torch.Generator().manual_seed(1000 * n1 + 10 * n2 + FAMILIES.index(family))
    a, b = _features(g, B, n1, n2, family)
    s1, s2 = torch.randn(B, n1, 1, generator=g), torch.randn(B, n2, 1, generator=g)
    l1, l2 = _labels(g, B, n1, n2), _labels(g, B, n2, n1)
    if all_background:
        l1, l2 = torch.zeros_like(l1), torch.zeros_like(l2)
    gs = [torch.randn(B, generator=g), torch.randn(B, n1, 1, generator=g), torch.randn(B, n2, 1, generator=g)]
    dev = torch.device("cuda")
    a, b, s1, s2, l1, l2 = (t.to(dev) for t in (a, b, s1, s2, l1, l2))
    gs = [t.to(dev) for t in gs]
    r = ref.reference(a, b, s1, s2, l1, l2, TAU, *gs)
    return (a, b, s1, s2, l1, l2), gs, r


def _leaves(inputs, grads=(True, True, True, True)):
    return [t.clone().requires_grad_(rg) for t, rg in zip(inputs[:4], grads)]


def _run(fn, inputs, gs, grads=(True, True, True, True), leaves=None):
    """fn(a, b, s1, s2, l1, l2) -> (loss, m1, m2, pred); -> dict of the outputs and the gradients of the leaves that ask for one."""
    l1, l2 = inputs[4:]
    leaves = _leaves(inputs, grads) if leaves is None else leaves
    loss, m1, m2, pred = fn(*leaves, l1, l2)
    out = dict(loss=loss.detach(), m1=m1.detach().flatten(1), m2=m2.detach().flatten(1), pred=pred)
    if any(grads):
        ((loss * gs[0]).sum() + (m1 * gs[1]).sum() + (m2 * gs[2]).sum()).backward()
    for name, leaf in zip(("da", "db", "ds1", "ds2"), leaves):
        out[name] = None if leaf.grad is None else leaf.grad.flatten(1) if name.startswith("ds") else leaf.grad
    return out


def _kernel(a, b, s1, s2, l1, l2):
    from unopose_amd import ops

    return ops.match_head(a, b, s1, s2, l1, l2, TAU, True)


def _composite(a, b, s1, s2, l1, l2):
    """The route with the switch off: the fp32 similarity, ops.infonce_two_way, ops.saliency_pair, max(2)[1]."""
    from unopose_amd import ops

    S = (a @ b.transpose(1, 2)) * TAU
    m1, m2 = ops.saliency_pair(S, s1, s2)
    return ops.infonce_two_way(S, l1, l2), m1, m2, S[:, 1:, :].max(2)[1]


def _errs(got, want):
    scale = want.abs().max().item()
    e = (got.double() - want).abs().max().item()
    fro = (got.double() - want).norm().item() / max(want.norm().item(), 1e-300)
    return e, scale, fro


def _check(label, got, r, comp=None):
    for name in NAMES:
        want = r[name].flatten(1) if name.startswith("ds") else r[name]
        g = got[name]
        assert torch.isfinite(g).all(), (label, name)
        e, scale, fro = _errs(g, want)
        line = f"{label} {name}: kernel {e / max(scale, 1e-300):.2e} (fro {fro:.2e})"
        if comp is not None:
            ec, _, froc = _errs(comp[name], want)
            line += f", fp32 composite {ec / max(scale, 1e-300):.2e} (fro {froc:.2e})"
        print(line)
        EL, FRO = BOUNDS[name]
        assert e <= EL * scale + ATOL, (label, name, e, scale)
        if want.norm().item() > 1e3 * ATOL:
            assert fro <= FRO, (label, name, fro)
    # the arg max by value: any index whose reference logit is within the logit bound of the row maximum
    S = r["S"][:, 1:, :]
    pred = got["pred"]
    assert pred.dtype == torch.int64 and pred.shape == S.shape[:2] and (pred >= 0).all() and (pred < S.shape[2]).all(), label
    at = torch.gather(S, 2, pred.unsqueeze(2)).squeeze(2)
    short = (S.max(2)[0] - at).max().item()
    print(f"{label} pred: reference logit at pred below the row maximum by at most {short:.2e}")
    assert short <= LOGIT_BOUND, (label, short)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("B,n1,n2", SHAPES)
def test_values_and_gradients_match_float64(B, n1, n2, family):
    inputs, gs, r = _case(B, n1, n2, family)
    _check(f"({B},{n1},{n2}) {family}", _run(_kernel, inputs, gs), r, _run(_composite, inputs, gs))


def test_every_label_background():
    inputs, gs, r = _case(2, 130, 257, "peaked", True)
    assert (inputs[4] == 0).all() and (inputs[5] == 0).all()
    _check("(2,130,257) peaked, labels all 0", _run(_kernel, inputs, gs), r, _run(_composite, inputs, gs))


def test_two_runs_give_equal_bits():
    inputs, gs, _ = _case(2, 130, 257, "peaked")
    x, y = _run(_kernel, inputs, gs), _run(_kernel, inputs, gs)
    for name in NAMES + ("pred",):
        assert torch.equal(x[name], y[name]), name


def test_partial_gradients_and_no_backward_without_any():
    from torch.profiler import ProfilerActivity, profile

    inputs, gs, _ = _case(2, 130, 257, "peaked")
    full = _run(_kernel, inputs, gs)
    part = _run(_kernel, inputs, gs, grads=(True, True, False, False))
    assert part["ds1"] is None and part["ds2"] is None
    assert torch.equal(part["da"], full["da"]) and torch.equal(part["db"], full["db"])
    only_b = _run(_kernel, inputs, gs, grads=(False, True, False, False))
    assert only_b["da"] is None and torch.equal(only_b["db"], full["db"])
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        a, b, s1, s2, l1, l2 = inputs
        loss, m1, m2, _ = _kernel(a, b, s1, s2, l1, l2)
        torch.cuda.synchronize()
    assert not loss.requires_grad and not m1.requires_grad and not m2.requires_grad
    names = [e.key for e in prof.key_averages()]
    assert any("match_fwd_kernel" in n for n in names) and not any("match_bwd_kernel" in n for n in names), names


def _peak_rise(fn, inputs, gs):
    leaves = _leaves(inputs)  # (the leaves exist before the call: its own allocations are what is measured)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = _run(fn, inputs, gs, leaves=leaves)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    del out
    return rise


def test_no_similarity_sized_tensor_is_allocated():
    """Forward + backward at (2, 4096, 4096) raise the allocator's peak by less than half of one (B, R, C) fp32 matrix; the composite by
    more than one."""
    B, n = 2, 4096
    g = torch.Generator().manual_seed(3)
    dev = torch.device("cuda")
    a = F.normalize(torch.randn(B, n + 1, 256, generator=g), dim=2).to(dev)
    b = F.normalize(torch.randn(B, n + 1, 256, generator=g), dim=2).to(dev)
    s1, s2 = torch.randn(B, n, 1, generator=g).to(dev), torch.randn(B, n, 1, generator=g).to(dev)
    l1, l2 = _labels(g, B, n, n).to(dev), _labels(g, B, n, n).to(dev)
    gs = [torch.randn(B, generator=g).to(dev), torch.randn(B, n, 1, generator=g).to(dev), torch.randn(B, n, 1, generator=g).to(dev)]
    inputs = (a, b, s1, s2, l1, l2)
    matrix = B * (n + 1) * (n + 1) * 4
    own = _peak_rise(_kernel, inputs, gs)
    comp = _peak_rise(_composite, inputs, gs)
    print(f"peak rise over the call: kernels {own / 2**20:.1f} MiB, composite {comp / 2**20:.1f} MiB, one matrix {matrix / 2**20:.1f} MiB")
    assert own < matrix / 2, (own, matrix)
    assert comp > matrix, (comp, matrix)


def test_training_step_routes_the_match_heads_through_the_kernels():
    """A training forward + backward of the small model: with ops.TRAIN_OWN_MATCH the sweeps run and neither a bmm over an (R x C) matrix
    nor an InfoNCE / saliency kernel does; with the switch off they come back."""
    from oracle.unopose_ref import default_cfg, random_state_dict  # weights only
    from torch.profiler import ProfilerActivity, profile
    from train_case import make_train_batch

    from unopose_amd import ops
    from unopose_amd.losses import process_loss
    from unopose_amd.model import UNOPose, default_model_cfg
    from unopose_amd.train import freeze_backbone

    model = UNOPose(default_model_cfg(fine_npoint=512))
    model.load_state_dict(random_state_dict(default_cfg(), seed=0, tame=0.1), strict=True)
    model = freeze_backbone(model.cuda()).train()
    batch, aug = make_train_batch()
    sims = {(197, 197), (513, 513)}  # (R, C) of the coarse and the fine matcher

    def step():
        ep = {k: v.cuda() for k, v in batch.items()}
        ep["aug_pose"] = (aug[0].cuda(), aug[1].cuda())
        model.zero_grad(set_to_none=True)
        process_loss(model(ep))["loss"].backward()
        torch.cuda.synchronize()
        return ep

    def observe():
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA], record_shapes=True) as prof:
            step()
        names = [e.key for e in prof.key_averages()]
        big = 0
        for e in prof.key_averages(group_by_input_shape=True):
            if e.key == "aten::bmm" and len(e.input_shapes) >= 2 and len(e.input_shapes[0]) == 3 and len(e.input_shapes[1]) == 3:
                x, y = e.input_shapes[0], e.input_shapes[1]
                if {(x[1], x[2]), (y[1], y[2]), (x[1], y[2])} & sims:
                    big += 1
        old = sorted({n for n in names if "infonce" in n.lower() or "saliency" in n.lower()})
        return names, big, old

    default = ops.TRAIN_OWN_MATCH
    try:
        ops.TRAIN_OWN_MATCH = True
        step()  # caches
        names, big, old = observe()
        for k in ("match_split_kernel", "match_fwd_kernel", "match_bwd_kernel"):
            assert any(k in n for n in names), k
        assert big == 0 and old == [], (big, old)
        ops.TRAIN_OWN_MATCH = False
        names, big, old = observe()
    finally:
        ops.TRAIN_OWN_MATCH = default
    assert not any("match_fwd_kernel" in n for n in names)
    assert big >= 1 and len(old) >= 2, (big, old)
