"""csrc/embed.hip through the C ABI and through ops.geo_embedding against the float64 reference of tests/geo_embed_ref.py: the 3-NN lists
of geo_knn_kernel, the split-operand and plain-bf16 matrix-core kernels, the 4- and 6-point table kernels, the training forward (with its
recorded arg-max) and the table backward's global-atomic branch.  Every output element, the diagonal included, must lie within the bound
derived there; test_geo_embed_ref_cpu.py shows that the mutants a kernel could turn into leave that bound on these cases."""
import copy
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geo_embed_ref as G  # noqa: E402

pytestmark = pytest.mark.gpu

_MODULES, _REFS = {}, {}


def _module(regime, reduction):
    key = (regime, reduction)
    if key not in _MODULES:
        _MODULES[key] = G.make_module(regime, reduction).cuda()
    return _MODULES[key]


def _run(route, out_bf16, pts, m):
    """One entry point of csrc/embed.hip on NaN-filled outputs: (out, knn, amax or None)."""
    from unopose_amd._lib import call, ptr, stream_ptr
    from unopose_amd.ops import geometry as Gm

    B, n, _ = pts.shape
    dev = pts.device
    out = torch.full((B, n, n, 256), float("nan"), dtype=torch.bfloat16 if out_bf16 else torch.float32, device=dev)
    knn = torch.full((B, n, 3), -1, dtype=torch.int32, device=dev)
    bias = (m.proj_d.bias.detach().float() + m.proj_a.bias.detach().float()).contiguous()
    div = m.embedding.div_term.detach().float().contiguous()
    mean = int(m.reduction_a == "mean")
    amax = None
    keep = []
    if route in ("split", "bf16"):
        wdh, wdl = (Gm._mfma_fragment_order(t) for t in Gm._bf16_split(m.proj_d.weight.detach()))
        wah, wal = (Gm._mfma_fragment_order(t) for t in Gm._bf16_split(m.proj_a.weight.detach()))
        keep = [wdh, wdl, wah, wal]
        call("unopose_geo_embedding", ptr(pts), B, n, ptr(wdh), ptr(wdl), ptr(wah), ptr(wal), ptr(bias), ptr(div), float(m.sigma_d),
             float(m.factor_a), mean, int(route == "split"), int(out_bf16), ptr(knn), ptr(out), stream_ptr())
    elif route in ("table4", "table6"):
        npoint = int(route[-1])
        tab = Gm._geo_tables(m, ("test_geo_embedding_gpu",), npoint)
        call("unopose_geo_embedding_table", ptr(pts), B, n, ptr(tab[0]), tab[0].shape[0], ptr(tab[1]), tab[1].shape[0], ptr(bias), ptr(tab[2]),
             ptr(div), 4, npoint, float(m.sigma_d), float(m.factor_a), mean, int(out_bf16), ptr(knn), ptr(out), stream_ptr())
    else:
        assert route == "train" and not out_bf16
        rows_a = int(math.floor(math.pi * float(m.factor_a) * 4)) + 7
        rows_d = 64 * 4 + 6
        td = (Gm._geo_grid(m, rows_d, 6) @ m.proj_d.weight.detach().double().t()).float().contiguous()
        ta = (Gm._geo_grid(m, rows_a, 6) @ m.proj_a.weight.detach().double().t()).float().contiguous()
        wdf = m.proj_d.weight.detach().float().contiguous()
        amax = torch.full((B, n, n, 64), -1, dtype=torch.int32, device=dev)
        keep = [td, ta, wdf]
        call("unopose_geo_embedding_train_forward", ptr(pts), B, n, ptr(td), rows_d, ptr(ta), rows_a, ptr(bias), ptr(wdf), ptr(div), 4,
             float(m.sigma_d), float(m.factor_a), mean, ptr(knn), ptr(out), ptr(amax), stream_ptr())
    torch.cuda.synchronize()
    del keep
    return out, knn, amax


def _reference(key, pts, m, knn):
    """embedding64 for the kernel's (validated) list, computed once per (cloud, weights, list) and left unchanged."""
    hit = _REFS.get(key)
    if hit is None or not torch.equal(hit[0], knn):
        if len(_REFS) > 2:
            _REFS.clear()
        _REFS[key] = hit = (knn.clone(), G.embedding64(pts, m, knn))
    return hit[1]


# ------------------------------------------------------------------------------------------------------------ neighbour lists
@torch.no_grad()
@pytest.mark.parametrize("kind,B,n", G.KNN_CASES, ids=lambda v: str(v))
def test_knn_of_every_entry_point(kind, B, n):
    """geo_knn_kernel as each entry point launches it: self excluded by index, strict <, so the smaller index wins a tie.  Bit-exact with
    knn_exact on the lattice and the duplicated clouds (exact ties) and on the clouds whose gaps test_geo_embed_ref_cpu.py asserts; valid on all."""
    pts = G.make_batch(kind, B, n).cuda()
    m = _module("default", "max")
    lists = [_run(route, False, pts, m)[1] for route in ("split", "table6", "train")]
    assert torch.equal(lists[0], lists[1]) and torch.equal(lists[0], lists[2])
    assert bool(G.knn_valid(pts, lists[0]).all())
    if kind in G.EXACT_KINDS:
        want, _ = G.knn_exact(pts)
        assert torch.equal(lists[0], want), (lists[0] != want).any(-1).nonzero()[:8].tolist()


# ------------------------------------------------------------------------------------------------------------ forward
@torch.no_grad()
@pytest.mark.parametrize("case", sorted(G.CASES, key=lambda c: (c[6], c[5], c[4], c[3], c[2])), ids=lambda c: "-".join(map(str, c)))
def test_forward_routes_vs_float64(case):
    route, out_bf16, reduction, regime, kind, B, n = case
    pts = G.make_batch(kind, B, n).cuda()
    m = _module(regime, reduction)
    out, knn, _ = _run(route, out_bf16, pts, m)
    assert not bool(torch.isnan(out).any()), "rows left unwritten"
    assert bool(G.knn_valid(pts, knn).all())
    ref = _reference((reduction, regime, kind, B, n), pts, m, knn)
    bnd = G.bound(pts, m, knn, "table6" if route == "train" else route, out_bf16, ref=ref)
    err = (out.double() - ref).abs()
    eye = torch.eye(n, dtype=torch.bool, device="cuda")
    print("RATIO %s %s %s B=%d n=%d %s %s worst %.4f diagonal %.4f" % (route, "bf16" if out_bf16 else "fp32", kind, B, n, reduction, regime,
                                                                        float((err / bnd).max()), float((err / bnd)[:, eye].max())))
    assert bool((err <= bnd).all()), (float((err / bnd).max()), float(err.max()))


@torch.no_grad()
def test_training_forward_records_the_first_maximum():
    """dup_heavy: a point's second and third neighbour are copies of each other, so two of the three angle terms are bit-identical, and on the
    diagonal all three are: the recorded arg-max must be the FIRST of equal maxima (where torch.max sends the gradient), and a maximum."""
    B, n = 2, 33
    pts = G.make_batch("dup_heavy", B, n).cuda()
    m = _module("trained", "max")
    out, knn, amax = _run("train", False, pts, m)
    assert bool(G.knn_valid(pts, knn).all())
    am = amax.view(torch.uint8).reshape(B, n, n, 256).long()
    assert int(am.min()) >= 0 and int(am.max()) <= 2
    ref, terms = G.embedding64(pts, m, knn, terms=True)
    bnd = G.bound(pts, m, knn, "table6", ref=ref)
    picked = torch.gather(terms, 3, am.unsqueeze(3)).squeeze(3)
    assert bool((picked >= terms.amax(3) - 2 * bnd).all())
    q = torch.stack([pts[b][knn[b].long()] for b in range(B)])              # (B,n,3 neighbours,3)
    same = lambda a, b: (q[:, :, a] == q[:, :, b]).all(-1)[:, :, None, None]  # noqa: E731  (identical reference vectors: identical terms)
    assert bool(same(1, 2).any())
    assert not bool(((am == 2) & (same(1, 2) | same(0, 2))).any()) and not bool(((am == 1) & same(0, 1)).any())
    eye = torch.eye(n, dtype=torch.bool, device="cuda")
    assert int(am[:, eye].max()) == 0                                        # anchor 0: all three angles are 0


@torch.no_grad()
def test_empty_batch_on_every_route():
    m = _module("default", "max")
    pts = torch.empty(0, 33, 3, device="cuda")
    for route, out_bf16 in G.ROUTES:
        out, knn, _ = _run(route, out_bf16, pts, m)
        assert out.shape == (0, 33, 33, 256) and knn.shape == (0, 33, 3)
    from unopose_amd import ops

    assert ops.geo_embedding(pts, m).shape == (0, 33, 33, 256)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert ops.geo_embedding(pts, m).dtype == torch.bfloat16
    ops.GEO_TABLE = ops.GEO_TABLE_F32 = False
    try:
        assert ops.geo_embedding(pts, m).shape == (0, 33, 33, 256)
    finally:
        ops.GEO_TABLE = ops.GEO_TABLE_F32 = True


# ------------------------------------------------------------------------------------------------------------ the op's routing
@torch.no_grad()
def test_op_routing_follows_autocast_and_the_switches():
    from unopose_amd import ops

    pts = G.make_batch("bg", 2, 65).cuda()
    m = copy.deepcopy(_module("trained", "max"))
    assert torch.equal(ops.geo_embedding(pts, m), _run("table6", False, pts, m)[0])
    with torch.autocast("cuda", dtype=torch.bfloat16):
        got = ops.geo_embedding(pts, m)
    assert got.dtype == torch.bfloat16 and torch.equal(got, _run("table4", True, pts, m)[0])
    ops.GEO_TABLE = ops.GEO_TABLE_F32 = False
    try:
        assert torch.equal(ops.geo_embedding(pts, m), _run("split", False, pts, m)[0])
        with torch.autocast("cuda", dtype=torch.bfloat16):
            got = ops.geo_embedding(pts, m)
        assert got.dtype == torch.bfloat16 and torch.equal(got, _run("bf16", True, pts, m)[0])
    finally:
        ops.GEO_TABLE = ops.GEO_TABLE_F32 = True


@torch.no_grad()
@pytest.mark.parametrize("table", [True, False])
def test_op_routing_follows_an_edit_of_one_bias(table):
    """The cache key of ops.geo_embedding names the version of every parameter: an in-place edit of proj_a.bias alone must show."""
    from unopose_amd import ops

    pts = G.make_batch("random", 2, 33).cuda()
    m = copy.deepcopy(_module("default", "max"))
    ops.GEO_TABLE_F32 = table
    try:
        before = ops.geo_embedding(pts, m)
        m.proj_a.bias.add_(0.375)
        after = ops.geo_embedding(pts, m)
    finally:
        ops.GEO_TABLE_F32 = True
    knn = _run("table6", False, pts, m)[1]
    assert bool(G.knn_valid(pts, knn).all())
    ref = G.embedding64(pts, m, knn)
    assert bool(((after.double() - ref).abs() <= G.bound(pts, m, knn, "table6" if table else "split")).all())
    assert float((after - before - 0.375).abs().max()) < 1e-6


# ------------------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("kind,reduction,B,n", G.BACKWARD_CASES)
def test_backward_global_branch_vs_float64(kind, reduction, B, n):
    """The table backward on clouds that are NOT radius-normalised: distance indices in [16, 60] go through global atomics into `full_d`,
    and the workgroups' shares cut rows and batches.  The four parameter gradients against float64 autograd over the composite, at the
    tolerance of test_geo_embedding_under_autograd_matches_the_composite_in_float64; the forward within the table bound."""
    from unopose_amd import ops

    pts = G.make_batch(kind, B, n).cuda()
    m = copy.deepcopy(_module("default", reduction))
    for p in m.parameters():
        p.grad = None
    x = G.distance_index64(pts, m)
    assert G.D_LDS + 8 < float(x.max()) <= G.MAX_BWD_INDEX     # (past 64 the backward ends in a device assert: never run it there)
    g = torch.Generator().manual_seed(B * 1000 + n)
    dE = torch.randn(B, n, n, 256, generator=g).cuda()
    with ops.differentiable():
        out = ops.geo_embedding(pts, m)
    assert out.grad_fn is not None and "GeoEmbed" in type(out.grad_fn).__name__
    knn = out.grad_fn.saved_tensors[1]
    assert bool(G.knn_valid(pts, knn).all())
    out.backward(dE)
    got = {k: p.grad.clone() for k, p in m.named_parameters()}
    m64 = copy.deepcopy(m).double()
    for p in m64.parameters():
        p.grad = None
    ref = G.composite64(pts.double(), knn.long(), m64, reduction)
    ref.backward(dE.double())
    with torch.no_grad():
        want = G.embedding64(pts, m, knn)
        assert bool(((out.detach().double() - want).abs() <= G.bound(pts, m, knn, "table6")).all())
    for k, p in m64.named_parameters():
        scale = p.grad.abs().max().item()
        err = (got[k].double() - p.grad).abs().max().item()
        fro = ((got[k].double() - p.grad).norm() / p.grad.norm()).item()
        print("BACKWARD %s %s B=%d n=%d %s err/scale %.2e fro %.2e" % (kind, reduction, B, n, k, err / scale, fro))
        assert err < 1e-2 * scale + 1e-6 and fro < 3e-3, (k, err, scale, fro)
