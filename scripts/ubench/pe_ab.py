"""Same-box A/B of the bf16x3 positional-encoding path between two TREES (e.g. this one and an export of its parent commit).

    python scripts/ubench/pe_ab.py run TREE OUTDIR     # one fresh process per tree: timings + the arrays of the identity check
    python scripts/ubench/pe_ab.py compare DIR_A DIR_B # torch.equal on every array both runs wrote

`run` imports `unopose_amd` from TREE (its library must be built), times one `ops.pe_group_mlp_max` call per scale at 32 x 2048
(whatever launches that call makes in that tree), the two-scale `PositionalEncoding.groups_split` path and, where the tree has it,
the geometry kernel alone, then writes features, lists and counts on: the bench clouds (B = 32, both scales, fp32 and split output),
`norm_clouds(2048, 3, seed=5)` with duplicated points, and the edge clouds of tests/test_model_gpu.py's grid-query test.
It also writes `ops.query_lrf_group` at (r 0.1, S 64) and (r 0.2, S 256) on all of those clouds, at (r 0.2, S 40) on
`norm_clouds(777, 3, seed=11)`, and one `ops.lrf_group_idx` result on the inputs of tests/test_geom_gpu.py's "other options" test.
The library is TREE's own, or the one UNOPOSE_LIB names (another build of the same ABI under TREE's Python).
"""
import os
import sys

mode = sys.argv[1]
if mode == "compare":
    import torch

    a, b = (torch.load(os.path.join(d, "pe_ab.pt")) for d in sys.argv[2:4])
    bad = 0
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            print(f"{k:44s} only in one run")
            bad += 1
            continue
        x, y = a[k], b[k]
        eq = x.shape == y.shape and x.dtype == y.dtype and torch.equal(x.view(torch.uint8) if x.is_floating_point() else x,
                                                                       y.view(torch.uint8) if y.is_floating_point() else y)
        extra = ""
        if not eq and x.shape == y.shape:
            d = (x.double() - y.double()).abs()
            extra = f"  max|diff| {d.max().item():.3e}  differing {int((d > 0).sum())} of {d.numel()}"
        print(f"{k:44s} {'equal (bitwise)' if eq else 'DIFFERENT'}{extra}")
        bad += not eq
    print("IDENTICAL" if not bad else f"{bad} arrays differ")
    sys.exit(1 if bad else 0)

tree, outdir = os.path.abspath(sys.argv[2]), sys.argv[3]
sys.path.insert(0, tree)
sys.path.insert(0, os.path.join(tree, "tests"))
import torch  # noqa: E402
from test_geom_gpu import norm_clouds  # noqa: E402
from unopose_amd import ops  # noqa: E402
from unopose_amd.model import UNOPose, default_model_cfg  # noqa: E402
from unopose_amd.synthetic import make_batch, trained_like_  # noqa: E402

assert os.path.abspath(ops.__file__).startswith(tree), ops.__file__
torch.set_grad_enabled(False)
torch.manual_seed(0)  # (trained_like_ keeps torch's default init of the conv weights: the same in both processes)
m = trained_like_(UNOPose(default_model_cfg())).cuda().eval()
pe = m.fine_point_matching.PE
batch, _, _ = make_batch(32, device="cuda")
rad = torch.norm(batch["tem1_pts"] - batch["tem1_pts"].mean(1, keepdim=True), dim=2).max(1)[0]
x = (batch["pts"] / (rad.reshape(-1, 1, 1) + 1e-6)).contiguous()  # the bench clouds, 32 x 2048


def timed(f, n=10):
    for _ in range(3):
        f()
    best = 1e30
    for _ in range(3):
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(n):
            f()
        e.record()
        torch.cuda.synchronize()
        best = min(best, s.elapsed_time(e) / n * 1e3)
    return best


out = {}
buf = torch.zeros(32, 2048, 512, dtype=torch.bfloat16, device="cuda")
for name, mlp, r, S in (("wide", pe.mlp2, pe.r2, pe.ns2), ("narrow", pe.mlp1, pe.r1, pe.ns1)):
    f, (l, c) = ops.pe_group_mlp_max(x, r, S, mlp, bf16x3=True, want_cand=True)
    out[f"bench.{name}.feat"], out[f"bench.{name}.lists"], out[f"bench.{name}.counts"] = f, l, c
    print(f"pe_group_mlp_max 32x2048 S={S:3d} r={r}: {timed(lambda: ops.pe_group_mlp_max(x, r, S, mlp, bf16x3=True)):8.1f} us", flush=True)
    if hasattr(ops, "pe_geometry"):
        print(f"  geometry alone (one scale)          : {timed(lambda: ops.pe_geometry(x, r, S)):8.1f} us", flush=True)
        g = ops.pe_geometry(x, r, S)[0]
        print(f"  MLP alone                           : {timed(lambda: ops.pe_mlp_max(x, r, S, mlp, g)):8.1f} us", flush=True)
with torch.autocast("cuda", dtype=torch.bfloat16):
    pe.groups_split(x, buf, 0)
    out["bench.groups_split"] = buf.clone()
    print(f"PE.groups_split 32x2048 (both scales) : {timed(lambda: pe.groups_split(x, buf, 0)):8.1f} us", flush=True)
    out["bench.groups"] = pe.groups(x)
if hasattr(ops, "pe_geometry"):
    print(f"  geometry alone (both scales)        : {timed(lambda: ops.pe_geometry(x, pe.r2, pe.ns2, pe.r1, pe.ns1)):8.1f} us", flush=True)

xd = norm_clouds(2048, 3, seed=5)
xd[1, 1000:1400] = xd[1, :400]
clouds = {"dup": xd}
for kind in ["unit", "wide", "clumped", "flat", "identical", "n256", "n4096"]:
    g = torch.Generator().manual_seed(len(kind))
    N = {"n256": 256, "n4096": 4096}.get(kind, 2048)
    y = torch.rand(2, N, 3, generator=g) * 2 - 1
    if kind == "wide":
        y = y * 7.0
    elif kind == "clumped":
        y[:, : N // 2] = y[:, : N // 2] * 0.05 + 0.3
    elif kind == "flat":
        y[:, :, 2] = 0.25
    elif kind == "identical":
        y[:] = 0.125
    clouds[kind] = y
for kind, y in clouds.items():
    y = y.cuda().contiguous()
    wide = None
    for mlp, r, S in ((pe.mlp2, 0.2, 256), (pe.mlp1, 0.1, 64)):
        f, (l, c) = ops.pe_group_mlp_max(y, r, S, mlp, bf16x3=True, want_cand=True)
        out[f"{kind}.S{S}.feat"], out[f"{kind}.S{S}.lists"], out[f"{kind}.S{S}.counts"] = f, l, c
        if wide is None:
            wide = (l, c)
        else:
            out[f"{kind}.S{S}.feat_from_wide"] = ops.pe_group_mlp_max(y, r, S, mlp, bf16x3=True, cand_in=wide)
# the unfused grouping kernel (training path, `_ext`-level API): its own ball query, and lists handed in
clouds["bench"] = x
for kind, y in clouds.items():
    for r, S in ((0.1, 64), (0.2, 256)):
        out[f"{kind}.query_lrf_group.S{S}"] = ops.query_lrf_group(y.cuda().contiguous(), r, S)
out["n777.query_lrf_group.S40"] = ops.query_lrf_group(norm_clouds(777, 3, seed=11).cuda(), 0.2, 40)
from unopose_amd.pointnet2 import _ext  # noqa: E402

xo = norm_clouds(1024, 2, seed=5, repl_every=9).cuda()
new = (xo + 0.03 * torch.randn(xo.shape, generator=torch.Generator().manual_seed(6)).cuda()).contiguous()
out["shifted.lrf_group_idx.S32"] = ops.lrf_group_idx(xo, new, _ext.ball_query(new, xo, 0.2, 32), 0.2)
torch.cuda.synchronize()
os.makedirs(outdir, exist_ok=True)
torch.save({k: v.cpu() for k, v in out.items()}, os.path.join(outdir, "pe_ab.pt"))
print("wrote", len(out), "arrays to", outdir)
