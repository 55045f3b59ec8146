"""Output bytes of the kernels whose wave reductions moved onto common.h's wave_all / block_sum_256, between two LIBRARIES.

    python scripts/ubench/wave_reduce_ab.py run OUTDIR      # one fresh process per library: this tree's, or the one UNOPOSE_LIB names
    python scripts/ubench/wave_reduce_ab.py compare DIR_A DIR_B

`run` feeds seeded inputs to: `ops.cloud_radius` (B = 3, N in {1, 63, 257, 2048}); `ops.pose_score` at the same sizes; BatchNorm + ReLU
forward and backward at (B, C, L) = (2, 3, 70) and (2, 3, 16389) -- L is no multiple of 4 there, so `ops.bn_relu` takes its torch route
and no kernel of the library runs -- and at the nearest sizes the kernels accept, (2, 3, 72) and (2, 3, 16392) (two chunks, the last one
eight elements long); BatchNorm + ReLU + max-pool at (2, 3, 5, 32); `ops.vsd_counts` on the pairs of bop_eval_case.make_vsd_case and
bop_score_case.make_large_case; `ops.gt_visibility` on gt_info_case's scenes at the sizes of tests/test_gt_info_gpu.py and on its random
maps; `ops.ref_select` on the cases of tests/test_ref_targets_gpu.py; the hand-made chunk of online_pairs_case through
`OnlinePairs.chunk_device` (radius, points, indices).  `compare` wants every array byte-equal.
"""
import os
import sys

mode = sys.argv[1]
if mode == "compare":
    import torch

    a, b = (torch.load(os.path.join(d, "wave_reduce_ab.pt")) for d in sys.argv[2:4])
    bad = 0
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            print(f"{k:52s} only in one run")
            bad += 1
            continue
        x, y = a[k], b[k]
        eq = x.shape == y.shape and x.dtype == y.dtype and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))
        print(f"{k:52s} {tuple(x.shape)} {'equal (bitwise)' if eq else 'DIFFERENT'}")
        bad += not eq
    print("IDENTICAL" if not bad else f"{bad} arrays differ")
    sys.exit(1 if bad else 0)

outdir = sys.argv[2]
tree = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, tree)
sys.path.insert(0, os.path.join(tree, "tests"))
import tempfile  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

from unopose_amd import _lib, bop_eval, ops, ref_targets  # noqa: E402

print("library:", _lib.SO_PATH, flush=True)
out = {}


def keep(name, v):
    out[name] = (torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v.detach().cpu()).reshape(-1).clone()


gen = torch.Generator().manual_seed(3)
for N in (1, 63, 257, 2048):
    pts = (torch.randn(3, N, 3, generator=gen) * 0.3 + 0.7).cuda()
    dis, w = torch.rand(3, N, generator=gen).cuda(), torch.rand(3, N, generator=gen).cuda()
    with torch.no_grad():  # (the two take their kernels only where autograd is not recording)
        keep(f"cloud_radius.N{N}", ops.cloud_radius(pts))
        keep(f"pose_score.N{N}", ops.pose_score(dis, w, 0.4))

for shape, pool in (((2, 3, 70, 1), False), ((2, 3, 16389, 1), False), ((2, 3, 72, 1), False), ((2, 3, 16392, 1), False), ((2, 3, 5, 32), True)):
    bn = torch.nn.BatchNorm2d(shape[1]).cuda().train()
    with torch.no_grad():
        bn.weight.copy_(torch.tensor([0.7, -1.3, 1.1]))
        bn.bias.copy_(torch.tensor([0.2, 0.1, -0.4]))
    x = (torch.randn(*shape, generator=gen) * 2.0 + 5.0).cuda().requires_grad_(True)
    y = (ops.bn_relu_maxpool if pool else ops.bn_relu)(x, bn)
    y.backward(torch.randn(*y.shape, generator=gen).cuda())
    tag = "bn_relu" + ("_maxpool." if pool else ".") + "x".join(map(str, shape))
    for name, v in (("y", y), ("dx", x.grad), ("dgamma", bn.weight.grad), ("dbeta", bn.bias.grad), ("running_mean", bn.running_mean), ("running_var", bn.running_var)):
        keep(f"{tag}.{name}", v)

# ---- vsd_counts: every scored pair of the two cases, object by object (tests/test_bop_score_gpu.py's launch)
import bop_score_case  # noqa: E402
from bop_eval_case import make_vsd_case  # noqa: E402
from test_bop_score_gpu import _pairs, _renderer  # noqa: E402

for which, case in (("vsd_case", make_vsd_case()), ("large", bop_score_case.make_large_case())):
    models, depth_images = case[0], case[5]
    ren, pairs = _renderer(case), _pairs(case)
    images = list(dict.fromkeys((p[2], p[3]) for p in pairs))
    test = torch.from_numpy(np.stack([depth_images[s][i] for s, i in images])).cuda()
    for obj_id in models:
        sel = [k for k, p in enumerate(pairs) if p[5] == obj_id]
        K4 = np.asarray([[p[4][0, 0], p[4][1, 1], p[4][0, 2], p[4][1, 2]] for p in (pairs[k] for k in sel)])
        d_est = ren.render_batch(obj_id, np.stack([pairs[k][0]["R"] for k in sel]), np.stack([pairs[k][0]["t"] for k in sel]), K4)
        d_gt = ren.render_batch(obj_id, np.stack([pairs[k][1]["R"] for k in sel]), np.stack([pairs[k][1]["t"] for k in sel]), K4)
        keep(f"vsd_counts.{which}.obj{obj_id}", ops.vsd_counts(test, d_gt, d_est, K4, 15.0, models[obj_id]["diameter"], bop_eval.VSD_TAUS,
                                                              image_index=[images.index((pairs[k][2], pairs[k][3])) for k in sel]))
rs = np.random.RandomState(0)
maps = (rs.uniform(300, 420, size=(3, 2, 37, 51)) * (rs.rand(3, 2, 37, 51) < 0.7)).astype(np.float32)  # 37 x 51: the scalar loop
t, g, e = (torch.from_numpy(m).cuda() for m in maps)
keep("vsd_counts.scalar_loads", ops.vsd_counts(t, g, e, [60.0, 61.0, 25.2, 18.1], 15.0, 100.0, bop_eval.VSD_TAUS))

# ---- gt_visibility
import gt_info_case  # noqa: E402
from test_gt_info_gpu import SIZES, _scene_launch  # noqa: E402

for H, W in SIZES + [(480, 640)]:
    test, canvas, image_index, K4 = _scene_launch(W, H, **({"images": [(1, 1)]} if H == 480 else {}))
    got = ops.gt_visibility(torch.from_numpy(test).cuda(), torch.from_numpy(canvas).cuda(), K4, gt_info_case.DELTA, image_index=image_index, masks=True)
    for name, v in zip(("ints", "mask", "mask_visib"), got):
        keep(f"gt_visibility.scenes.{H}x{W}.{name}", v)
    if H == 480:
        continue
    rs = np.random.RandomState(H * 100 + W)
    canvas = np.where(rs.rand(5, 3 * H, 3 * W) < 0.45, rs.uniform(600, 900, (5, 3 * H, 3 * W)), 0.0).astype(np.float32)
    test = np.where(rs.rand(2, H, W) < 0.2, 0.0, rs.uniform(600, 900, (2, H, W))).astype(np.float32)
    K4 = np.stack([[30.0 + k, 31.0, W / 2.0 - 0.3 * k, H / 2.0 + 0.1] for k in range(5)])
    got = ops.gt_visibility(torch.from_numpy(test).cuda(), torch.from_numpy(canvas).cuda(), K4, [15.0, 5.0, 15.0, 0.0, 40.0], image_index=rs.randint(0, 2, 5), masks=True)
    for name, v in zip(("ints", "mask", "mask_visib"), got):
        keep(f"gt_visibility.random.{H}x{W}.{name}", v)

# ---- ref_select (ref_finish_kernel: the count sum left the (nearest, preferred) exchange loop)
import ref_targets_case  # noqa: E402

for seed, Q, C, S, slab in ((11, 1, 1, 1, None), (11, 70, 257, 1, None), (11, 70, 257, 2, None), (11, 33, 130, 315, None), (11, 70, 257, 2, 5), (13, 9, 150, 1, 1),
                            (12, 5, 22, 2, 7), (12, 3, 9, 315, 2)):
    case = ref_targets_case.make_case(seed, Q, C, S)
    for max_rot in (20.0, 50.0):
        got = ops.ref_select(case["Rq"], case["q_scene"], case["q_key"], case["Rc"], case["c_scene"], case["c_key"], case["syms"],
                             ref_targets.trace_min_of(max_rot), 0, True, "cuda", slab=slab)
        for name, v in zip(("pick", "n_eligible", "nearest", "nearest_trace"), got):
            keep(f"ref_select.{seed}.{Q}x{C}x{S}.slab{slab}.rot{max_rot:g}.{name}", v)

# ---- items_points_kernel: the hand-made chunk of the online pairs
import online_pairs_case  # noqa: E402
import render_train_case  # noqa: E402
from unopose_amd.provider_online import OnlinePairs  # noqa: E402

with tempfile.TemporaryDirectory() as tmp:
    src = OnlinePairs(os.path.join(render_train_case.write_dataset(tmp), "models"), dict(online_pairs_case.CFG), "cuda", 5, augment=False)
    views, recipe = online_pairs_case.chunk()
    up = lambda *names: torch.from_numpy(np.concatenate([views[n] for n in names])).cuda()  # noqa: E731
    res = src.chunk_device(recipe, (up("q_rgb", "ref_rgb"), up("q_depth", "ref_depth"), up("occ_rgb"), up("occ_depth")))
    keep("items.radius", res["radius"])
    keep("items.valid", np.asarray(res["valid"]).astype(np.uint8))
    for k in np.flatnonzero(res["valid"]):
        for key in ("pts", "rgb_choose", "tem1_pts", "tem1_choose"):
            keep(f"items.{online_pairs_case.NAMES[k]}.{key}", res[key][k])

torch.cuda.synchronize()
os.makedirs(outdir, exist_ok=True)
torch.save(out, os.path.join(outdir, "wave_reduce_ab.pt"))
print("wrote", len(out), "arrays to", outdir)
