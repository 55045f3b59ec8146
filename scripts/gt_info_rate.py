"""Time the ground-truth visibility (unopose_amd/gt_info.py) on the large synthetic case (tests/bop_score_case.py, 480 x 640) in ground
truths per second through two routes, both on the HIP rasteriser's canvas renders:

    host     `compute_gt_info(...)`            (numpy per ground truth: the canvas map comes to the host)
    device   `compute_gt_info(..., device=)`   (csrc/gtinfo.hip: maps stay on the GPU)

with and without masks.  One warm-up call per route, then --rounds rounds in which the routes run alternately; the wall clock is around the
whole call and the device is synchronised before it is read.  Both routes must return the same dictionaries and masks.  Then the kernel
alone: --repeats launches of `unopose_gt_visibility` over one prepared chunk between two device events, against the bytes a launch
moves -- per ground truth the canvas (3H x 3W x 4 B), 4 B of test depth per silhouette pixel of the image, and with masks 2 B per image
pixel written.  The canvas maps were just written by the rasteriser and a chunk fits the Infinity Cache, so the rate is that of a
resident stream, not of HBM; --cold evicts them with a 512 MB fill before every timed launch.  Prints one JSON line and, with --out, appends
the ranges as text.

    python scripts/gt_info_rate.py [--images 4] [--rounds 3] [--repeats 20] [--out profiles/gt_info_rate.txt]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--images", type=int, default=4, help="images per scene of make_large_case (3 scenes, 3 to 4 ground truths per image)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out")
    args = ap.parse_args()

    import numpy as np
    import torch

    import bop_score_case as C
    from unopose_amd import gt_info
    from unopose_amd._lib import call, ptr, stream_ptr
    from unopose_amd.ops.score import vsd_delta_as_compared
    from unopose_amd.render import HipDepthRenderer

    assert torch.cuda.is_available(), "gt_info_rate.py measures on a GPU"
    models, scene_gt, cameras, _, _, depth_images, (W, H) = C.make_large_case(images_per_scene=args.images)
    ren = HipDepthRenderer(3 * W, 3 * H)
    for oid, m in models.items():
        ren.add_object(oid, m["verts"], m["faces"])
    n_gt = sum(len(g) for ims in scene_gt.values() for g in ims.values())
    a = (scene_gt, cameras, depth_images, ren, 15.0)
    routes = {"host": {}, "device": dict(device="cuda")}

    def run(route, masks):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = gt_info.compute_gt_info(*a, masks=masks, **routes[route])
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    lines, rec = [f"{n_gt} ground truths in {3 * args.images} images of {W} x {H} (canvas {3 * W} x {3 * H}), {args.rounds} alternating rounds after a warm-up call each"], {}
    for masks in (False, True):
        outs = {r: run(r, masks)[1] for r in routes}  # warm-up
        if masks:
            assert outs["device"][0] == outs["host"][0], "device differs from host"
            for sid, ims in outs["host"][1].items():
                for iid, pairs in ims.items():
                    for (m, mv), (dm, dmv) in zip(pairs, outs["device"][1][sid][iid]):
                        assert np.array_equal(m, dm) and np.array_equal(mv, dmv), "device masks differ from host"
        else:
            assert outs["device"] == outs["host"], "device differs from host"
        secs = {r: [] for r in routes}
        for _ in range(args.rounds):
            for r in routes:
                secs[r].append(run(r, masks)[0])
        rate = {r: sorted(n_gt / s for s in v) for r, v in secs.items()}
        key = "with_masks" if masks else "without_masks"
        rec[key] = dict(gt_per_s={r: [round(v[0], 1), round(v[-1], 1)] for r, v in rate.items()},
                        device_over_host=[round(rate["device"][0] / rate["host"][-1], 2), round(rate["device"][-1] / rate["host"][0], 2)])
        lines.append(f"  {'with' if masks else 'without'} masks")
        for r, v in rate.items():
            lines.append(f"    {r:7s} {v[0]:9.1f} .. {v[-1]:9.1f} ground truths/s   ({min(secs[r]):.3f} .. {max(secs[r]):.3f} s per call)")
        lines.append(f"    device / host: {rec[key]['device_over_host'][0]} .. {rec[key]['device_over_host'][1]} x; dictionaries{' and masks' if masks else ''} equal")

    # the kernel alone, on one chunk: the ground truths of the first scene
    sid = next(iter(scene_gt))
    items = gt_info._flat({sid: scene_gt[sid]}, cameras)
    order = list(dict.fromkeys((it[0], it[1]) for it in items))
    test = torch.stack([torch.from_numpy(np.ascontiguousarray(depth_images[s][i], dtype=np.float32)) for s, i in order]).cuda()
    G = len(items)
    canvas = torch.empty(G, 3 * H, 3 * W, dtype=torch.float32, device="cuda")
    for n, it in enumerate(items):
        ren.render_batch(it[3]["obj_id"], it[3]["R"][None], it[3]["t"][None], np.asarray([gt_info._canvas_k4(it[4], W, H)]), out=canvas[n:n + 1])
    index = torch.tensor([[n, order.index((it[0], it[1]))] for n, it in enumerate(items)], dtype=torch.int32).cuda()
    params = torch.tensor([[it[4][0, 0], it[4][1, 1], it[4][0, 2], it[4][1, 2], vsd_delta_as_compared(15.0)] for it in items], dtype=torch.float64).cuda()
    out = torch.empty(G, 11, dtype=torch.int32, device="cuda")
    masks = torch.empty(2, G, H, W, dtype=torch.uint8, device="cuda")
    in_image = int((canvas[:, H:2 * H, W:2 * W] > 0).sum())
    evict = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")

    def kernel(with_masks, cold):
        import ctypes

        null = ctypes.c_void_p(None)
        times = []
        for _ in range(args.repeats + 2):
            if cold:
                evict.fill_(1)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call("unopose_gt_visibility", ptr(canvas), G, ptr(test), int(test.shape[0]), ptr(index), ptr(params), G, H, W, ptr(out),
                 ptr(masks[0]) if with_masks else null, ptr(masks[1]) if with_masks else null, stream_ptr())
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) * 1e-3)
        return sorted(times[2:])  # the first two launches warm up

    lines.append(f"  kernel alone (the init launch included): {G} ground truths per launch, {args.repeats} launches between device events each")
    rec["kernel"] = {}
    for with_masks in (False, True):
        nbytes = G * 9 * H * W * 4 + in_image * 4 + (2 * G * H * W if with_masks else 0)
        for cold in (False, True):
            t = kernel(with_masks, cold)
            med = t[len(t) // 2]
            name = f"{'masks' if with_masks else 'counts'}_{'cold' if cold else 'resident'}"
            rec["kernel"][name] = dict(us_per_launch=[round(t[0] * 1e6, 1), round(med * 1e6, 1), round(t[-1] * 1e6, 1)], us_per_gt=round(med * 1e6 / G, 2),
                                       mbytes=round(nbytes / 1e6, 2), tbytes_per_s=round(nbytes / med / 1e12, 3))
            lines.append(f"    {name:16s} {t[0] * 1e6:8.1f} / {med * 1e6:8.1f} / {t[-1] * 1e6:8.1f} us per launch (min / median / max), {med * 1e6 / G:7.2f} us per ground truth, "
                         f"{nbytes / 1e6:.1f} MB -> {nbytes / med / 1e12:.3f} TB/s")
    rec.update(ground_truths=n_gt, image=[W, H], rounds=args.rounds, kernel_ground_truths=G)
    print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
