"""Time the pose visualisation of one image -- colour renders of its poses (render.HipColorRenderer, csrc/raster_color.hip) and their
composition with the depth-difference image (ops.compose_poses, csrc/vis.hip) -- in images per second:

    device   640 x 480, --poses poses (three objects of tests/bop_score_case.py in turn, 80 faces each), photo and captured depth already on
             the GPU; the wall clock runs around --images images in a row and ends in a device synchronise, --rounds rounds after a warm-up
             round; `compose_poses` reads the boxes and the statistics back per image, as the command does, so that copy is inside
    mirror   tests/raster_rgb_np.py (numpy, one core) on the same poses at 160 x 120, a SMALLER image, stated with the figure; its
             composition must equal the device's on that size before anything is timed

Recorded as measured; no threshold.  Prints one JSON line and writes the lines to --out.

    python scripts/vis_poses_rate.py [--poses 8] [--images 1000] [--rounds 5] [--out profiles/vis_poses_rate.txt]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--poses", type=int, default=8)
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vis_poses_rate.txt"))
    args = ap.parse_args()

    import numpy as np
    import torch

    import bop_score_case as C
    from bop_eval_case import rot
    from raster_rgb_np import NumpyColorRenderer, compose
    from unopose_amd.ops import compose_poses
    from unopose_amd.render import HipColorRenderer
    from unopose_amd.vis_poses import palette, render_poses

    assert torch.cuda.is_available(), "vis_poses_rate.py measures on a GPU"
    models = C._models()
    pal = palette(models)
    rs = np.random.RandomState(2)
    objs = sorted(models)
    poses = sorted([dict(obj_id=objs[k % len(objs)], R=rot(rs.randn(3), rs.rand() * 3),
                         t=np.array([(k % 4 - 1.5) * 140.0 + rs.uniform(-20, 20), (k // 4 - 0.5) * 160.0 + rs.uniform(-20, 20), rs.uniform(650, 900)]))
                    for k in range(args.poses)], key=lambda p: p["obj_id"])

    def problem(W, H):
        K = C.K_A * np.array([[W / 640.0], [H / 480.0], [1.0]])
        r2 = np.random.RandomState(3)
        return K, r2.randint(0, 256, size=(H, W, 3)).astype(np.uint8), (r2.uniform(600, 1000, size=(H, W)) * (r2.rand(H, W) > 0.03)).astype(np.float32)

    def device_image(ren, K, photo_d, depth_d):
        depths, rgbs = render_poses(ren, poses, K)
        return compose_poses(rgbs, depths, photo_d, depth_d, resolve_visib=True, delta=15.0)

    def renderer(cls, W, H):
        ren = cls(W, H)
        for o, m in models.items():
            ren.add_object(o, m["verts"], m["faces"], surf_color=pal[o])
        return ren

    # the mirror, at its own smaller size, and the equality of the two routes there
    w, h = 160, 120
    K, photo, depth = problem(w, h)
    mirror, small = renderer(NumpyColorRenderer, w, h), renderer(HipColorRenderer, w, h)
    secs_mirror = []
    for _ in range(3):
        t0 = time.perf_counter()
        outs = [mirror.render_object(p["obj_id"], p["R"], p["t"], K[0, 0], K[1, 1], K[0, 2], K[1, 2]) for p in poses]
        want = compose(np.stack([o["rgb"] for o in outs]), np.stack([o["depth"] for o in outs]), photo, depth, True, 15.0)
        secs_mirror.append(time.perf_counter() - t0)
    got = device_image(small, K, torch.from_numpy(photo).cuda(), torch.from_numpy(depth).cuda())
    assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[3].cpu().numpy(), want[3]) and got[1] == want[1], "device differs from the mirror"
    drawn = sum(b is not None for b in want[1])

    W, H = 640, 480
    K, photo, depth = problem(W, H)
    ren = renderer(HipColorRenderer, W, H)
    photo_d, depth_d = torch.from_numpy(photo).cuda(), torch.from_numpy(depth).cuda()
    secs = []
    for r in range(args.rounds + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.images):
            out = device_image(ren, K, photo_d, depth_d)
        torch.cuda.synchronize()
        if r:  # round 0 warms up
            secs.append(time.perf_counter() - t0)
    covered = float((out[2] > 0).float().mean())
    rate = sorted(args.images / s for s in secs)
    rate_m = sorted(1.0 / s for s in secs_mirror)
    rec = dict(poses=args.poses, poses_drawn=drawn, faces_per_object=int(len(models[objs[0]]["faces"])), device=dict(image=[W, H], images_per_s=[round(rate[0], 1), round(rate[-1], 1)],
               ms_per_image=[round(1e3 / rate[-1], 3), round(1e3 / rate[0], 3)], covered=round(covered, 3), rounds=args.rounds, images_per_round=args.images),
               mirror=dict(image=[w, h], images_per_s=[round(rate_m[0], 2), round(rate_m[-1], 2)]))
    lines = [f"render + compose of one image with {args.poses} poses ({drawn} of them in view at the small size), objects of {rec['faces_per_object']} faces, depth-difference image included",
             f"  device  {W} x {H}: {rate[0]:9.1f} .. {rate[-1]:9.1f} images/s ({1e3 / rate[-1]:.3f} .. {1e3 / rate[0]:.3f} ms per image; {args.rounds} rounds of {args.images} images after a warm-up round,"
             f" {covered:.0%} of the pixels covered; per image: one render launch sequence per object, two composition launch sequences, one read-back of boxes and statistics)",
             f"  mirror  {w} x {h}: {rate_m[0]:9.2f} .. {rate_m[-1]:9.2f} images/s (numpy, one core, 1/16 of the pixels; its composition equals the device's at this size)"]
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
