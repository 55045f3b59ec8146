"""Time the training-view renderer -- visibility at ssaa x the resolution, shading, texture lookup and the area mean of
render.HipShadedRenderer (csrc/raster_shade.hip) -- in views per second:

    device   640 x 480 output, ssaa 4 (2560 x 1920 samples per view), Phong, a textured ellipsoid of 20480 faces (an icosahedron split five
             times) seen from the 162 views of the hinterstoisser sphere; the wall clock runs around one `render_batch` of all views, chunked
             by the renderer's byte budget, and ends in a device synchronise; --rounds rounds after a warm-up round.  The views stay on the
             device: PNG encoding and the depth render are not in the figure.
    mirror   unopose_amd/shade_host.py (numpy, one core) on the SAME model at 160 x 120 output, ssaa 4 -- 1/16 of the samples -- and --mirror-views
             views, stated with the figure; its bytes must equal the device's at that size before anything is timed

Recorded as measured; no threshold.  Prints one JSON line and writes the lines to --out.

    python scripts/render_train_rate.py [--rounds 5] [--mirror-views 2] [--out profiles/render_train_rate.txt]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--mirror-views", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_train_rate.txt"))
    args = ap.parse_args()

    import numpy as np
    import torch

    from unopose_amd import view_sampler as vs
    from unopose_amd.render import HipShadedRenderer
    from unopose_amd.shade_host import NumpyShadedRenderer

    assert torch.cuda.is_available(), "render_train_rate.py measures on a GPU"
    pts, faces = vs._icosahedron()
    levels = [0] * len(pts)
    for level in range(1, 6):
        faces = vs._split_faces(pts, levels, faces, level)
    unit = np.array(pts)
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    axes = np.array([100.0, 90.0, 80.0])
    verts, faces = unit * axes, np.array(faces, np.int32)
    normals = unit / axes
    uv = np.stack([np.arctan2(unit[:, 1], unit[:, 0]) / (2 * np.pi) + 0.5, np.arcsin(np.clip(unit[:, 2], -1, 1)) / np.pi + 0.5], axis=1)
    texture = np.random.RandomState(1).randint(40, 256, size=(256, 512, 3)).astype(np.uint8)
    views, _ = vs.sample_views(162, 330.0)
    Rs, ts = np.array([v["R"] for v in views]), np.array([v["t"].reshape(3) for v in views])

    def renderer(cls, W, H):
        ren = cls(W, H, shading="phong", ssaa=4)
        ren.add_object(1, verts, faces, normals=normals, texture=texture, texture_uv=uv)
        return ren, [572.4 * W / 640.0, 573.6 * H / 480.0, 325.3 * W / 640.0, 242.0 * H / 480.0]

    w, h, n = 160, 120, args.mirror_views
    mirror, k4 = renderer(NumpyShadedRenderer, w, h)
    pick = np.linspace(0, len(Rs) - 1, n).astype(int)
    t0 = time.perf_counter()
    want = mirror.render_batch(1, Rs[pick], ts[pick], k4)
    secs_mirror = time.perf_counter() - t0
    small, _ = renderer(HipShadedRenderer, w, h)
    assert np.array_equal(small.render_batch(1, Rs[pick], ts[pick], k4).cpu().numpy(), want), "device differs from the mirror"

    W, H = 640, 480
    ren, k4 = renderer(HipShadedRenderer, W, H)
    out = torch.empty(len(Rs), H, W, 3, dtype=torch.uint8, device="cuda")
    secs = []
    for r in range(args.rounds + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ren.render_batch(1, Rs, ts, k4, out=out)
        torch.cuda.synchronize()
        if r:  # round 0 warms up
            secs.append(time.perf_counter() - t0)
    covered = float((out > 0).any(dim=3).float().mean())
    rate = sorted(len(Rs) / s for s in secs)
    rec = dict(faces=int(len(faces)), views=int(len(Rs)), ssaa=4, device=dict(image=[W, H], views_per_s=[round(rate[0], 1), round(rate[-1], 1)], covered=round(covered, 3),
               rounds=args.rounds, views_per_chunk=ren.views_per_chunk()), mirror=dict(image=[w, h], views=n, views_per_s=round(n / secs_mirror, 3)))
    lines = [f"render + resolve of {len(Rs)} views of a textured model of {len(faces)} faces, Phong, ssaa 4",
             f"  device  {W} x {H}: {rate[0]:9.1f} .. {rate[-1]:9.1f} views/s ({1e3 / rate[-1]:.3f} .. {1e3 / rate[0]:.3f} ms per view; {args.rounds} rounds of one batch of {len(Rs)} views"
             f" after a warm-up round, {ren.views_per_chunk()} views per launch under the {ren.chunk_bytes >> 20} MiB key budget, {covered:.0%} of the pixels covered;"
             " views stay on the device, no PNG encoding, no depth render)",
             f"  mirror  {w} x {h}: {n / secs_mirror:9.3f} views/s (numpy, one core, the same model and ssaa, 1/16 of the samples, {n} views; its bytes equal the device's at this size)"]
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
