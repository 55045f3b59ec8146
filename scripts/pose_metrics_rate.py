"""Time the further error types (`ad,AUCad,rete,proj,projS`) on the large synthetic case (tests/bop_score_case.py) in (estimate, ground
truth) pairs per second through this tree's two routes:

    host     `average_recall(..., error_types=...)`            (numpy per pair; ADI a chunked brute force) -- the specification
    device   `average_recall(..., error_types=..., device=)`   (csrc/posemetrics.hip)

The models' `pts` are replaced by denser point sets on the same surfaces (--points, sampled on the triangles), the size that rules the
cost of ADI.  One warm-up call per route, then --rounds rounds in which the routes run alternately; the wall clock is around the whole
call with the device synchronised on both sides.  Both routes must return the same recall tables.  --images: images per scene of the
case for each point count (fewer where the host's n^2 loop would take minutes per call).  Where scipy is present the toolkit-style
KD-tree `adi` is timed on the same ADI pairs as a second witness.  Prints one JSON line per size and, with --out, appends the table.

    python scripts/pose_metrics_rate.py [--points 600,5000,20000] [--images 10,3,1] [--rounds 3] [--out profiles/pose_metrics_ab.txt]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
TYPES = "ad,AUCad,rete,proj,projS"


def sample_surface(verts, faces, n, rs):
    """n points on the triangles of a mesh, by area."""
    import numpy as np

    a, b, c = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    f = rs.choice(len(faces), size=n, p=area / area.sum())
    u, v = rs.rand(n, 1), rs.rand(n, 1)
    flip = (u + v) > 1.0
    u, v = np.where(flip, 1.0 - u, u), np.where(flip, 1.0 - v, v)
    return a[f] + u * (b[f] - a[f]) + v * (c[f] - a[f])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--points", default="600,5000,20000")
    ap.add_argument("--images", default="10,3,1", help="images per scene of the case, one value per point count")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--n-top", type=int, default=-1)
    ap.add_argument("--device-only", action="store_true", help="skip the host route (for a kernel trace)")
    ap.add_argument("--out")
    args = ap.parse_args()

    import numpy as np
    import torch

    import bop_score_case as C
    from unopose_amd import bop_eval

    lines = []
    for n_pts, images in zip((int(v) for v in args.points.split(",")), (int(v) for v in args.images.split(","))):
        models, scene_gt, cameras, results, im_width = C.make_large_case(images_per_scene=images)[:5]
        rs = np.random.RandomState(n_pts)
        models = {o: dict(m, pts=sample_surface(m["verts"], m["faces"], n_pts, rs)) for o, m in models.items()}
        walk = list(bop_eval._walk(results, scene_gt, cameras, args.n_top, None))
        pairs = bop_eval.metric_pairs(walk, models, bop_eval.parse_error_types(TYPES), set(bop_eval.default_symmetric_obj_ids(models)))
        n_adi = sum("adi" in p["bases"] for p in pairs)
        routes = {"host": {}, "device": dict(device="cuda")}
        if args.device_only:
            del routes["host"]

        def run(route):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = bop_eval.average_recall(results, scene_gt, models, cameras, im_width, n_top=args.n_top, error_types=TYPES, **routes[route])
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out

        outs = {r: run(r)[1] for r in routes}  # warm-up
        for r in routes:
            assert all(outs[r]["errors"][T]["recalls"] == outs["device"]["errors"][T]["recalls"] for T in outs[r]["errors"]), f"{r} differs from device"
        secs = {r: [] for r in routes}
        for _ in range(args.rounds):
            for r in routes:
                secs[r].append(run(r)[0])
        rate = {r: sorted(len(pairs) / s for s in v) for r, v in secs.items()}
        rec = dict(points=n_pts, images_per_scene=images, estimates=len(results), pairs=len(pairs), adi_pairs=n_adi, rounds=args.rounds, types=TYPES,
                   recalls_ad=outs["device"]["errors"]["ad"]["recalls"], pairs_per_s={r: [round(v[0], 1), round(v[-1], 1)] for r, v in rate.items()},
                   seconds={r: [round(min(v), 4), round(max(v), 4)] for r, v in secs.items()})
        lines.append(f"{n_pts} points per model, {len(results)} estimates, {len(pairs)} pairs of which {n_adi} need ADI ({images} images per scene), "
                     f"{TYPES}, {args.rounds} alternating rounds after a warm-up call each")
        for r, v in rate.items():
            lines.append(f"    {r:7s} {v[0]:10.1f} .. {v[-1]:10.1f} pairs/s   ({min(secs[r]):.4f} .. {max(secs[r]):.4f} s per call)")
        if "host" in rate:
            rec.update(device_over_host=[round(rate["device"][0] / rate["host"][-1], 2), round(rate["device"][-1] / rate["host"][0], 2)],
                       ranges_apart=rate["device"][0] > rate["host"][-1])
            lines.append(f"    device / host: {rec['device_over_host'][0]} .. {rec['device_over_host'][1]} x; ranges "
                         f"{'apart' if rec['ranges_apart'] else 'OVERLAP'}; recall tables equal on both routes")
        try:
            from scipy import spatial
        except ImportError:
            spatial = None
        if spatial is not None and n_adi:
            t0 = time.perf_counter()
            for p in pairs:
                if "adi" in p["bases"]:
                    pts = models[p["obj_id"]]["pts"]
                    spatial.cKDTree(pts @ p["r"]["R"].T + p["r"]["t"]).query(pts @ p["g"]["R"].T + p["g"]["t"], k=1)[0].mean()
            kd = (time.perf_counter() - t0) / n_adi
            rec.update(kdtree_adi_ms_per_pair=round(1e3 * kd, 3))
            lines.append(f"    toolkit-style cKDTree adi alone: {1e3 * kd:.3f} ms per pair, one pass over the {n_adi} ADI pairs")
        print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
