"""Time the symmetry kernel (csrc/symmetry.hip, `ops.sym_deviation`) and the search built on it (`model_sym.find_symmetries`):

    kernel        `unopose_sym_deviation` with bound^2 = inf (no early exit) on a box surface lattice of 14594 vertices -- the size of a
                  models_eval mesh -- for 64 and for 4096 candidate rotations, over prepared buffers, between device events: (candidate,
                  point, point) triples per second;
    search        `find_symmetries(device="cuda")` on the same vertices with the defaults (1024 axes, orders 2 .. 6, tol 0.02: early exit
                  on), wall clock per object: uploads, every call of the coarse pass, the refinement, the sweep and the closure -- the
                  best case, since the lattice's true axes are among the exact candidates and need no refinement -- and on the same vertices
                  with noise, where nothing is exact and every survivor is refined to the smallest step;
    host          the host route beside it at the shapes it finishes in: `sym_deviation_host` on 2048 of the vertices for 16 candidates
                  without a bound, and the whole search on the 230-vertex box of the tests, there on both routes.
The shapes differ between the device and the host lines, so no ratio between them is formed.  Prints one JSON line and, with --out, appends the
lines as text.

    python scripts/model_sym_rate.py [--repeats 5] [--out profiles/model_sym_rate.txt]"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def lattice(sx, sy, sz, grid):
    import numpy as np

    ax = [np.arange(-s / 2.0, s / 2.0 + 1e-9, grid) for s in (sx, sy, sz)]
    g = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3)
    return g[(np.abs(np.abs(g) - np.array([sx, sy, sz]) / 2.0) < 1e-9).any(axis=1)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()

    import numpy as np
    import torch

    from unopose_amd import model_sym
    from unopose_amd._lib import call, ptr, stream_ptr
    from unopose_amd.ops.score import sym_deviation_sizes

    assert torch.cuda.is_available(), "model_sym_rate.py measures on a GPU"
    rs = np.random.RandomState(3)
    pts = lattice(40.0, 60.0, 90.0, 1.25)
    n = len(pts)
    tile, per_launch = sym_deviation_sizes()
    lines, rec = [f"symmetry kernel: query tiles of {tile} points, {per_launch} candidates per launch; {args.repeats} launches between device events after a warm-up; "
                  f"box 40 x 60 x 90 surface lattice, {n} vertices"], {}

    def events(fn):
        times = []
        for _ in range(args.repeats + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) * 1e-3)
        return sorted(times[1:])  # the first launch warms up

    p_d = torch.from_numpy(pts).cuda()
    for c in (64, 4096):
        axes = rs.randn(c, 3)
        axes /= np.linalg.norm(axes, axis=1, keepdims=True)
        angles = rs.uniform(0.001, 0.01, c)  # small turns: every minimum is found near the point itself, as for a true symmetry
        R = model_sym.rotation(axes, np.cos(angles)[:, None, None], np.sin(angles)[:, None, None])
        table = torch.from_numpy(np.concatenate([R.reshape(c, 9), np.zeros((c, 3))], axis=1)).cuda()
        out = torch.empty(c, dtype=torch.float64, device="cuda")
        t = events(lambda: call("unopose_sym_deviation", ptr(p_d), n, ptr(table), c, math.inf, ptr(out), stream_ptr()))
        med, triples = t[len(t) // 2], c * n * n
        assert torch.isfinite(out).all() and float(out.max()) < 4.0
        rec[f"kernel_c{c}"] = dict(ms=[round(v * 1e3, 3) for v in (t[0], med, t[-1])], triples_per_s=triples / med)
        lines.append(f"  kernel, {c:5d} candidates, no bound: {t[0] * 1e3:9.3f} / {med * 1e3:9.3f} / {t[-1] * 1e3:9.3f} ms (min / median / max): "
                     f"{triples / med:.3e} triples/s ({triples / t[-1]:.3e} .. {triples / t[0]:.3e})")

    def clock(fn, repeats):
        secs, res = [], None
        for _ in range(repeats):
            t0 = time.perf_counter()
            res = fn()
            secs.append(time.perf_counter() - t0)
        return sorted(secs), res

    model_sym.find_symmetries(pts[::16], device="cuda", axes=256)  # warm-up
    secs, res = clock(lambda: model_sym.find_symmetries(pts, device="cuda"), args.repeats)
    assert len(res["symmetries_discrete"]) == 3 and res["report"]["status"] == "ok"
    rec["search_device"] = dict(seconds=[round(s, 4) for s in secs], coarse_count=res["report"]["coarse_count"], coarse_passed=res["report"]["coarse_passed"])
    lines.append(f"  search on the device, {n} vertices, defaults (early exit on): {secs[0]:.4f} .. {secs[-1]:.4f} s per object over {len(secs)} runs; "
                 f"{res['report']['coarse_passed']} of {res['report']['coarse_count']} coarse candidates passed; group of 4 found")

    noisy = pts + rs.normal(0.0, 0.02, pts.shape)  # no exact symmetry: every survivor is refined down to the smallest step
    secs, res = clock(lambda: model_sym.find_symmetries(noisy, device="cuda"), 3)
    assert len(res["symmetries_discrete"]) == 3 and res["report"]["status"] == "ok"
    worst = max(e["deviation"] for e in res["report"]["symmetries"])
    rec["search_device_noisy"] = dict(seconds=[round(s, 4) for s in secs], coarse_passed=res["report"]["coarse_passed"], worst_deviation=worst)
    lines.append(f"  the same with Gaussian noise of 0.02 units on every coordinate (no exact symmetry, full refinement): {secs[0]:.4f} .. {secs[-1]:.4f} s per "
                 f"object over {len(secs)} runs; {res['report']['coarse_passed']} coarse candidates passed; group of 4 found, worst deviation / d {worst:.2e}")

    sub, T16 = pts[:2048], np.zeros((16, 4, 4))
    T16[:, 3, 3], T16[:, :3, :3] = 1.0, model_sym.rotation(np.array([0.0, 0.0, 1.0]), np.cos(0.002 * np.arange(16))[:, None, None], np.sin(0.002 * np.arange(16))[:, None, None])
    secs, _ = clock(lambda: model_sym.sym_deviation_host(sub, T16), 3)
    triples = 2 * 16 * len(sub) ** 2  # both directions
    rec["host_deviation"] = dict(seconds=[round(s, 4) for s in secs], triples_per_s=triples / secs[1])
    lines.append(f"  host specification, {len(sub)} points, 16 transforms both ways, no bound: {secs[0]:.4f} .. {secs[-1]:.4f} s: {triples / secs[1]:.3e} triples/s")
    small = lattice(40.0, 60.0, 90.0, 10.0)
    secs_h, res_h = clock(lambda: model_sym.find_symmetries(small), 3)
    secs_d, res_d = clock(lambda: model_sym.find_symmetries(small, device="cuda"), 3)
    assert res_h == res_d, "device differs from host"
    rec["search_small"] = dict(host_seconds=[round(s, 4) for s in secs_h], device_seconds=[round(s, 4) for s in secs_d])
    lines.append(f"  search, {len(small)} vertices, defaults: host route {secs_h[0]:.4f} .. {secs_h[-1]:.4f} s, device route {secs_d[0]:.4f} .. {secs_d[-1]:.4f} s, "
                 f"identical output")
    print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
