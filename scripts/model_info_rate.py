"""Time the diameter kernel (csrc/modelinfo.hip, `ops.pts_extent`) and put it beside the ADI kernel, whose all-pairs loop it follows:

    brute force   `unopose_pts_extent` with prune = 0 on sphere shells of 2^15 and 2^17 points (nothing could be pruned there anyway),
                  between two device events over prepared buffers: distances evaluated per second -- the kernel visits the tile pairs
                  (a, b >= a), i.e. tiles (tiles + 1) / 2 x tile^2 distances for n points -- and n^2 / time, the rate an all-pairs pass
                  without the symmetry would need;
    adi           `unopose_adi` for ADI_PAIRS = 4 pairs of poses at the same n (enough workgroups to fill the device), the same way:
                  4 n^2 distances per launch.  It does the same three
                  subtractions and one product chain per distance, but may use fused multiply-adds where the diameter kernel by contract
                  may not (its value must carry the host's bits);
    whole call    `ops.pts_extent` (checks, upload, pruning, all pairs, read-back) on a box surface of 2^20 points, wall clock;
    host          `model_info.extent_host` at 2^13 points, with and without pruning, for scale.

Prints one JSON line and, with --out, appends the lines as text.

    python scripts/model_info_rate.py [--repeats 5] [--out profiles/model_info_rate.txt]"""
import argparse
import ctypes
import json
import os
import sys
import time

ADI_PAIRS = 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()

    import numpy as np
    import torch

    from unopose_amd import model_info, ops
    from unopose_amd._lib import call, lib, ptr, stream_ptr
    from unopose_amd.ops.score import adi_sizes, pts_extent_tile

    assert torch.cuda.is_available(), "model_info_rate.py measures on a GPU"
    rs = np.random.RandomState(3)

    def shell(n):
        d = rs.randn(n, 3)
        return (100.0 * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32).astype(np.float64)

    def box(n):
        u = rs.uniform(-1, 1, (n, 3))
        u[np.arange(n), rs.randint(0, 3, n)] = rs.choice([-1.0, 1.0], n)
        return (u * np.array([60.0, 35.0, 90.0])).astype(np.float32).astype(np.float64)

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

    T, doubles = pts_extent_tile(), int(lib().unopose_pts_extent_doubles())
    lines, rec = [f"diameter kernel: tiles of {T} points; ADI: tiles of {adi_sizes()[0]}, slabs of {adi_sizes()[1]}; {args.repeats} launches between device events after a warm-up"], {}
    null = ctypes.c_void_p(None)
    for n in (1 << 15, 1 << 17):
        pts = shell(n)
        offsets = np.array([0, n], np.int64)
        p_d, o_d = torch.from_numpy(pts).cuda(), torch.from_numpy(offsets).cuda()
        out = torch.empty(1, doubles, dtype=torch.float64, device="cuda")
        t = events(lambda: call("unopose_pts_extent", ptr(p_d), ctypes.c_void_p(offsets.ctypes.data), ptr(o_d), 1, 0, null, null, ptr(out), stream_ptr()))
        tiles = -(-n // T)
        evaluated = tiles * (tiles + 1) // 2 * T * T
        pose = torch.from_numpy(np.tile(np.concatenate([np.eye(3).reshape(9), np.zeros(3)]), (ADI_PAIRS, 1))).cuda()
        pose2 = torch.from_numpy(np.tile(np.concatenate([np.eye(3).reshape(9), [1.0, 2.0, 3.0]]), (ADI_PAIRS, 1))).cuda()
        work = torch.empty(ADI_PAIRS * -(-n // adi_sizes()[1]), dtype=torch.float64, device="cuda")
        res = torch.empty(ADI_PAIRS, dtype=torch.float64, device="cuda")
        ta = [v / ADI_PAIRS for v in events(lambda: call("unopose_adi", ptr(p_d), n, ptr(pose), ptr(pose2), ADI_PAIRS, ptr(work), ptr(res), stream_ptr()))]
        med, meda = t[len(t) // 2], ta[len(ta) // 2]
        rec[f"n{n}"] = dict(extent_ms=[round(v * 1e3, 3) for v in (t[0], med, t[-1])], adi_ms=[round(v * 1e3, 3) for v in (ta[0], meda, ta[-1])],
                            extent_evaluated_per_s=evaluated / med, extent_n2_per_s=n * n / med, adi_n2_per_s=n * n / meda,
                            evaluated_ratio_to_adi=round(evaluated / med / (n * n / meda), 3), n2_ratio_to_adi=round(meda / med, 3),
                            diameter=float(np.sqrt(out.cpu().numpy()[0, 6])))
        lines.append(f"  n = {n:7d} shell  diameter kernel {t[0] * 1e3:8.3f} / {med * 1e3:8.3f} / {t[-1] * 1e3:8.3f} ms (min / median / max): "
                     f"{evaluated / med:.3e} distances evaluated/s, n^2 / t = {n * n / med:.3e}/s")
        lines.append(f"  {'':18s}ADI, per pair   {ta[0] * 1e3:8.3f} / {meda * 1e3:8.3f} / {ta[-1] * 1e3:8.3f} ms: {n * n / meda:.3e} distances/s;  "
                     f"diameter / ADI = {evaluated / med / (n * n / meda):.2f} per evaluated distance, {meda / med:.2f} per n^2")
    n = 1 << 20
    pts = box(n)
    ops.pts_extent([pts[:4096]], "cuda")  # warm-up
    torch.cuda.synchronize()
    secs = []
    for _ in range(3):
        t0 = time.perf_counter()
        d = ops.pts_extent([pts], "cuda")[2][0]
        secs.append(time.perf_counter() - t0)
    kept = int(model_info.prune_keep(pts).sum())
    rec["box_2e20"] = dict(seconds=[round(s, 4) for s in sorted(secs)], kept_points_host_rule=kept, diameter=float(d))
    lines.append(f"  n = {n} box surface, ops.pts_extent with pruning (checks, upload, kernels, read-back): {min(secs):.4f} .. {max(secs):.4f} s; "
                 f"the rule keeps {kept} of the points; diameter {float(d)!r}")
    n = 1 << 13
    pts = shell(n)
    for name, p, prune in (("shell, no pruning", pts, False), ("box, pruned", box(n), True)):
        t0 = time.perf_counter()
        dh = model_info.extent_host(p, prune=prune)[2]
        sec = time.perf_counter() - t0
        assert dh == ops.pts_extent([p], "cuda", prune=prune)[2][0], "device differs from host"
        rec[f"host_{'pruned' if prune else 'brute'}_2e13"] = round(sec, 4)
        lines.append(f"  n = {n} host route ({name}): {sec:.4f} s, equal to the device's bits")
    print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
