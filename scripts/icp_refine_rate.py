"""Time the pose refinement (`ops.icp_refine`, csrc/icp.hip: the whole loop of a pair in one workgroup, one launch) against the same rule as a
composite of existing operators (`ops.icp_refine_torch`: per iteration a (B, N1, N2) distance matrix, torch's min, the HIP weighted
Procrustes), and `UNOPose.forward` with `fine_point_matching.icp_iters` 0 against 10.

    operator   B = 32 and B = 1, N1 = N2 = 2048, iters 10 and 20, on partial-view pairs of tests/icp_ref.py (`problem`: the inlier count
               grows over several iterations; how many iterations each pair really takes is printed: a pair that stops early costs the
               kernel nothing more and the composite a full iteration)
    forward    32 pairs, 224 x 224, bf16 autocast, synthetic batch and trained-like weights as in bench.py, eager calls

Device events around every call, --warmup calls per arm first, then --rounds rounds in which the arms run alternately, one process.  Every
line gives the median and the range of the rounds.  No threshold: the numbers are the result.  With --out the table is appended to a file.

    python scripts/icp_refine_rate.py [--rounds 7] [--warmup 3] [--skip-forward] [--out profiles/icp_refine_rate.txt]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def timed(fn, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def ab(arms, rounds, warmup, torch):
    """arms: {name: callable} -> {name: sorted ms}; alternating rounds after `warmup` calls each."""
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            ms[k].append(timed(fn, torch))
    return {k: sorted(v) for k, v in ms.items()}


def fmt(v):
    return f"median {statistics.median(v):9.3f} ms   range {v[0]:9.3f} .. {v[-1]:9.3f}"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tau", type=float, default=0.03)
    ap.add_argument("--skip-forward", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()

    import numpy as np
    import torch

    import icp_ref as I
    from unopose_amd import ops

    torch.set_grad_enabled(False)
    lines = [f"{torch.cuda.get_device_name(0)}; device events, {args.warmup} warm-up calls per arm, {args.rounds} alternating rounds, one process"]
    zs = [I.problem(100 + s, n1=2048, n2=2048) for s in range(32)]
    dev = [torch.from_numpy(np.stack([z[k] for z in zs])).cuda() for k in ("P", "Q", "R0", "t0")]
    for B in (32, 1):
        x = [v[:B].contiguous() for v in dev]
        for iters in (10, 20):
            trace = ops.icp_refine(*x, iters=iters, inlier_thres=args.tau, return_trace=True)[2]
            same = torch.equal(trace, ops.icp_refine_torch(*x, iters=iters, inlier_thres=args.tau, return_trace=True)[2])
            ran = (trace >= 0).sum(1).tolist()
            ms = ab({"kernel": lambda: ops.icp_refine(*x, iters=iters, inlier_thres=args.tau),
                     "composite": lambda: ops.icp_refine_torch(*x, iters=iters, inlier_thres=args.tau)}, args.rounds, args.warmup, torch)
            ratio = statistics.median(ms["composite"]) / statistics.median(ms["kernel"])
            lines.append(f"operator B = {B}, N1 = N2 = 2048, iters = {iters}, tau = {args.tau}: searches run per pair min {min(ran)} / mean {sum(ran) / len(ran):.1f} / "
                         f"max {max(ran)}; traces of the two arms {'equal' if same else 'DIFFER'}")
            for k, v in ms.items():
                lines.append(f"    {k:10s} {fmt(v)}")
            lines.append(f"    composite / kernel (medians): {ratio:.2f} x; ranges {'apart' if ms['kernel'][-1] < ms['composite'][0] or ms['composite'][-1] < ms['kernel'][0] else 'OVERLAP'}")
            print(json.dumps(dict(B=B, iters=iters, searches=ran, kernel_ms=ms["kernel"], composite_ms=ms["composite"], traces_equal=same)), flush=True)
    if not args.skip_forward:
        from unopose_amd.model import UNOPose, default_model_cfg
        from unopose_amd.synthetic import make_batch, trained_like_

        model = trained_like_(UNOPose(default_model_cfg(feature_extraction=dict(img_size=224)))).cuda().eval()
        batch, _, _ = make_batch(32, S=224, seed=0, device="cuda")
        batch["coarse_rand"] = torch.rand(32, 6000 * 3, device="cuda")
        fine = model.fine_point_matching

        def forward(iters):
            def run():
                fine.cfg["icp_iters"] = iters
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    return model(dict(batch))
            return run

        rec = {}
        fine.icp_taps = rec
        forward(10)()
        fine.icp_taps = None
        ran = (rec["icp_trace"] >= 0).sum(1).tolist()
        ms = ab({"icp_iters = 0": forward(0), "icp_iters = 10": forward(10)}, args.rounds, args.warmup, torch)
        fine.cfg["icp_iters"] = 0
        lines.append(f"UNOPose.forward, 32 pairs, 224 x 224, bf16 autocast, eager; inlier_thres 0.1; searches run per pair min {min(ran)} / mean {sum(ran) / len(ran):.1f} / max {max(ran)}")
        for k, v in ms.items():
            lines.append(f"    {k:15s} {fmt(v)}")
        lines.append(f"    difference of the medians: {statistics.median(ms['icp_iters = 10']) - statistics.median(ms['icp_iters = 0']):.3f} ms per forward")
        print(json.dumps(dict(forward_ms=ms, searches=ran)), flush=True)
    print("\n".join(lines))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
