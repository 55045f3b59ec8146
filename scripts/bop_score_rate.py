"""Time the BOP'19 scorer on the large synthetic case (tests/bop_score_case.py) in (estimate, ground truth) pairs per second through
up to three routes, all with the HIP rasteriser:

    parent   `average_recall` of another version of unopose_amd/bop_eval.py (--parent FILE, e.g. `git show HEAD~1:unopose_amd/bop_eval.py`)
    host     this tree's `average_recall(...)`           (numpy per pair; the same code as the parent's)
    device   this tree's `average_recall(..., device=)`  (csrc/bopscore.hip)

One warm-up call per route, then --rounds rounds in which the routes run alternately; the wall clock is around the whole call and the
device is synchronised before it is read.  Every route must return the same recall tables.  Prints one JSON line per variant and,
with --out, appends the ranges as text.

    python scripts/bop_score_rate.py [--parent FILE] [--rounds 3] [--extra 0,7] [--out profiles/bop_score_ab.txt]"""
import argparse
import importlib.util
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--parent", help="a bop_eval.py of another commit, timed as the baseline")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--extra", default="0", help="comma-separated `extra_estimates` of make_large_case: 0 = the tests' case (210 estimates), 7 -> 850, 20 -> 2155")
    ap.add_argument("--n-top", type=int, default=-1)
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch

    import bop_score_case as C
    from unopose_amd import bop_eval
    from unopose_amd.render import HipDepthRenderer

    routes = {}
    if args.parent:
        spec = importlib.util.spec_from_file_location("bop_eval_parent", args.parent)
        parent = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(parent)
        routes["parent"] = lambda *a, **k: parent.average_recall(*a, **k)
    routes["host"] = lambda *a, **k: bop_eval.average_recall(*a, **k)
    routes["device"] = lambda *a, **k: bop_eval.average_recall(*a, device="cuda", **k)
    lines = []
    for extra in (int(v) for v in args.extra.split(",")):
        models, scene_gt, cameras, results, im_width, depth_images, (W, H) = C.make_large_case(extra_estimates=extra)
        ren = HipDepthRenderer(W, H)
        for oid, m in models.items():
            ren.add_object(oid, m["verts"], m["faces"])
        units = bop_eval.scored_pairs(bop_eval._walk(results, scene_gt, cameras, args.n_top, None))
        n_pairs = sum(len(u[4]) * len(u[5]) for u in units)

        def run(route):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = routes[route](results, scene_gt, models, cameras, im_width, n_top=args.n_top, renderer=ren, depth_images=depth_images)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out

        outs = {r: run(r)[1] for r in routes}  # warm-up
        for r in routes:
            assert all(outs[r][k] == outs["host"][k] for k in ("recalls_vsd", "recalls_mssd", "recalls_mspd")), f"{r} differs from host"
        secs = {r: [] for r in routes}
        for _ in range(args.rounds):
            for r in routes:
                secs[r].append(run(r)[0])
        rate = {r: sorted(n_pairs / s for s in v) for r, v in secs.items()}
        base = "parent" if "parent" in rate else "host"
        rec = dict(estimates=len(results), pairs=n_pairs, image=[W, H], n_top=args.n_top, rounds=args.rounds, AR=outs["host"]["AR"],
                   pairs_per_s={r: [round(v[0], 1), round(v[-1], 1)] for r, v in rate.items()},
                   seconds={r: [round(min(v), 4), round(max(v), 4)] for r, v in secs.items()},
                   device_over_baseline=[round(rate["device"][0] / rate[base][-1], 2), round(rate["device"][-1] / rate[base][0], 2)], baseline=base,
                   ranges_apart=rate["device"][0] > rate[base][-1])
        print(json.dumps(rec), flush=True)
        lines.append(f"{len(results)} estimates, {n_pairs} pairs, {W} x {H}, n_top {args.n_top}, {args.rounds} alternating rounds after a warm-up call each")
        for r, v in rate.items():
            lines.append(f"    {r:7s} {v[0]:9.1f} .. {v[-1]:9.1f} pairs/s   ({min(secs[r]):.3f} .. {max(secs[r]):.3f} s per call)")
        lines.append(f"    device / {base}: {rec['device_over_baseline'][0]} .. {rec['device_over_baseline'][1]} x; ranges "
                     f"{'apart' if rec['ranges_apart'] else 'OVERLAP'}; recall tables equal on every route")
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
