"""Time the reference-view search (csrc/reftargets.hip, `ops.ref_select`):

    kernels       `unopose_ref_select` (both launches) at (Q, C, S) = (256, 4096, 1) and (256, 4096, 315), over prepared buffers: windows of
                  about 0.1 s of back-to-back calls between two device events, time per call; (query, candidate, symmetry) triples per
                  second, and the float64 VALU operations that is -- 9
                  multiply / fma, 2 additions, the clamp and the max per triple, i.e. 13 -- beside the composition's 27 per (candidate,
                  symmetry, query tile);
    slab sizes    the 315-symmetry shape at the automatic slab size and at four times and a quarter of it, the same way: what the split costs;
    whole call    `ops.ref_select` (checks, upload, both kernels, read-back) at both shapes, wall clock;
    host          `ref_targets.select_host` at (40, 300, 315), for scale, and the assertion that the device gives its bits there.

Prints one JSON line and, with --out, appends the lines as text.

    python scripts/ref_targets_rate.py [--repeats 5] [--out profiles/ref_targets_rate.txt]   (--out appends: the file's first line is the script's own)"""
import argparse
import json
import os
import sys
import time

OPS_PER_TRIPLE = 13
WINDOW_S = 0.1  # device time of one timed window
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()

    import numpy as np
    import torch

    from unopose_amd import bop_eval, ops, ref_targets
    from unopose_amd._lib import call, ptr, stream_ptr
    from unopose_amd.ops.score import ref_select_sizes, ref_select_slab

    assert torch.cuda.is_available(), "ref_targets_rate.py measures on a GPU"
    rs = np.random.RandomState(3)

    def rotations(n):
        q = rs.randn(n, 4)
        w, x, y, z = (q / np.linalg.norm(q, axis=1, keepdims=True)).T
        return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                         2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1).reshape(n, 3, 3)

    def case(Q, C, S):
        info = {} if S == 1 else {"symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}
        syms = np.stack([s["R"] for s in bop_eval.symmetry_transformations(info)])
        assert len(syms) == S
        q_scene, c_scene = rs.randint(0, 20, Q).astype(np.int64), rs.randint(0, 20, C).astype(np.int64)
        key = lambda scene, im: (scene.astype(np.uint64) << np.uint64(32)) | im.astype(np.uint64)
        return (rotations(Q), q_scene, key(q_scene, np.arange(Q)), rotations(C), c_scene, key(c_scene, Q + np.arange(C)), syms)

    def events(fn):
        """Seconds per call: `args.repeats` windows, each one pair of device events around as many back-to-back calls as fill WINDOW_S."""
        def window(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e-3 / n

        window(3)  # the first launches warm up
        n = max(10, int(WINDOW_S / window(10)))
        return sorted(window(n) for _ in range(args.repeats)), n

    trace_min = ref_targets.trace_min_of(50.0)
    q_tile, e_tile = ref_select_sizes()
    lines = [f"scripts/ref_targets_rate.py on one {torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]} device, measured on {time.strftime('%Y-%m-%d')} (one visit: the ranges are within-run spreads)",
             f"reference-view search: {q_tile} queries per workgroup (one wave), LDS tiles of {e_tile} entries; {args.repeats} windows of about {WINDOW_S:g} s of back-to-back "
             "calls (both kernels) between two device events, after a warm-up"]
    rec = {}
    for Q, C, S in ((256, 4096, 1), (256, 4096, 315)):
        Rq, q_scene, q_key, Rc, c_scene, c_key, syms = host = case(Q, C, S)
        dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (Rq, q_scene, q_key.view(np.int64), Rc, c_scene, c_key.view(np.int64), syms)]
        auto = ref_select_slab(Q, C, S)
        triples = Q * C * S
        for slab in [auto] + ([min(C, 4 * auto), max(1, auto // 4)] if S > 1 else []):
            slabs = -(-C // slab)
            work = torch.empty(5 * Q * slabs, dtype=torch.int64, device="cuda")
            out = torch.empty(4, Q, dtype=torch.int64, device="cuda")
            t, calls = events(lambda: call("unopose_ref_select", ptr(dev[0]), ptr(dev[1]), ptr(dev[2]), Q, ptr(dev[3]), ptr(dev[4]), ptr(dev[5]), C, ptr(dev[6]), S,
                                    trace_min, 0, 1, slab, ptr(work), ptr(out), stream_ptr()))
            med = t[len(t) // 2]
            rec[f"q{Q}_c{C}_s{S}_slab{slab}"] = dict(ms=[round(v * 1e3, 4) for v in (t[0], med, t[-1])], calls_per_window=calls, workgroups=slabs * -(-Q // q_tile), triples_per_s=triples / med,
                                                     valu_ops_per_s=triples * OPS_PER_TRIPLE / med)
            lines.append(f"  (Q, C, S) = ({Q}, {C}, {S:3d}), {slab:4d} candidates per slab{' (automatic)' if slab == auto else '':12s}, {slabs * -(-Q // q_tile):5d} workgroups: "
                         f"{t[0] * 1e3:8.4f} / {med * 1e3:8.4f} / {t[-1] * 1e3:8.4f} ms per call (min / median / max of the windows, {calls} calls each): {triples / med:.3e} triples/s, "
                         f"{triples * OPS_PER_TRIPLE / med:.3e} float64 VALU operations/s")
        ops.ref_select(*host, trace_min)  # warm-up
        secs = []
        for _ in range(3):
            t0 = time.perf_counter()
            got = ops.ref_select(*host, trace_min)
            secs.append(time.perf_counter() - t0)
        rec[f"q{Q}_c{C}_s{S}_call_s"] = [round(s, 5) for s in sorted(secs)]
        lines.append(f"  {'':24s}ops.ref_select (checks, upload, kernels, read-back): {min(secs) * 1e3:.3f} .. {max(secs) * 1e3:.3f} ms; "
                     f"{int((got[0] >= 0).sum())} of {Q} queries have an eligible view, median n_eligible {float(np.median(got[1])):g}")
    Q, C, S = 40, 300, 315
    host = case(Q, C, S)
    t0 = time.perf_counter()
    want = ref_targets.select_host(*host, trace_min)
    sec = time.perf_counter() - t0
    got = ops.ref_select(*host, trace_min)
    assert all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3])) and np.array_equal(got[3].view(np.int64), want[3].view(np.int64)), "device differs from host"
    rec["host_q40_c300_s315"] = dict(seconds=round(sec, 3), triples_per_s=Q * C * S / sec)
    lines.append(f"  (Q, C, S) = ({Q}, {C}, {S}) host rule: {sec:.3f} s, {Q * C * S / sec:.3e} triples/s, equal to the device's bits")
    print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
