"""Same-box A/B of `ops.query_lrf_group` at 32 x 2048 between two builds of the library.

    python scripts/ubench/lrf_group_ab.py time            # one process: median launch time per configuration, device events
    python scripts/ubench/lrf_group_ab.py ab LIB_A LIB_B [PROCESSES]

`ab` starts PROCESSES (default 6) fresh `time` processes per library, alternating A, B, A, B, ..., each with UNOPOSE_LIB set to its
library and under a time limit of its own; it stops at the first process that fails.  Per configuration it prints both series of
process medians, the spread (the range of A's own process medians) and whether B's median exceeds A's by more than that spread.
"""
import os
import statistics
import subprocess
import sys

CONFIGS = ((0.1, 64), (0.2, 256))


def time_one_process():
    import torch

    from unopose_amd import ops
    from unopose_amd.synthetic import make_batch

    torch.manual_seed(0)
    batch, _, _ = make_batch(32, device="cuda")
    rad = torch.norm(batch["tem1_pts"] - batch["tem1_pts"].mean(1, keepdim=True), dim=2).max(1)[0]
    x = (batch["pts"] / (rad.reshape(-1, 1, 1) + 1e-6)).contiguous()  # the bench clouds, 32 x 2048
    for r, S in CONFIGS:
        for _ in range(5):
            ops.query_lrf_group(x, r, S)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(40)]
        for s, e in ev:
            s.record()
            ops.query_lrf_group(x, r, S)
            e.record()
        torch.cuda.synchronize()
        print(f"MEDIAN_US {r} {S} {statistics.median(s.elapsed_time(e) for s, e in ev) * 1e3:.2f}", flush=True)


def ab(lib_a, lib_b, n):
    series = {(lib, c): [] for lib in "AB" for c in CONFIGS}
    for i in range(2 * n):
        name, lib = ("A", lib_a) if i % 2 == 0 else ("B", lib_b)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "time"], env=dict(os.environ, UNOPOSE_LIB=os.path.abspath(lib)),
                           capture_output=True, text=True, timeout=120)
        if r.returncode != 0:
            print(f"process {i} ({name}) failed with status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            return 1
        for line in r.stdout.splitlines():
            if line.startswith("MEDIAN_US"):
                _, rr, S, us = line.split()
                series[(name, (float(rr), int(S)))].append(float(us))
    print(f"A = {lib_a}\nB = {lib_b}\n{n} fresh processes each, alternating; per process the median of 40 launches (device events), us")
    slower = False
    for c in CONFIGS:
        a, b = series[("A", c)], series[("B", c)]
        ma, mb, spread = statistics.median(a), statistics.median(b), max(a) - min(a)
        bad = mb - ma > spread
        slower |= bad
        print(f"query_lrf_group 32 x 2048 r={c[0]} S={c[1]}\n  A: {' '.join(f'{v:.2f}' for v in a)}   median {ma:.2f}, spread (range) {spread:.2f}\n"
              f"  B: {' '.join(f'{v:.2f}' for v in b)}   median {mb:.2f}\n  B - A = {mb - ma:+.2f} us: {'SLOWER by more than the spread' if bad else 'within the spread'}")
    print("VERDICT:", "B is slower" if slower else "B is not slower than A by more than A's own spread")
    return 1 if slower else 0


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    if sys.argv[1] == "time":
        time_one_process()
    else:
        sys.exit(ab(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 6))
