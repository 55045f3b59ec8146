"""Same-box A/B of the training step (bench.py --train shape) for one `unopose_amd.ops` attribute: one process per measurement, alternating.
usage: python scripts/ubench/train_ab.py TRAIN_OWN_GEMM_MIN_FLOP 2e10 1e10 [--dtype bf16]   (--dtype: bench.py's --train-dtype, default fp32)"""
import io, json, os, subprocess, sys
from contextlib import redirect_stdout
R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, R)
if sys.argv[1] == "--one":
    import bench
    from unopose_amd import ops
    name, val = sys.argv[2], sys.argv[3]
    assert hasattr(ops, name), name
    setattr(ops, name, {"True": True, "False": False}.get(val, None) if val in ("True", "False") else float(val))
    dtype = sys.argv[4] if len(sys.argv) > 4 else "fp32"
    sys.argv = ["bench.py", "--train", "--steps", "5", "--warmup", "2", "--train-dtype", dtype]
    buf = io.StringIO()
    with redirect_stdout(buf):
        bench.main()
    line = json.loads(buf.getvalue().strip().splitlines()[-1])
    print(f"{name}={val} ({dtype}): {line['ms_per_step']:.2f} ms/step  loss {line['loss_first_last'][1]:.4f}", flush=True)
else:
    rest = sys.argv[2:]
    dtype = rest.pop(rest.index("--dtype") + 1) if "--dtype" in rest else "fp32"
    name, vals, reps = sys.argv[1], [a for a in rest if not a.startswith("--")], 3
    for rep in range(reps):
        for v in vals:
            subprocess.run([sys.executable, os.path.abspath(__file__), "--one", name, v, dtype], stderr=subprocess.DEVNULL)
