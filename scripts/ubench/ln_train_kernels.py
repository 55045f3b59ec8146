"""Device time per launch (torch profiler) of the residual add + LayerNorm training kernels (csrc/ln_train.hip) and of the kernels of the torch
composite they replace, forward + backward on hot inputs, per shape.  Run on the GPU box: python scripts/ubench/ln_train_kernels.py"""
import os, sys
import torch
import torch.nn.functional as F
from torch.profiler import ProfilerActivity, profile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from unopose_amd import ops

N = 20
for rows, C in ((1576, 256), (65536, 256), (131072, 256), (4099, 1024)):
    a = torch.randn(rows, C, device="cuda", requires_grad=True); b = torch.randn(rows, C, device="cuda", requires_grad=True)
    w = torch.randn(C, device="cuda", requires_grad=True); bias = torch.randn(C, device="cuda", requires_grad=True)
    dy = torch.randn(rows, C, device="cuda")
    for name, fn in (("kernels", lambda: ops._AddLayerNormFn.apply(a, b, w, bias, 1e-5)), ("composite", lambda: F.layer_norm(a + b, (C,), w, bias, 1e-5))):
        def it():
            torch.autograd.grad(fn(), (a, b, w, bias), dy)
        for _ in range(3): it()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(N): it()
            torch.cuda.synchronize()
        tot = 0.0
        for e in sorted(prof.key_averages(), key=lambda e: -e.self_device_time_total):
            if e.self_device_time_total > 0:
                tot += e.self_device_time_total / N
                print(f"rows={rows} C={C} {name}: {e.self_device_time_total / N:8.1f} us x {e.count / N:.0f}  {e.key[:90]}")
        print(f"rows={rows} C={C} {name}: {tot:8.1f} us in all", flush=True)
