"""Device time per launch (torch profiler) of the small trainable linears' kernels (csrc/linear_small_train.hip: forward, dX, dW + db and
its combining launch) and of the kernels of the route they replace (nn.Linear under autograd: the library's forward GEMM, the two mm of the
backward, the bias gradient's sum and, with ReLU, the clamp and the mask multiply), forward + backward on hot inputs, per shape.  Twenty
repetitions after three warm-up runs; the figures are the profiler's device durations, so launch gaps and host time are not in them.
Run on the GPU box: python scripts/ubench/small_linear_train_kernels.py"""
import os, sys
import torch
import torch.nn.functional as F
from torch.profiler import ProfilerActivity, profile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from unopose_amd import ops

R = 20
for rows, K, N in ((1576, 256, 256), (3152, 256, 512), (3152, 512, 256)):
    for relu in (False, True):
        torch.manual_seed(0)
        lin = torch.nn.Linear(K, N).cuda()
        x = torch.randn(rows, K, device="cuda", requires_grad=True)
        g = torch.randn(rows, N, device="cuda")
        leaves = (x, lin.weight, lin.bias)

        def own():
            return ops._SmallLinearFn.apply(x, lin.weight, lin.bias, relu)

        def library():
            y = F.linear(x, lin.weight, lin.bias)
            return F.relu(y) if relu else y

        for name, fn in (("kernels", own), ("library", library)):
            def it():
                torch.autograd.grad(fn(), leaves, g)
            for _ in range(3): it()
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(R): it()
                torch.cuda.synchronize()
            tot, n = 0.0, 0.0
            tag = f"({rows},{K})->{N} relu={int(relu)} {name}"
            for e in sorted(prof.key_averages(), key=lambda e: -e.self_device_time_total):
                if e.self_device_time_total > 0:
                    tot += e.self_device_time_total / R
                    n += e.count / R
                    print(f"{tag}: {e.self_device_time_total / R:8.1f} us x {e.count / R:.0f}  {e.key[:100]}")
            print(f"{tag}: {tot:8.1f} us in all over {n:.0f} launches", flush=True)
