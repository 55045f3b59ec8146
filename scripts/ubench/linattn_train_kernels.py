"""Device time per launch (torch profiler) of the focused linear attention's training kernels (csrc/linattn_train.hip: key state, query
forward, query-side and key-side backward, the partial sums) and of the kernels of the torch composite they replace, forward + backward
on hot inputs, per shape.  Run on the GPU box: python scripts/ubench/linattn_train_kernels.py"""
import os, sys
import torch
import torch.nn.functional as F
from torch.profiler import ProfilerActivity, profile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from unopose_amd import ops


def composite(yq, yk, v, s):
    """the core of ops.focused_linear_attention_torch from the projections' outputs"""
    q, k = (F.relu(yq) + 1e-6) * s, (F.relu(yk) + 1e-6) * s
    qn, kn = q.norm(dim=-1, keepdim=True), k.norm(dim=-1, keepdim=True)
    q, k = q ** 3, k ** 3
    q = q / q.norm(dim=-1, keepdim=True) * qn
    k = k / k.norm(dim=-1, keepdim=True) * kn
    B, N, _ = q.shape
    q, k, v = q.reshape(B, N, 4, 64), k.reshape(B, -1, 4, 64), v.reshape(B, -1, 4, 64)
    z = 1 / (torch.einsum("bihc,bhc->bih", q, k.sum(dim=1)) + 1e-6)
    kv = torch.einsum("bjhc,bjhd->bhcd", k, v)
    return (torch.einsum("bihc,bhcd->bihd", q, kv) * z.unsqueeze(-1)).reshape(B, N, 256)


R = 10
for B, N, J in ((16, 4096, 196), (16, 2048, 196)):
    yq = torch.randn(B, N, 256, device="cuda", requires_grad=True)
    yk = torch.randn(B, J, 256, device="cuda", requires_grad=True); v = torch.randn(B, J, 256, device="cuda", requires_grad=True)
    s = (0.5 + torch.rand(256, device="cuda")).requires_grad_(True)
    dO = torch.randn(B, N, 256, device="cuda")
    for name, fn in (("kernels", lambda: ops._LinearAttnFn.apply(yq, yk, v, s)), ("composite", lambda: composite(yq, yk, v, s))):
        def it():
            torch.autograd.grad(fn(), (yq, yk, v, s), dO)
        for _ in range(3): it()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(R): it()
            torch.cuda.synchronize()
        tot = 0.0
        for e in sorted(prof.key_averages(), key=lambda e: -e.self_device_time_total):
            if e.self_device_time_total > 0:
                tot += e.self_device_time_total / R
                print(f"({B},{N},256)x{J} {name}: {e.self_device_time_total / R:8.1f} us x {e.count / R:.0f}  {e.key[:90]}")
        print(f"({B},{N},256)x{J} {name}: {tot:8.1f} us in all", flush=True)
