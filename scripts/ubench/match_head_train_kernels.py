"""Device time per launch (torch profiler) of the match head's training kernels (csrc/match_train.hip: the split pass, the row and column
forward sweeps, the row and column backward sweeps) and of the kernels of the composite they replace (the fp32 similarity, ops.infonce_two_way,
ops.saliency_pair, max(2)[1]), forward + backward on hot inputs, per shape; and the sweeps' share of the bf16 MFMA time of their
6 products x 3 MFMAs x 2 B R C 256 FLOP (2 forward, 4 backward).  Run on the GPU box: python scripts/ubench/match_head_train_kernels.py"""
import os, sys
import torch
import torch.nn.functional as F
from torch.profiler import ProfilerActivity, profile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from unopose_amd import ops

TAU = 10.0
PEAK = 2.5e15  # dense bf16 FLOP/s of the MI355X


def composite(a, b, s1, s2, l1, l2):
    S = (a @ b.transpose(1, 2)) * TAU
    m1, m2 = ops.saliency_pair(S, s1, s2)
    return ops.infonce_two_way(S, l1, l2), m1, m2, S[:, 1:, :].max(2)[1]


R = 5
for B, n in ((8, 4096), (8, 2048)):
    g = torch.Generator().manual_seed(1)
    a = F.normalize(torch.randn(B, n + 1, 256, generator=g), dim=2).cuda().requires_grad_(True)
    b = F.normalize(torch.randn(B, n + 1, 256, generator=g), dim=2).cuda().requires_grad_(True)
    s1, s2 = (torch.randn(B, n, 1, generator=g).cuda().requires_grad_(True) for _ in range(2))
    l1, l2 = (torch.randint(0, n + 1, (B, n), generator=g).cuda() for _ in range(2))
    gL, g1, g2 = torch.randn(B, generator=g).cuda(), torch.randn(B, n, 1, generator=g).cuda(), torch.randn(B, n, 1, generator=g).cuda()
    for name, fn in (("kernels", lambda: ops.match_head(a, b, s1, s2, l1, l2, TAU, True)), ("composite", lambda: composite(a, b, s1, s2, l1, l2))):
        def it():
            loss, m1, m2, _ = fn()
            torch.autograd.grad((loss, m1, m2), (a, b, s1, s2), (gL, g1, g2))
        for _ in range(2): it()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(R): it()
            torch.cuda.synchronize()
        tot = sweeps = 0.0
        for e in sorted(prof.key_averages(), key=lambda e: -e.self_device_time_total):
            if e.self_device_time_total > 0:
                tot += e.self_device_time_total / R
                if "match_fwd_kernel" in e.key or "match_bwd_kernel" in e.key:
                    sweeps += e.self_device_time_total / R
                print(f"({B},{n + 1},{n + 1}) {name}: {e.self_device_time_total / R:8.1f} us x {e.count / R:.0f}  {e.key[:90]}")
        print(f"({B},{n + 1},{n + 1}) {name}: {tot:8.1f} us in all", flush=True)
        if sweeps:
            ideal = 6 * 3 * 2.0 * B * (n + 1) * (n + 1) * 256 / PEAK * 1e6
            print(f"({B},{n + 1},{n + 1}) kernels: the four sweeps {sweeps:.1f} us; their 18 bf16 MFMA passes at {PEAK / 1e15:.1f} PFLOP/s {ideal:.1f} us "
                  f"= {100 * ideal / sweeps:.1f} % of the sweeps' time", flush=True)
