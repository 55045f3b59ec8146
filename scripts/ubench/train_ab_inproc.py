"""In-process A/B of the training step (bench.py --train shape) for one boolean `unopose_amd.ops` switch: one model, the switch alternated in
blocks of three steps, every step timed on its own (synchronise, host clock, synchronise).  Complements train_ab.py (a process per measurement)
where the process-to-process spread hides a small difference: both positions see the same clocks, allocator state and drift.
usage: python scripts/ubench/train_ab_inproc.py TRAIN_OWN_LN [fp32|bf16]"""
import os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from unopose_amd import ops
from unopose_amd.model import UNOPose, default_model_cfg
from unopose_amd.synthetic import make_train_batch, trained_like_
from unopose_amd.train import build_optimizer, freeze_backbone, train_step

name, dtype = sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "fp32"
assert isinstance(getattr(ops, name), bool), name
dev = torch.device("cuda:0")
torch.manual_seed(0)
model = freeze_backbone(trained_like_(UNOPose(default_model_cfg(fine_npoint=4096, feature_extraction=dict(img_size=224)))).to(dev))
batch = make_train_batch(8, 4096, 4096 + 2048, 224, seed=300, device=dev)
opt, sched = build_optimizer(model, lr=1e-4, total_iters=188340)
amp = torch.bfloat16 if dtype == "bf16" else None


def step():
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    train_step(model, batch, opt, sched, amp_dtype=amp)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


for v in (True, False):  # warm-up of both routes
    setattr(ops, name, v)
    for _ in range(3):
        step()
times = {True: [], False: []}
for rnd in range(5):
    for v in (True, False):
        setattr(ops, name, v)
        times[v] += [step() for _ in range(3)]
for v in (True, False):
    t = sorted(times[v])
    print(f"{dtype} {name}={v}: min {t[0]:.2f} median {t[len(t) // 2]:.2f} max {t[-1]:.2f} ms/step over {len(t)} steps: " + " ".join(f"{x:.1f}" for x in times[v]), flush=True)
for v in (True, False):  # peak memory of one step per position
    setattr(ops, name, v)
    step()
    torch.cuda.reset_peak_memory_stats()
    step()
    print(f"{dtype} {name}={v}: peak memory of a step {torch.cuda.max_memory_allocated() / 2 ** 20:.1f} MiB", flush=True)
