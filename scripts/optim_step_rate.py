"""Time from the end of backward() to the end of the parameter update on the real model's trainable parameter set, for two routes:

  parent  train.zero_nonfinite_grads_  ->  clip_grad_norm_(35)  ->  torch.optim.Adam.step   (what train.train_step runs)
  fused   optim.FusedAdam.step(finite, 35)                                                  (csrc/optim.hip: three launches)

    python scripts/optim_step_rate.py [--rounds 3] [--iters 30] [--out profiles/fused_adam_ab.txt]

The gradients come from one real backward (frozen backbone, trained-like weights, a synthetic batch) and are copied into fresh tensors before
every timed step, as after zero_grad(set_to_none=True).  Each measurement is a fresh process (`--route`), the routes alternate over the rounds
in one visit, no profiler runs during the timed steps; the kernel launches of one further step are counted with torch's profiler afterwards.
The parent process never touches the GPU.  A route that fails ends the visit: nothing more is started."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(route, iters, warm):
    import torch

    from unopose_amd.losses import process_loss
    from unopose_amd.model import UNOPose, default_model_cfg
    from unopose_amd.optim import FusedAdam
    from unopose_amd.synthetic import make_train_batch, trained_like_
    from unopose_amd.train import freeze_backbone, zero_nonfinite_grads_

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = freeze_backbone(trained_like_(UNOPose(default_model_cfg(fine_npoint=1024))).to(dev)).train()
    batch = make_train_batch(2, 1024, 2500, 224, seed=300, device=dev)
    process_loss(model(dict(batch)))["loss"].backward()
    params = [p for p in model.parameters() if p.grad is not None]
    grads = [p.grad.detach().clone() for p in params]
    kw = dict(lr=1e-4, betas=(0.5, 0.999), eps=1e-6, weight_decay=0.0)
    finite = torch.ones(1, dtype=torch.bool, device=dev)
    if route == "fused":
        opt = FusedAdam(params, **kw)

        def step():
            opt.step(finite, 35.0)
    else:
        opt = torch.optim.Adam(params, **kw)

        def step():
            zero_nonfinite_grads_(model)
            torch.nn.utils.clip_grad_norm_(params, 35.0)
            opt.step()

    def fresh_grads():
        for p, g in zip(params, grads):
            p.grad = g.clone()

    times = []
    for i in range(warm + iters):
        fresh_grads()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        step()
        b.record()
        b.synchronize()
        if i >= warm:
            times.append(a.elapsed_time(b) * 1e3)
    launches = None
    try:  # one more step under the profiler, after the timed ones
        fresh_grads()
        torch.cuda.synchronize()
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        launches = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
                       and "memset" not in e.name.lower())
    except Exception as e:  # the count is an extra: the timing above stands without it
        launches = f"not counted ({type(e).__name__})"
    times.sort()
    print(json.dumps({"route": route, "tensors": len(params), "elements": sum(p.numel() for p in params), "iters": iters,
                      "us_median": times[len(times) // 2], "us_min": times[0], "us_max": times[-1], "kernel_launches": launches}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--route", choices=["parent", "fused"], help="(child) measure one route in this process")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fused_adam_ab.txt"))
    args = ap.parse_args()
    if args.route:
        return child(args.route, args.iters, args.warm)
    rows = []
    for r in range(args.rounds):
        for route in ("parent", "fused"):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--route", route, "--iters", str(args.iters), "--warm", str(args.warm)],
                               capture_output=True, text=True, timeout=args.timeout)
            if p.returncode != 0:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                sys.exit(f"route {route} failed in round {r + 1} (exit code {p.returncode}): stopping")
            rows.append(dict(json.loads(p.stdout.strip().splitlines()[-1]), round=r + 1))
            print(rows[-1], flush=True)
    lines = ["scripts/optim_step_rate.py: end of backward -> end of the update, device events, microseconds per step",
             "%d tensors, %d elements; %d rounds, routes alternating, a fresh process each, %d timed steps after %d warm-up steps, profiler off"
             % (rows[0]["tensors"], rows[0]["elements"], args.rounds, args.iters, args.warm)]
    for route in ("parent", "fused"):
        mine = [r for r in rows if r["route"] == route]
        med = [r["us_median"] for r in mine]
        lines.append("%-6s median per round %s  range of the medians %.1f .. %.1f  (all steps %.1f .. %.1f)  kernel launches per step: %s"
                     % (route, " ".join("%.1f" % m for m in med), min(med), max(med), min(r["us_min"] for r in mine), max(r["us_max"] for r in mine),
                        mine[0]["kernel_launches"]))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
