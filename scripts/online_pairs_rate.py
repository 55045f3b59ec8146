"""Does the online pair source (unopose_amd/provider_online.py) keep a training step fed?  Three numbers on one GPU, one process, at the
training shape of `bench.py --train` with the reference's configured point counts (8 pairs, 2048 observed and 5000 template points,
fine_npoint 2048, 224 x 224 crops, frozen backbone, fp32, `train.train_step_gated` on `optim.FusedAdam`):

  source    batches per second of `OnlinePairs.batch` alone (recipe, renders, item kernels, colour augmentation, crops), each batch
            waited for, host clock
  fed       seconds per step of the training step on `OnlinePairs.iterate()` -- batch i + 1 prepared on the side stream by the helper
            thread while step i runs
  resident  seconds per step on one batch that stays on the device

    python scripts/online_pairs_rate.py [--models DIR] [--rounds 3] [--steps 10] [--scene] [--out profiles/online_pairs_rate.txt]

--scene adds a leg with the scene stage at its defaults (`dataloader.train.online.scene`: background plane, depth-sensor model) to `source` and
`fed`, measured beside the scene-off leg in the same process, the two alternating round by round, and reports the stage's cost per batch; the
output then goes to profiles/online_scene_rate.txt.

Without --models, four ellipsoids (5120 faces each, vertex colours) are written to a temporary folder.  `fed` and `resident` alternate
`--rounds` times in the same process; the spread is min - max of the rounds' means.  The aim: `fed` within `resident`'s own spread."""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _icosphere(levels):
    import numpy as np

    p = (1 + 5 ** 0.5) / 2
    v = [np.asarray(x, np.float64) / np.linalg.norm(x) for x in
         [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(levels):
        cache, out = {}, []

        def mid(a, b):
            k = (min(a, b), max(a, b))
            if k not in cache:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                cache[k] = len(v) - 1
            return cache[k]

        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = out
    return np.stack(v), np.asarray(f, np.int32)


def write_models(folder, n=4):
    """n ellipsoids of about 100 to 160 mm as ASCII PLYs with normals and vertex colours."""
    import numpy as np

    v, f = _icosphere(4)
    rs = np.random.RandomState(0)
    for o in range(1, n + 1):
        axes = rs.uniform(50.0, 80.0, 3)
        pts, nrm = v * axes, v / axes
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        col = (127 + 120 * np.sin(v @ rs.uniform(2, 9, (3, 3)))).astype(np.uint8)
        with open(os.path.join(folder, f"obj_{o:06d}.ply"), "w") as fh:
            fh.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\n"
                     "property float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nelement face %d\nproperty list uchar int vertex_indices\n"
                     "end_header\n" % (len(pts), len(f)))
            for p, q, c in zip(pts, nrm, col):
                fh.write("%.6f %.6f %.6f %.6f %.6f %.6f %d %d %d\n" % (*p, *q, *c))
            for t in f:
                fh.write("3 %d %d %d\n" % tuple(t))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--models", default=None, help="a folder of obj_XXXXXX.ply files (default: four synthetic ellipsoids)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--scene", action="store_true", help="add the legs with the scene stage on, beside the scene-off ones")
    ap.add_argument("--out", default=None, help="default: profiles/online_pairs_rate.txt, with --scene profiles/online_scene_rate.txt")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "online_scene_rate.txt" if args.scene else "online_pairs_rate.txt")

    import torch

    from unopose_amd.model import UNOPose, default_model_cfg
    from unopose_amd.optim import FusedAdam
    from unopose_amd.provider_online import ONLINE_DEFAULTS, OnlinePairs
    from unopose_amd.synthetic import trained_like_
    from unopose_amd.train import freeze_backbone, train_step_gated

    if not torch.cuda.is_available():
        sys.exit("online_pairs_rate: needs a GPU (a rate measured elsewhere says nothing)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    tmp = None
    if args.models is None:
        tmp = tempfile.TemporaryDirectory()
        write_models(tmp.name)
    cfg = dict(img_size=224, n_sample_observed_point=2048, n_sample_template_point=5000, min_px_count_visib=512, min_visib_fract=0.1, dilate_mask=True,
               rgb_mask_flag=True, shift_range=0.01, online=dict(ONLINE_DEFAULTS))
    src = OnlinePairs(args.models or tmp.name, cfg, dev, seed=1, batch_size=args.pairs)
    legs = [("", src)]
    if args.scene:
        legs.append(("+scene", OnlinePairs(args.models or tmp.name, dict(cfg, online=dict(ONLINE_DEFAULTS, scene={})), dev, seed=1, batch_size=args.pairs)))
    lines = ["online_pairs_rate: %d pairs, %d observed / %d template points, %d^2 crops, canvas %s, ssaa %d, %d models; %s" % (
        args.pairs, cfg["n_sample_observed_point"], cfg["n_sample_template_point"], cfg["img_size"], tuple(ONLINE_DEFAULTS["canvas"]), ONLINE_DEFAULTS["ssaa"],
        len(src.models), torch.cuda.get_device_name(dev))]

    def say(line):
        print(line, flush=True)
        lines.append(line)

    # -- the source alone
    for _, source in legs:
        for i in range(2):
            source.batch(i)
    torch.cuda.synchronize()
    rates = {name: [] for name, _ in legs}
    for r in range(args.rounds):
        for name, source in legs:
            t0 = time.perf_counter()
            for i in range(args.steps):
                source.batch(100 * r + i)
                torch.cuda.synchronize()
            rates[name].append(args.steps / (time.perf_counter() - t0))
    for name, _ in legs:
        say("%-9s %.1f batches/s (rounds: %s)" % ("source" + name, sum(rates[name]) / len(rates[name]), ", ".join("%.1f" % v for v in rates[name])))
    if args.scene:
        cost = [1000.0 / on - 1000.0 / off for on, off in zip(rates["+scene"], rates[""])]
        say("scene stage in the source: %.2f ms per batch (rounds: %s)" % (sum(cost) / len(cost), ", ".join("%.2f" % v for v in cost)))

    # -- the step, fed and resident, alternating
    torch.manual_seed(0)
    model = freeze_backbone(trained_like_(UNOPose(default_model_cfg(fine_npoint=2048, feature_extraction=dict(img_size=224)))).to(dev))
    opt = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=1e-4, betas=(0.5, 0.999), eps=1e-6, weight_decay=0.0)
    resident = src.batch(7)
    for _ in range(3):
        train_step_gated(model, resident, opt, None, clip_max_norm=35.0)
    torch.cuda.synchronize()

    def run(batches):
        t0 = time.perf_counter()
        for _ in range(args.steps):
            train_step_gated(model, next(batches), opt, None, clip_max_norm=35.0)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps

    fed, res = [], []
    streams = [(name, source.iterate(1000), []) for name, source in legs]
    for _, stream, _ in streams:
        next(stream)  # the first batch is not prefetched under a step
    for _ in range(args.rounds):
        for _, stream, times in streams:
            times.append(run(stream))
        res.append(run(iter(lambda: resident, None)))
    for _, stream, _ in streams:
        stream.close()
    fed = streams[0][2]
    for name, _, times in streams:
        say("%-9s %.4f s/step (rounds: %s)" % ("fed" + name, sum(times) / len(times), ", ".join("%.4f" % v for v in times)))
    say("resident  %.4f s/step (rounds: %s)" % (sum(res) / len(res), ", ".join("%.4f" % v for v in res)))
    spread = max(res) - min(res)
    gap = sum(fed) / len(fed) - sum(res) / len(res)
    say("resident spread %.4f s; fed - resident %.4f s: the aim (a prefetched batch is ready before its step) is %s" % (
        spread, gap, "met" if gap <= spread else "NOT met"))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    if tmp is not None:
        tmp.cleanup()


if __name__ == "__main__":
    main()
