"""Crops per second of the two ways a training crop is finished (window crop -> 80 %: colour augmentation -> mask -> resize -> normalise):

  host    what `MegaPoseOneRefTrainSet._crop_tensor` does in a loader worker, on one core
  device  what a `device_crops` loader leaves to the training process: `ops.finish_crops` on a collated batch (upload from pinned memory,
          `ops.color_augment`, `PrepPlan` + `prep_crop_resize`), host clock around work that ends in a device synchronise; and, on its own
          line, what stays in the worker: drawing the plans and collating (`ColorAugmentor.plan`, `collate_pairs_device`)

    python scripts/color_aug_rate.py [--batches 20] [--out profiles/color_aug_rate.txt]

Batches of 16 crops (8 pairs) of 160 x 160 and 320 x 320 random pixels under an elliptic mask, resized to 224; both routes see the same
crops and the same draws (equal seeds).  One process, the host route first; two warm-up batches per shape on the device."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--img-size", type=int, default=224)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "color_aug_rate.txt"))
    args = ap.parse_args()

    import numpy as np
    import torch

    from unopose_amd import ops
    from unopose_amd.provider import resize_bilinear_u8, to_tensor_normalize
    from unopose_amd.provider_train import AugPlan, ColorAugmentor, collate_pairs_device

    if not torch.cuda.is_available():
        sys.exit("color_aug_rate: needs a GPU (a rate measured elsewhere says nothing)")
    torch.set_num_threads(1)
    dev = torch.device("cuda", 0)
    n = 2 * args.pairs
    lines = ["scripts/color_aug_rate.py on one MI355X: crops finished per second, %d batches of %d crops per shape, resized to %d" % (args.batches, n, args.img_size),
             "host = one core, torch threads 1; device = finish_crops on a pinned collated batch, host clock to the device synchronise",
             "(min / median / max over the batches; the chains differ from batch to batch)"]

    def stats(per_batch_s):
        r = sorted(n / s for s in per_batch_s)
        return "%8.0f / %8.0f / %8.0f crops/s" % (r[0], r[len(r) // 2], r[-1])

    for side in (160, 320):
        yy, xx = np.mgrid[0:side, 0:side]
        mask = ((((yy - side / 2) / (0.45 * side)) ** 2 + ((xx - side / 2) / (0.4 * side)) ** 2) <= 1.0).astype(np.uint8)
        host_s, pack_s, dev_s, lengths = [], [], [], []
        for b in range(-2, args.batches):  # two warm-up batches (first launches load the code objects)
            rng = np.random.default_rng([side, b + 2])
            crops = [rng.integers(0, 256, (side, side, 3), dtype=np.uint8) for _ in range(n)]
            coins = rng.random(n) < 0.8
            aug = ColorAugmentor(1000 * side + b + 2)
            t0 = time.perf_counter()
            for crop, coin in zip(crops, coins):
                rgb = aug.augment_image(crop) if coin else crop
                rgb = rgb * (mask[:, :, None] > 0).astype(np.uint8)
                to_tensor_normalize(resize_bilinear_u8(np.ascontiguousarray(rgb), args.img_size))
            t1 = time.perf_counter()
            aug = ColorAugmentor(1000 * side + b + 2)
            plans = [aug.plan(side, side) if coin else AugPlan() for coin in coins]
            items = [{"rgb_crop": crops[i], "rgb_cropmask": mask, "rgb_plan": plans[i], "tem1_crop": crops[args.pairs + i], "tem1_cropmask": mask,
                      "tem1_plan": plans[args.pairs + i]} for i in range(args.pairs)]
            batch = collate_pairs_device(items, img_size=args.img_size)
            t2 = time.perf_counter()
            batch = {k: v.pin_memory() for k, v in batch.items()}  # the loader's pin thread does this
            torch.cuda.synchronize(dev)
            t3 = time.perf_counter()
            out = ops.finish_crops(batch, dev)
            torch.cuda.synchronize(dev)
            t4 = time.perf_counter()
            assert out["rgb"].shape == (args.pairs, 3, args.img_size, args.img_size)
            if b >= 0:
                host_s.append(t1 - t0), pack_s.append(t2 - t1), dev_s.append(t4 - t3), lengths.append(sum(len(p) for p in plans) / n)
        lines.append("%3d x %3d  host finishing        %s" % (side, side, stats(host_s)))
        lines.append("           device finish_crops   %s   (mean chain length %.1f operators)" % (stats(dev_s), sum(lengths) / len(lengths)))
        lines.append("           worker plan + collate %s" % stats(pack_s))
        lines.append("           medians: device / host = %.1fx; worker share left = 1 / %.1f of the host finishing"
                     % (sorted(host_s)[len(host_s) // 2] / sorted(dev_s)[len(dev_s) // 2], sorted(host_s)[len(host_s) // 2] / sorted(pack_s)[len(pack_s) // 2]))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
