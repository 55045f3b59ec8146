"""Rate of `python -m unopose_amd.coco_gt` on one scene, the device route (ops.rle_encode) against `--host` (numpy).

    python scripts/coco_gt_rate.py DIR

writes the reference scene of tests/bop_scenes.py's recipe under DIR (15 images of 480 x 640, 23 ground truths after
tests/gt_info_case.py's `extend_bop_scenes`), its masks and `scene_gt_info.json` with `unopose_amd.gt_info`, then times
`coco_gt.write_coco_gt` over the scene for both routes (reading the mask files included; one warm-up pass each, the median of five) and
the encoding alone on the same masks held in memory.  Prints one JSON line."""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, os.path.join(HERE, ".."))


def main():
    import numpy as np
    import torch

    import bop_scenes
    import gt_info_case
    from unopose_amd import coco_gt, gt_info
    from unopose_amd.provider import read_image

    root = sys.argv[1]
    bop_scenes.build(root, n_images=1, dets_per_image=(1, 1))
    _, sid = gt_info_case.extend_bop_scenes(root)
    gt_info.write_gt_info(root, "lm", "test", scene_ids=[sid], overwrite=True)
    folder = os.path.join(root, "lm", "test", f"{sid:06d}", "mask_visib")
    masks = np.stack([read_image(os.path.join(folder, f)) > 0 for f in sorted(os.listdir(folder))])
    res = dict(scene=sid, size=list(masks.shape[1:]), masks=len(masks))

    def median_of(fn, n=5):
        fn()
        out = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append(time.perf_counter() - t0)
        return float(np.median(out))

    for name, device in (("host", None), ("device", "cuda")):
        whole = median_of(lambda: coco_gt.write_coco_gt(root, "lm", "test", scene_ids=[sid], device=device, force=True))
        coco = json.load(open(coco_gt.coco_path(root, "lm", "test", sid)))
        enc = median_of(lambda: coco_gt.encode_masks(masks, device))
        res[name] = dict(images=len(coco["images"]), annotations=len(coco["annotations"]), seconds=round(whole, 4),
                         images_per_s=round(len(coco["images"]) / whole, 1), encode_only_ms=round(enc * 1e3, 3),
                         encode_only_masks_per_s=round(len(masks) / enc, 1))
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
