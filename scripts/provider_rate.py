"""Rate of the BOP test provider and of the CLI's image loop, host path against device path (`BOPTestsetOneRef(..., device=...)`).

    python scripts/provider_rate.py ROOT --data DIR --build [--images 50]     write the seeded folder (tests/bop_scenes.py's recipe:
                                                                              480 x 640, 5-15 detections per image) once
                                                              [--dets LO HI]  detections per image (default 5 15)
    python scripts/provider_rate.py ROOT --data DIR --leg provider --path host|device|device-masks
    python scripts/provider_rate.py ROOT --data DIR --leg cli --path host|device|device-masks
    python scripts/provider_rate.py ROOT --data DIR --leg decode [--masks 100]

ROOT is the package root to measure (this tree, or an export of another commit built from source): `unopose_amd` is imported from
there, the scene recipe always from this file's tree.  On a tree whose provider has no `device` argument the device legs print
`"skipped"`; likewise `device-masks` (the run-length masks decoded on the device too, `device_masks=True`) on a tree without it.  One leg = one process; each prints one JSON line.  The profiler is off; every leg makes a warm-up pass first.

  provider  one pass over all items; both paths end with `pts`, `rgb`, `rgb_choose` on the GPU (the host path uploads them, as
            `runner.run_image` does next), the clock stops after a stream synchronise -> items/s, instances/s
  cli       `runner.inference_and_save` over all images at the reference's contract (224 x 224, 2048 / 5000 points, batches of 16
            instances, random `trained_like_` weights), fp32 then bf16 autocast -> images/s
  decode    the first `--masks` detections of the folder (lists and strings as they come): `provider.rle_decode` of each on the host against
            one `ops.rle_decode` for all -- the two kernels between events, and the whole call with packing, upload and the stats readback"""
import argparse
import inspect
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("root")
    ap.add_argument("--data", required=True)
    ap.add_argument("--build", action="store_true")
    ap.add_argument("--images", type=int, default=50)
    ap.add_argument("--dets", type=int, nargs=2, default=(5, 15))
    ap.add_argument("--masks", type=int, default=100)
    ap.add_argument("--leg", choices=("provider", "cli", "decode"))
    ap.add_argument("--path", choices=("host", "device", "device-masks"), default="host")
    ap.add_argument("--label", default=None)
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, os.path.join(HERE, "..", "tests"))
    sys.path.insert(0, root)

    import numpy as np

    import bop_scenes

    meta = os.path.join(args.data, "meta.json")
    if args.build:
        cfg, det_path = bop_scenes.build(args.data, n_images=args.images, dets_per_image=tuple(args.dets), seed=0)
        json.dump(dict(cfg=cfg, det_path=det_path), open(meta, "w"))
        print(json.dumps(dict(built=args.data, images=args.images, dets_per_image=list(args.dets))))
        return 0
    m = json.load(open(meta))
    cfg, det_path = m["cfg"], m["det_path"]

    import torch

    from unopose_amd import provider as P

    assert os.path.abspath(P.__file__).startswith(root + os.sep), (P.__file__, root)
    res = dict(tree=args.label or os.path.basename(root), leg=args.leg, path=args.path)
    has_device = "device" in inspect.signature(P.BOPTestsetOneRef.__init__).parameters
    has_masks = "device_masks" in inspect.signature(P.BOPTestsetOneRef.__init__).parameters
    if (args.path != "host" and not has_device) or ((args.path == "device-masks" or args.leg == "decode") and not has_masks):
        print(json.dumps(dict(res, skipped="this tree's provider has no such path")))
        return 0
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ds = P.BOPTestsetOneRef(cfg, "lm", det_path, **(dict(device=dev) if args.path != "host" else {}),
                            **(dict(device_masks=True) if args.path == "device-masks" else {}))

    if args.leg == "provider":
        def one_pass():
            np.random.seed(1)
            n = 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(len(ds)):
                item = ds[i]
                on_gpu = [item[k].to(dev, non_blocking=True) for k in ("pts", "rgb", "rgb_choose")]
                n += on_gpu[0].shape[0]
            torch.cuda.current_stream().synchronize()
            return time.perf_counter() - t0, n

        one_pass()
        dt, n = one_pass()
        res.update(items=len(ds), instances=n, seconds=round(dt, 4), items_per_s=round(len(ds) / dt, 2), instances_per_s=round(n / dt, 1))
    elif args.leg == "decode":
        from unopose_amd.ops import rle

        segs = [d["segmentation"] for dets in ds.dets.values() for d in dets][:args.masks]
        t0 = time.perf_counter()
        want = np.stack([P.rle_decode(s) for s in segs])
        host_s = time.perf_counter() - t0
        H, W, desc, buf, ints, n_starts = rle.pack_segs(segs)
        up = [torch.from_numpy(np.concatenate([a, np.zeros(1, a.dtype)])).to(dev) for a in (desc.reshape(-1), ints, buf)]
        starts = torch.empty(n_starts, dtype=torch.int32, device=dev)
        stats = torch.empty((len(segs), 6), dtype=torch.int32, device=dev)
        masks = torch.empty((len(segs), H, W), dtype=torch.uint8, device=dev)
        depth = torch.ones((H, W), dtype=torch.float64, device=dev)
        times = {"parse": [], "fill": []}
        for _ in range(12):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            rle.call("unopose_rle_parse", rle.ptr(up[2]), rle.ptr(up[1]), rle.ptr(up[0]), len(segs), H, W, rle.ptr(starts), rle.ptr(stats), rle.stream_ptr(dev))
            ev[1].record()
            rle.call("unopose_rle_fill", rle.ptr(up[0]), rle.ptr(starts), rle.ptr(depth), len(segs), H, W, rle.ptr(masks), rle.ptr(stats), rle.stream_ptr(dev))
            ev[2].record()
            torch.cuda.synchronize()
            times["parse"].append(ev[0].elapsed_time(ev[1]))
            times["fill"].append(ev[1].elapsed_time(ev[2]))
        assert np.array_equal(masks.cpu().numpy(), want)
        calls = []
        for _ in range(6):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rle.rle_decode(segs, dev, depth=depth)
            calls.append(time.perf_counter() - t0)
        med = lambda v: round(float(np.median(v[2:])), 4)  # noqa: E731
        res.update(masks=len(segs), size=[H, W], strings=int(desc[:, 0].sum()), counts=int(desc[:, 3].sum()), string_bytes=len(buf),
                   host_ms=round(host_s * 1e3, 2), host_ms_per_mask=round(host_s * 1e3 / len(segs), 3), parse_kernel_ms=med(times["parse"]),
                   fill_kernel_ms=med(times["fill"]), whole_call_ms=round(float(np.median(calls[2:])) * 1e3, 3))
    else:
        from unopose_amd.model import UNOPose, default_model_cfg
        from unopose_amd.runner import inference_and_save
        from unopose_amd.synthetic import trained_like_

        class Images:
            dets = ds.dets

            def __init__(self, count):
                self.count = count

            def __len__(self):
                return self.count

            def __getitem__(self, i):
                return P.collate_image(ds[i])

        torch.manual_seed(3)
        model = trained_like_(UNOPose(default_model_cfg(feature_extraction=dict(img_size=cfg["img_size"])))).to(dev).eval()
        out = os.path.join(args.data, f"rate_{os.getpid()}.csv")
        for name, amp in (("fp32", False), ("bf16", True)):
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
                np.random.seed(1)
                torch.manual_seed(5)
                inference_and_save(model, Images(min(6, len(ds))), out, instance_batch_size=16, device=dev)  # warm-up
                np.random.seed(1)
                torch.manual_seed(5)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                lines = inference_and_save(model, Images(len(ds)), out, instance_batch_size=16, device=dev)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
            res[name] = dict(images=len(ds), rows=len(lines), seconds=round(dt, 4), images_per_s=round(len(ds) / dt, 2))
        for f in (out, out.replace(".csv", ".json")):
            os.remove(f)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
