"""Ground-truth visibility of a BOP dataset: `scene_gt_info.json`, `mask/` and `mask_visib/` without the toolkit's OpenGL renderer.

The reference makes these files with `lib/pysixd/scripts/calc_gt_info.py` and `third_party/bop_toolkit/scripts/calc_gt_masks.py`: the
object model is rendered in each ground-truth pose on a canvas of 3W x 3H pixels whose principal point is moved by (W, H), so that the part
of the silhouette outside the image is counted; the image is the central crop.  From the rendered and the test depth come
`px_count_all` (silhouette pixels on the canvas), `px_count_valid` (silhouette pixels in the image with a depth measurement),
`px_count_visib` (pixels of the "bop19" visibility mask, `bop_eval._visib_mask`), `visib_fract = px_count_visib / px_count_all`, the
bounding boxes `bbox_obj` (of the whole silhouette, may leave the image) and `bbox_visib`, and the two masks.

`gt_counts_host` / `gt_info_host` are the numpy specification for one ground truth.  `compute_gt_info` does a whole dataset: on the
host with any `render_object` renderer, or -- with a CUDA `device` -- on maps that never leave the GPU (`render.HipDepthRenderer` on the
canvas, csrc/gtinfo.hip through `ops.score.gt_visibility`; equal integers, equal masks).  `write_gt_info` writes the toolkit's files,
`python -m unopose_amd.gt_info` is its command line.  `bop_eval.average_recall(..., gt_info=...)` uses the result for the toolkit's rule
of which ground truths count."""
import argparse
import json
import os
import os.path as osp
import sys

import numpy as np

from .bop_eval import DEVICE_CHUNK_BYTES, VSD_DELTA, VSD_DELTAS, _cuda_device, _visib_mask, depth_to_dist

INT_MAX, INT_MIN = np.iinfo(np.int32).max, np.iinfo(np.int32).min
INFO_KEYS = ("px_count_all", "px_count_valid", "px_count_visib", "visib_fract", "bbox_obj", "bbox_visib")
WRITE_IMAGES = 16  # images `write_gt_info` hands to `compute_gt_info` at a time: their masks are held on the host until written


def _extent(mask, x0=0, y0=0):
    """min x, min y, max x, max y of a mask's pixels, shifted by (-x0, -y0); INT_MAX / INT_MIN for an empty mask."""
    ys, xs = mask.nonzero()
    if len(xs) == 0:
        return [INT_MAX, INT_MAX, INT_MIN, INT_MIN]
    return [int(xs.min()) - x0, int(ys.min()) - y0, int(xs.max()) - x0, int(ys.max()) - y0]


def gt_counts_host(depth_test, canvas_depth, K, delta):
    """calc_gt_info.py:110-159 for one ground truth.  depth_test (H, W) in mm; canvas_depth (3H, 3W): the object rendered with the principal
    point at (cx + W, cy + H); K (3, 3) of the image; delta: the visibility tolerance in mm.
    -> (the 11 integers of `ops.score.GT_COLUMNS`, mask (H, W) bool = dist_gt > 0, mask_visib (H, W) bool)."""
    depth_test, canvas_depth, K = np.asarray(depth_test), np.asarray(canvas_depth), np.asarray(K, np.float64).reshape(3, 3)
    H, W = depth_test.shape
    if canvas_depth.shape != (3 * H, 3 * W):
        raise ValueError(f"gt_info: a canvas of {canvas_depth.shape} for an image of {(H, W)}: expected {(3 * H, 3 * W)}")
    dist_gt, dist_test = depth_to_dist(canvas_depth[H:2 * H, W:2 * W], K), depth_to_dist(depth_test, K)
    visib = _visib_mask(dist_test, dist_gt, delta)
    large, mask = canvas_depth > 0, dist_gt > 0
    row = [int(large.sum()), int((dist_test[mask] > 0).sum()), int(visib.sum())] + _extent(large, W, H) + _extent(visib)
    return row, mask, visib


def info_from_counts(row):
    """The dictionary the toolkit stores (calc_gt_info.py:140-171) from the 11 integers: `calc_2d_bbox` is [x, y, xmax - xmin, ymax - ymin],
    unclipped, and both boxes are [-1, -1, -1, -1] when nothing is visible."""
    row = [int(v) for v in row]
    n_all, n_valid, n_visib = row[:3]
    box = lambda e: [e[0], e[1], e[2] - e[0], e[3] - e[1]] if n_visib > 0 else [-1, -1, -1, -1]  # noqa: E731
    return dict(px_count_all=n_all, px_count_valid=n_valid, px_count_visib=n_visib, visib_fract=float(n_visib / float(n_all)) if n_all > 0 else 0.0,
                bbox_obj=box(row[3:7]), bbox_visib=box(row[7:11]))


def gt_info_host(depth_test, canvas_depth, K, delta):
    """The numpy specification for one ground truth -> ({px_count_all, px_count_valid, px_count_visib, visib_fract, bbox_obj, bbox_visib},
    mask, mask_visib), the masks (H, W) bool."""
    row, mask, visib = gt_counts_host(depth_test, canvas_depth, K, delta)
    return info_from_counts(row), mask, visib


def _flat(scene_gt, cameras):
    """Every ground truth in file order -> [(scene_id, im_id, gt_id, ground truth, K)]."""
    return [(sid, iid, gid, g, np.asarray(cameras[sid][iid], np.float64).reshape(3, 3))
            for sid, ims in scene_gt.items() for iid, gts in ims.items() for gid, g in enumerate(gts)]


def _canvas_k4(K, W, H):
    return [K[0, 0], K[1, 1], K[0, 2] + W, K[1, 2] + H]


def _test_depth(depth_images, sid, iid, hw=None):
    d = np.ascontiguousarray(np.asarray(depth_images[sid][iid], dtype=np.float32))
    if d.ndim != 2 or (hw is not None and d.shape != hw):
        raise RuntimeError(f"gt_info: depth image {sid}/{iid} is {d.shape}" + (f", the renderer's canvas is for {hw}" if hw is not None else ""))
    return d


def _host_rows(items, depth_images, renderer, delta, masks):
    out = []
    for sid, iid, gid, g, K in items:
        depth = _test_depth(depth_images, sid, iid)
        H, W = depth.shape
        canvas = np.asarray(renderer.render_object(g["obj_id"], g["R"], g["t"], *_canvas_k4(K, W, H))["depth"])
        if canvas.shape != (3 * H, 3 * W):
            raise RuntimeError(f"gt_info: the renderer draws {canvas.shape}, the canvas of image {sid}/{iid} is {(3 * H, 3 * W)}")
        row, mask, visib = gt_counts_host(depth, canvas, K, delta)
        out.append((row, (mask, visib) if masks else None))
    return out


def _device_rows(items, depth_images, renderer, delta, device, masks, chunk_bytes):
    """`_host_rows` on maps that stay on the GPU.  Ground truths are taken in order, in chunks whose maps fit `chunk_bytes`: a canvas map is
    9 images, a test image 1, the two uint8 masks half of one.  Per chunk: the test depths it does not share with the previous chunk are
    uploaded, its ground truths are rendered into one canvas stack with one `render_batch` per object, one `gt_visibility` launch counts
    them, and the integers (and masks) are read back once.  -> (rows, number of chunks)."""
    import torch

    from .ops.score import gt_visibility
    from .render import HipDepthRenderer

    dev = _cuda_device(device)
    if not isinstance(renderer, HipDepthRenderer) or _cuda_device(renderer.device) != dev:
        raise RuntimeError(f"gt_info: the device route needs a render.HipDepthRenderer on {dev}, not {type(renderer).__name__}"
                           f"{' on ' + str(renderer.device) if isinstance(renderer, HipDepthRenderer) else ''}; there is no fallback to the host route")
    if renderer.H % 3 or renderer.W % 3:
        raise RuntimeError(f"gt_info: the renderer's {renderer.H} x {renderer.W} is no 3H x 3W canvas")
    H, W = renderer.H // 3, renderer.W // 3
    budget = max(10.0, int(chunk_bytes) / (4.0 * H * W))  # in images; one ground truth with its test image at least
    per_gt = 9.0 + (0.5 if masks else 0.0)
    chunks, used, images = [], budget + 1, set()
    for item in items:
        need = per_gt + ((item[0], item[1]) not in images)
        if used + need > budget or len(chunks[-1]) == 65535:
            chunks.append([])
            used, images = 0.0, set()
            need = per_gt + 1
        used += need
        images.add((item[0], item[1]))
        chunks[-1].append(item)
    out, on_dev = [], {}
    for chunk in chunks:
        order = list(dict.fromkeys((it[0], it[1]) for it in chunk))
        on_dev = {k: v for k, v in on_dev.items() if k in order}  # an image shared with the previous chunk is not uploaded again
        for sid, iid in order:
            if (sid, iid) not in on_dev:
                on_dev[(sid, iid)] = torch.from_numpy(_test_depth(depth_images, sid, iid, (H, W))).to(dev)
        test = on_dev[order[0]][None] if len(order) == 1 else torch.stack([on_dev[k] for k in order])
        by_obj = {}
        for n, it in enumerate(chunk):
            by_obj.setdefault(it[3]["obj_id"], []).append(n)
        canvas = torch.empty(len(chunk), 3 * H, 3 * W, dtype=torch.float32, device=dev)
        canvas_index, at = np.empty(len(chunk), np.int64), 0
        for obj_id, members in by_obj.items():  # the object's ground truths are rendered into a run of the stack
            renderer.render_batch(obj_id, np.stack([np.asarray(chunk[n][3]["R"], np.float64).reshape(3, 3) for n in members]),
                                  np.stack([np.asarray(chunk[n][3]["t"], np.float64).reshape(3) for n in members]),
                                  np.asarray([_canvas_k4(chunk[n][4], W, H) for n in members]), out=canvas[at:at + len(members)])
            canvas_index[members] = np.arange(at, at + len(members))
            at += len(members)
        K4 = np.asarray([[it[4][0, 0], it[4][1, 1], it[4][0, 2], it[4][1, 2]] for it in chunk])
        res = gt_visibility(test, canvas, K4, delta, image_index=[order.index((it[0], it[1])) for it in chunk], canvas_index=canvas_index, masks=masks)
        if masks:
            rows, m, mv = res[0].cpu().numpy(), res[1].cpu().numpy() > 0, res[2].cpu().numpy() > 0
            out += [(rows[n].tolist(), (m[n], mv[n])) for n in range(len(chunk))]
        else:
            out += [(r.tolist(), None) for r in res.cpu().numpy()]
        del canvas, res  # the maps are released with the chunk
    return out, len(chunks)


def compute_gt_info(scene_gt, cameras, depth_images, renderer, delta, device=None, masks=False, chunk_bytes=DEVICE_CHUNK_BYTES):
    """The toolkit's ground-truth info for every ground truth of `scene_gt` (layouts as in `bop_eval.average_recall`: scene_gt[scene_id][im_id]
    = [{"obj_id", "R", "t"}], cameras[scene_id][im_id] = K, depth_images[scene_id][im_id] = depth in mm).
    -> gt_info[scene_id][im_id] = [{px_count_all, px_count_valid, px_count_visib, visib_fract, bbox_obj, bbox_visib}], one per ground truth;
    with masks=True -> (gt_info, gt_masks) where gt_masks[scene_id][im_id] = [(mask, mask_visib)], (H, W) bool arrays.
    Without `device`: the host route, numpy on the depth maps of any `renderer` whose `render_object(obj_id, R, t, fx, fy, cx, cy)` draws the
    3W x 3H canvas.  With a CUDA `device`: `renderer` is a `render.HipDepthRenderer(3W, 3H)` on that device holding the objects; the canvas maps
    never leave the GPU and at most `chunk_bytes` of maps exist at a time (`_device_rows`).  The two routes give equal results."""
    items = _flat(scene_gt, cameras)
    if device is None:
        rows = _host_rows(items, depth_images, renderer, delta, masks)
    else:
        rows = _device_rows(items, depth_images, renderer, delta, device, masks, chunk_bytes)[0] if items else []
    info = {sid: {iid: [None] * len(gts) for iid, gts in ims.items()} for sid, ims in scene_gt.items()}
    held = {sid: {iid: [None] * len(gts) for iid, gts in ims.items()} for sid, ims in scene_gt.items()}
    for (sid, iid, gid, _, _), (row, m) in zip(items, rows):
        info[sid][iid][gid], held[sid][iid][gid] = info_from_counts(row), m
    return (info, held) if masks else info


def gt_info_path(root, name, split, scene_id):
    return osp.join(root, name, split, f"{scene_id:06d}", "scene_gt_info.json")


def load_gt_info(root, name, split, scene_ids):
    """`scene_gt_info.json` of the scenes -> gt_info[scene_id][im_id] = list of the toolkit's dictionaries.  A missing file is an error that
    names it: nothing is computed in its place."""
    out = {}
    for sid in scene_ids:
        path = gt_info_path(root, name, split, sid)
        if not osp.exists(path):
            raise FileNotFoundError(f"{path} is missing: write it with `python -m unopose_amd.gt_info`, or score with gt_visibility=\"compute\" "
                                    "(the visibility is then computed for the scored images)")
        with open(path) as f:
            out[sid] = {int(k): v for k, v in json.load(f).items()}
    return out


def _save_json(path, info):
    """One image per line, keys as strings, as the toolkit's `inout.save_json` lays scene files out."""
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f'  "{iid}": {json.dumps(info[iid])}' for iid in sorted(info)) + "\n}")


def write_gt_info(root, name, split, scene_ids=None, masks=True, device="cuda", delta=None, overwrite=False, chunk_bytes=DEVICE_CHUNK_BYTES,
                  renderer=None):
    """Write `<root>/<name>/<split>/<scene>/scene_gt_info.json` and, with `masks`, `mask/` and `mask_visib/<im:06d>_<gt:06d>.png` (uint8 0 / 255)
    for every image of the scenes' `scene_gt.json` -- not only the targets.  Models come from `models_eval/` (the objects the scenes show),
    depth from `depth/` times `depth_scale`.  `device`: the GPU of the device route, None = the host route (numpy; only the rasteriser runs on
    the current GPU -- or nothing does, with a `renderer` of the 3W x 3H canvas handed in: `add_object(obj_id, verts, faces)`, `render_object`).  `delta` defaults to the dataset's VSD tolerance (15 mm, ITODD 5 mm), the value the BOP files were made with.
    Existing files are an error unless `overwrite`; then, once every mask of a scene is written, each other `*.png` in its two mask folders is
    removed, so that no mask of another tool or of an earlier `scene_gt.json` is left for the provider to read -- and a run that fails midway
    (a missing model, a depth image of another size) has deleted nothing.  -> gt_info[scene_id][im_id] as written."""
    from .bop_eval import DepthImages, read_ply
    from .provider import load_json

    base = osp.join(root, name, split)
    if scene_ids is None:
        scene_ids = sorted(int(d) for d in os.listdir(base) if d.isdigit() and osp.exists(osp.join(base, d, "scene_gt.json")))
    scene_ids = [int(s) for s in scene_ids]
    delta = VSD_DELTAS.get(name, VSD_DELTA) if delta is None else delta
    scene_gt, cameras, scales = {}, {}, {}
    for sid in scene_ids:
        folder = osp.join(base, f"{sid:06d}")
        taken = [p for p in [gt_info_path(root, name, split, sid)] + ([osp.join(folder, "mask"), osp.join(folder, "mask_visib")] if masks else [])
                 if osp.exists(p) and (osp.isfile(p) or os.listdir(p))]
        if taken and not overwrite:
            raise FileExistsError(f"gt_info: {', '.join(taken)} exist(s); pass overwrite=True (--overwrite) to replace")
        gt, cam = load_json(osp.join(folder, "scene_gt.json")), load_json(osp.join(folder, "scene_camera.json"))
        scene_gt[sid] = {int(i): [dict(obj_id=int(g["obj_id"]), R=np.asarray(g["cam_R_m2c"], np.float64).reshape(3, 3),
                                       t=np.asarray(g["cam_t_m2c"], np.float64).reshape(3)) for g in gts] for i, gts in gt.items()}
        cameras[sid] = {i: np.asarray(cam[str(i)]["cam_K"], np.float64).reshape(3, 3) for i in scene_gt[sid]}
        scales[sid] = {i: float(cam[str(i)].get("depth_scale", 1.0)) for i in scene_gt[sid]}
    depth_images = DepthImages(base, scales)
    first = next(((sid, iid) for sid in scene_ids for iid in scene_gt[sid]), None)
    if first is None:
        return {}
    H, W = depth_images[first[0]][first[1]].shape
    dev = _cuda_device(device) if device is not None else None
    if renderer is None:
        import torch

        from .render import HipDepthRenderer

        renderer = HipDepthRenderer(3 * W, 3 * H, device=dev if dev is not None else torch.device("cuda", torch.cuda.current_device()))
    for obj_id in sorted({g["obj_id"] for ims in scene_gt.values() for gts in ims.values() for g in gts}):
        mesh = read_ply(osp.join(root, name, "models_eval", f"obj_{obj_id:06d}.ply"))
        renderer.add_object(obj_id, mesh["pts"], mesh["faces"])
    out = {}
    for sid in scene_ids:
        folder, im_ids = osp.join(base, f"{sid:06d}"), sorted(scene_gt[sid])
        out[sid] = {}
        if masks:
            from PIL import Image

            for sub in ("mask", "mask_visib"):
                os.makedirs(osp.join(folder, sub), exist_ok=True)
        fresh = set()
        for a in range(0, len(im_ids), WRITE_IMAGES):
            part = {sid: {i: scene_gt[sid][i] for i in im_ids[a:a + WRITE_IMAGES]}}
            res = compute_gt_info(part, cameras, depth_images, renderer, delta, device=dev, masks=masks, chunk_bytes=chunk_bytes)
            info, held = res if masks else (res, None)
            out[sid].update(info[sid])
            if masks:
                for iid, pairs in held[sid].items():
                    for gid, (m, mv) in enumerate(pairs):
                        fresh.add(f"{iid:06d}_{gid:06d}.png")
                        Image.fromarray(m.astype(np.uint8) * 255).save(osp.join(folder, "mask", f"{iid:06d}_{gid:06d}.png"))
                        Image.fromarray(mv.astype(np.uint8) * 255).save(osp.join(folder, "mask_visib", f"{iid:06d}_{gid:06d}.png"))
        for sub in ("mask", "mask_visib") if masks else ():  # leftovers exist only with overwrite: the check above refused otherwise
            for old in os.listdir(osp.join(folder, sub)):
                if old.endswith(".png") and old not in fresh:
                    os.remove(osp.join(folder, sub, old))
        _save_json(gt_info_path(root, name, split, sid), out[sid])
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m unopose_amd.gt_info", description="Write scene_gt_info.json, mask/ and mask_visib/ of a BOP dataset split "
                                 "(the toolkit's calc_gt_info.py and calc_gt_masks.py) with the HIP rasteriser and visibility kernel.")
    ap.add_argument("--data-dir", required=True, help="the folder that holds the dataset folder")
    ap.add_argument("--dataset", required=True)
    ap.add_argument("--split", required=True)
    ap.add_argument("--scenes", type=int, nargs="*", default=None, help="scene ids (default: every scene of the split with a scene_gt.json)")
    ap.add_argument("--no-masks", action="store_true", help="write scene_gt_info.json only")
    ap.add_argument("--host", action="store_true", help="numpy on the HIP renders instead of the visibility kernel, for comparison")
    ap.add_argument("--overwrite", action="store_true")
    ap.add_argument("--delta", type=float, default=None, help="visibility tolerance in mm (default: 15, ITODD 5)")
    args = ap.parse_args(argv)
    out = write_gt_info(args.data_dir, args.dataset, args.split, scene_ids=args.scenes or None, masks=not args.no_masks, device=None if args.host else "cuda",
                        delta=args.delta, overwrite=args.overwrite)
    print("%d ground truths in %d images of %d scenes -> %s" % (sum(len(g) for ims in out.values() for g in ims.values()), sum(len(ims) for ims in out.values()),
                                                               len(out), osp.join(args.data_dir, args.dataset, args.split)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
