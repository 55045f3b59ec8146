"""Draw ground-truth or estimated poses over the images of a BOP split: ``python -m unopose_amd.vis_poses --data-dir D --dataset N --split S``.

What the toolkit's ``scripts/vis_gt_poses.py`` and ``scripts/vis_est_poses.py`` do through ``visualization.vis_object_poses``
(third_party/bop_toolkit/bop_toolkit_lib/visualization.py:93-235), without its OpenGL renderer: the object models are rendered in colour by
the HIP rasteriser (`render.HipColorRenderer`, csrc/raster_color.hip), composed per image on the GPU (`ops.compose_poses`, csrc/vis.hip) --
the nearest pose per pixel, a box around every pose, blended half and half with the photo, and a depth-difference image against the
captured depth -- and written as ``<out>/<dataset>/<split>/<scene:06d>/<im:06d>.<ext>`` and ``..._depth_diff.<ext>`` (JPEG quality 95).
Without ``--results`` the ground truths of the targeted objects are drawn; with it the estimates the scorer would score: the same
selection routine as `bop_eval` (`_walk`: the ``--n-top`` best-scored per image and object, -1 = the targets' instance counts).
Every object gets a colour of the project's own palette (evenly spaced hues); ``--orig-color`` takes the vertex colours of the PLY where
it has them.  Captions (object : ground-truth index or score at each box, the depth statistics on the difference image) are drawn on the
host after the kernels; ``--no-text`` leaves them out.  ``--print-plan`` resolves paths and counts and touches no GPU."""
import argparse
import colorsys
import json
import os
import os.path as osp
import sys

import numpy as np


def palette(obj_ids):
    """One colour per object: hues evenly spaced over the sorted ids -> {obj_id: (r, g, b) in [0, 1]}."""
    ids = sorted(obj_ids)
    return {o: colorsys.hsv_to_rgb(i / float(max(1, len(ids))), 0.75, 1.0) for i, o in enumerate(ids)}


def output_paths(out_dir, dataset, split, scene_id, im_id, ext="jpg"):
    """-> (visualisation, depth-difference image)."""
    base = osp.join(out_dir, dataset, split, f"{scene_id:06d}", f"{im_id:06d}")
    return f"{base}.{ext}", f"{base}_depth_diff.{ext}"


def default_out_dir(results):
    return osp.join(osp.dirname(osp.abspath(results)), "vis") if results else "vis_gt_poses"


def _wanted(key, scene_ids, im_ids):
    return (not scene_ids or key[0] in scene_ids) and (not im_ids or key[1] in im_ids)


def select_poses(data, results=None, n_top=-1, scene_ids=None, im_ids=None):
    """The poses to draw per image -> {(scene_id, im_id): [dict(obj_id, R, t, label)]}, objects in ascending order (a render stack holds
    the poses of one object side by side).  results=None: the ground truths of the targeted objects, in ground-truth order, labelled
    "obj:gt index"; else the rows `bop_eval._walk` picks from `results` (`bop_eval.read_results`), best score first, labelled "obj:score"."""
    from .bop_eval import _walk

    out = {}
    for sid, iid, gts, K, picked in _walk(results or [], data["scene_gt"], data["cameras"], n_top, data["targets"]):
        if not _wanted((sid, iid), scene_ids, im_ids):
            continue
        if results is None:
            poses = [dict(obj_id=g["obj_id"], R=g["R"], t=g["t"], label=f"{g['obj_id']}:{gid}") for gid, g in enumerate(gts) if g["valid"]]
        else:
            poses = [dict(obj_id=o, R=r["R"], t=r["t"], label=f"{o}:{r['score']:.2f}") for o, rows in picked for r in rows]
        out[(sid, iid)] = sorted(poses, key=lambda p: p["obj_id"])  # stable: the order within an object stays
    return out


def render_poses(renderer, poses, K):
    """Renders of one image's poses in one stack -> depths (P,H,W), rgbs (P,H,W,3) on the renderer's device: one `render_batch` per
    object into its slice."""
    import torch

    P = len(poses)
    depths = torch.empty(P, renderer.H, renderer.W, dtype=torch.float32, device=renderer.device)
    rgbs = torch.empty(P, renderer.H, renderer.W, 3, dtype=torch.uint8, device=renderer.device)
    k4 = [K[0, 0], K[1, 1], K[0, 2], K[1, 2]]
    a = 0
    while a < P:
        b = a
        while b < P and poses[b]["obj_id"] == poses[a]["obj_id"]:
            b += 1
        renderer.render_batch(poses[a]["obj_id"], np.stack([p["R"] for p in poses[a:b]]), np.stack([p["t"] for p in poses[a:b]]), k4,
                              out=(depths[a:b], rgbs[a:b]))
        a = b
    return depths, rgbs


def _caption(image, lines, at):
    from PIL import Image, ImageDraw

    im = Image.fromarray(image)
    draw = ImageDraw.Draw(im)
    x, y = at
    for line in lines:
        draw.text((x, y), line, fill=(255, 255, 255))
        y += 11
    return np.asarray(im)


def _save(path, image, ext):
    from PIL import Image

    os.makedirs(osp.dirname(path), exist_ok=True)
    Image.fromarray(image).save(path, **(dict(quality=95) if ext == "jpg" else {}))


def _photo(files, folder, sid, iid, hw):
    im = files.colour(folder, sid, iid)
    if im.ndim == 2:
        im = np.repeat(im[:, :, None], 3, axis=2)
    im = np.ascontiguousarray(im[:, :, :3])
    if im.shape[:2] != hw:
        raise RuntimeError(f"vis_poses: colour image {sid}/{iid} is {im.shape[:2]}, the depth image {hw}")
    return im


def make_renderer(data, models_dir, device, orig_color=False):
    """A `HipColorRenderer` of the dataset's image size with its targeted objects: palette colours, or with `orig_color` the PLY's vertex
    colours where the file has them."""
    from .bop_eval import read_ply_colors
    from .render import HipColorRenderer

    W, H = data["im_size"]
    ren = HipColorRenderer(W, H, device=device)
    pal = palette(data["models"])
    for obj_id, m in data["models"].items():
        colors = read_ply_colors(osp.join(models_dir, f"obj_{obj_id:06d}.ply"))["colors"] if orig_color else None
        if colors is not None:
            ren.add_object(obj_id, m["verts"], m["faces"], colors=colors)
        else:
            ren.add_object(obj_id, m["verts"], m["faces"], surf_color=pal[obj_id])
    return ren


def visualise(data, split_folder, by_image, renderer, out_dir, dataset, split, resolve_visib=True, depth_diff=True, text=True, ext="jpg", delta=15.0):
    """Render, compose and write every image of `by_image` (`select_poses`) -> list of the files written.  An image without a pose to draw
    is written too (the photo at half brightness), as the toolkit's loop does."""
    import torch

    from .ops.vis import compose_poses
    from .provider import SceneFiles

    files, written, dev = SceneFiles(), [], renderer.device
    for (sid, iid), poses in by_image.items():
        K = data["cameras"][sid][iid]
        captured = np.ascontiguousarray(np.asarray(data["depth_images"][sid][iid], np.float32)) if depth_diff else None
        photo = _photo(files, split_folder, sid, iid, (renderer.H, renderer.W))
        if poses:
            depths, rgbs = render_poses(renderer, poses, K)
        else:  # a stack of one empty render
            depths = torch.zeros(1, renderer.H, renderer.W, dtype=torch.float32, device=dev)
            rgbs = torch.zeros(1, renderer.H, renderer.W, 3, dtype=torch.uint8, device=dev)
        vis, boxes, _, diff, stats = compose_poses(rgbs, depths, torch.from_numpy(photo).to(dev), None if captured is None else torch.from_numpy(captured).to(dev),
                                                   resolve_visib=resolve_visib, delta=delta)
        vis = vis.cpu().numpy()
        if text:
            for p, box in zip(poses, boxes):
                if box is not None:
                    vis = _caption(vis, [p["label"]], (box[0] + 2, box[1]))
        rgb_path, diff_path = output_paths(out_dir, dataset, split, sid, iid, ext)
        _save(rgb_path, vis, ext)
        written.append(rgb_path)
        if diff is not None:
            diff = diff.cpu().numpy()
            if text and stats is not None:
                diff = _caption(diff, [f"min diff:{stats['min']:.3f}", f"max diff:{stats['max']:.3f}", f"mean diff:{stats['mean']:.3f}"], (3, 0))
            _save(diff_path, diff, ext)
            written.append(diff_path)
    return written


def vis_dataset(root, name, split, results=None, targets_filename="test_targets_bop19.json", scene_ids=None, im_ids=None, n_top=-1, out_dir=None,
                orig_color=False, resolve_visib=True, depth_diff=True, text=True, ext="jpg", device="cuda", delta=None):
    """The command as a function -> list of the files written.  `results`: a result CSV (`bop_eval.read_results`) or None for the ground
    truth; `delta` defaults to the dataset's visibility tolerance (15 mm, ITODD 5 mm)."""
    from .bop_eval import VSD_DELTA, VSD_DELTAS, _cuda_device, dataset_paths, load_dataset, read_results

    if ext not in ("jpg", "png"):
        raise ValueError(f"vis_poses: ext {ext!r} (jpg or png)")
    data = load_dataset(root, name, split, targets_filename)
    paths = dataset_paths(root, name, split, targets_filename)
    by_image = select_poses(data, None if results is None else read_results(results), n_top, scene_ids, im_ids)
    if not by_image:
        return []
    renderer = make_renderer(data, paths["models"], _cuda_device(device), orig_color)
    return visualise(data, paths["split"], by_image, renderer, out_dir or default_out_dir(results), name, split, resolve_visib, depth_diff, text, ext,
                     VSD_DELTAS.get(name, VSD_DELTA) if delta is None else delta)


def plan(root, name, split, results=None, targets_filename="test_targets_bop19.json", scene_ids=None, im_ids=None, n_top=-1, out_dir=None, ext="jpg",
         depth_diff=True):
    """What `--print-plan` prints: the paths read and written and, where the targets file (and the result file) exist, how many images and
    estimates the filters leave.  No GPU, no image is read."""
    from .bop_eval import dataset_paths, read_results
    from .provider import load_json

    out_dir = out_dir or default_out_dir(results)
    p = dict(mode="gt" if results is None else "est", paths=dataset_paths(root, name, split, targets_filename), results=results, out_dir=out_dir, ext=ext,
             n_top=n_top, depth_diff=bool(depth_diff), n_images=None, n_estimates=None, first_files=None)
    if osp.exists(p["paths"]["targets"]):
        keys = sorted({(int(t["scene_id"]), int(t["im_id"])) for t in load_json(p["paths"]["targets"])})
        keys = [k for k in keys if _wanted(k, scene_ids, im_ids)]
        p["n_images"] = len(keys)
        if keys:
            p["first_files"] = list(output_paths(out_dir, name, split, keys[0][0], keys[0][1], ext))[:2 if depth_diff else 1]
        if results is not None and osp.exists(results):
            p["n_estimates"] = sum((r["scene_id"], r["im_id"]) in set(keys) for r in read_results(results))
    return p


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m unopose_amd.vis_poses", description=__doc__.split("\n\n")[0])
    ap.add_argument("--data-dir", required=True)
    ap.add_argument("--dataset", required=True)
    ap.add_argument("--split", required=True)
    ap.add_argument("--results", help="a result CSV: draw its estimates instead of the ground truth")
    ap.add_argument("--targets", default="test_targets_bop19.json", help="targets file name under the dataset folder")
    ap.add_argument("--scene-ids", type=int, nargs="*")
    ap.add_argument("--im-ids", type=int, nargs="*")
    ap.add_argument("--n-top", type=int, default=-1, help="estimates per image and object (-1: the targets' instance counts, 0: all)")
    ap.add_argument("--out", help="output folder (default: vis/ beside the CSV, vis_gt_poses/ for the ground truth)")
    ap.add_argument("--orig-color", action="store_true", help="vertex colours of the PLY where it has them")
    ap.add_argument("--no-resolve-visib", action="store_true", help="sum the renders instead of showing the nearest pose per pixel")
    ap.add_argument("--no-depth-diff", action="store_true")
    ap.add_argument("--no-text", action="store_true")
    ap.add_argument("--ext", choices=("jpg", "png"), default="jpg")
    ap.add_argument("--print-plan", action="store_true")
    a = ap.parse_args(argv)
    if a.print_plan:
        print(json.dumps(plan(a.data_dir, a.dataset, a.split, a.results, a.targets, a.scene_ids, a.im_ids, a.n_top, a.out, a.ext, not a.no_depth_diff)))
        return 0
    files = vis_dataset(a.data_dir, a.dataset, a.split, a.results, a.targets, a.scene_ids, a.im_ids, a.n_top, a.out, a.orig_color, not a.no_resolve_visib,
                        not a.no_depth_diff, not a.no_text, a.ext)
    print(f"{len(files)} files -> {a.out or default_out_dir(a.results)}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
