"""Render object-model training views as a BOP split: bop_toolkit's scripts/render_train_imgs.py on the HIP rasterisers.

    python -m unopose_amd.render_train --data-dir D --dataset N --radii 400 [--obj-ids 1 5] [--min-views 1000] [--mode hinterstoisser]
        [--azimuth-range A0 A1] [--elev-range E0 E1] [--ssaa 4] [--shading phong] [--ambient 0.5] [--models models] [--out DIR]
        [--host] [--force] [--check]

Every model `D/N/<models>/obj_XXXXXX.ply` (texture images beside it) is rendered from the views of `view_sampler.sample_views` on a sphere of
each radius, with the camera of `D/N/camera.json`, into
    OUT/{obj:06d}/rgb/{im:06d}.png       the shaded colour render: `render.HipShadedRenderer` (csrc/raster_shade.hip), supersampled `ssaa` times
    OUT/{obj:06d}/depth/{im:06d}.png     uint16 round(depth / depth_scale) of `render.HipDepthRenderer` at the camera's own resolution
    OUT/{obj:06d}/scene_camera.json      cam_K, depth_scale, view_level per image
    OUT/{obj:06d}/scene_gt.json          cam_R_m2c, cam_t_m2c, obj_id per image
in the toolkit's text format; `im_id` runs on across the radii.  OUT defaults to `D/N/train_render`.  `gt_info` and `coco_gt` finish such
a split.  The ranges default to the whole sphere and `--radii` has no default: the toolkit's per-dataset constants are not carried over.
`view_level` is `levels[view number]` of the UNFILTERED level list, as the toolkit's script writes it (unopose_amd/view_sampler.py).
A model is coloured by its texture where the PLY names one and has per-vertex uv, else by its vertex colours, else mid grey.

--host renders with the numpy forms of the two kernels (unopose_amd/shade_host.py) and writes the same files, byte for byte.
--check renders and compares every file with the one on disk, writes nothing and exits 1 on a difference (a missing, changed or surplus file).
An existing object folder is an error without --force, which replaces the folder."""
import argparse
import io
import json
import os
import os.path as osp
import shutil
import sys

import numpy as np

from .gt_info import _save_json
from .view_sampler import TWO_PI, sample_views

RENDER_VIEWS = 64  # views rendered and encoded at a time


def read_camera(path):
    """camera.json -> dict(K (3,3), depth_scale, im_size (W, H))."""
    with open(path) as f:
        c = json.load(f)
    K = np.array([[c["fx"], 0.0, c["cx"]], [0.0, c["fy"], c["cy"]], [0.0, 0.0, 1.0]])
    return dict(K=K, depth_scale=float(c["depth_scale"]), im_size=(int(c["width"]), int(c["height"])))


def load_model(models_dir, obj_id):
    """The model and what colours it -> keyword arguments of the shaded renderer's `add_object`."""
    from PIL import Image

    from .bop_eval import read_ply_model

    m = read_ply_model(osp.join(models_dir, f"obj_{obj_id:06d}.ply"))
    kw = dict(verts=m["pts"], faces=m["faces"], normals=m["normals"])
    if m["texture_file"] is not None and m["texture_uv"] is not None:
        kw.update(texture=np.asarray(Image.open(osp.join(models_dir, m["texture_file"])).convert("RGB")), texture_uv=m["texture_uv"])
    elif m["colors"] is not None:
        kw["colors"] = m["colors"]
    return kw


def object_views(radii, min_views, mode, azimuth_range, elev_range):
    """The views of one object in image order -> Rs (n,3,3), ts (n,3), view levels."""
    Rs, ts, levels = [], [], []
    for radius in radii:
        views, all_levels = sample_views(min_views, radius, azimuth_range, elev_range, mode)
        for view_id, view in enumerate(views):
            Rs.append(view["R"])
            ts.append(view["t"].reshape(3))
            levels.append(int(all_levels[view_id]))  # the toolkit's indexing: the unfiltered list by the filtered number
    return np.array(Rs).reshape(-1, 3, 3), np.array(ts).reshape(-1, 3), levels


def _png(array):
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(array).save(buf, format="PNG")
    return buf.getvalue()


def object_files(obj_id, Rs, ts, levels, cam, ren_rgb, ren_depth):
    """Generator of (path relative to the object folder, content) for one object: the PNGs in image order as bytes, then the two scene files
    as the dictionaries `_json_bytes` turns into the toolkit's text."""
    K = cam["K"]
    k4 = [K[0, 0], K[1, 1], K[0, 2], K[1, 2]]
    host = lambda x: x if isinstance(x, np.ndarray) else x.cpu().numpy()  # noqa: E731
    for a in range(0, len(Rs), RENDER_VIEWS):
        rgb = host(ren_rgb.render_batch(obj_id, Rs[a:a + RENDER_VIEWS], ts[a:a + RENDER_VIEWS], k4))
        depth = host(ren_depth.render_batch(obj_id, Rs[a:a + RENDER_VIEWS], ts[a:a + RENDER_VIEWS], k4))
        scaled = np.round(depth.astype(np.float32) / np.float32(cam["depth_scale"]))  # in float32, as the script divides its float32 render
        if scaled.max(initial=0) > 65535:
            raise RuntimeError(f"render_train: object {obj_id}: depth / depth_scale = {scaled.max()} does not fit 16 bits")
        for i in range(len(rgb)):
            yield osp.join("rgb", f"{a + i:06d}.png"), _png(rgb[i])
            yield osp.join("depth", f"{a + i:06d}.png"), _png(scaled[i].astype(np.uint16))
    scene_camera = {i: {"cam_K": K.flatten().tolist(), "depth_scale": cam["depth_scale"], "view_level": levels[i]} for i in range(len(Rs))}
    scene_gt = {i: [{"cam_R_m2c": Rs[i].flatten().tolist(), "cam_t_m2c": ts[i].flatten().tolist(), "obj_id": int(obj_id)}] for i in range(len(Rs))}
    yield "scene_camera.json", scene_camera
    yield "scene_gt.json", scene_gt


def _json_bytes(info, tmp):
    _save_json(tmp, info)  # the writer gt_info uses: one image per line, the toolkit's layout
    with open(tmp, "rb") as f:
        return f.read()


def render_train(data_dir, dataset, radii, obj_ids=None, min_views=1000, mode="hinterstoisser", azimuth_range=(0.0, TWO_PI),
                 elev_range=(-0.25 * TWO_PI, 0.25 * TWO_PI), ssaa=4, shading="phong", ambient=0.5, models="models", out=None, host=False,
                 force=False, check=False, device="cuda"):
    """-> dict(out=folder, images={obj_id: number of images}, differences=[...] (with `check`: what differs from the files on disk))."""
    import tempfile

    base = osp.join(data_dir, dataset)
    out = osp.join(base, "train_render") if out is None else out
    models_dir = osp.join(base, models)
    cam = read_camera(osp.join(base, "camera.json"))
    W, H = cam["im_size"]
    if obj_ids is None:
        obj_ids = sorted(int(f[4:10]) for f in os.listdir(models_dir) if f.startswith("obj_") and f.endswith(".ply") and f[4:10].isdigit())
    obj_ids = [int(o) for o in obj_ids]
    if not obj_ids or not radii:
        raise ValueError("render_train: no object or no radius to render")
    folders = {o: osp.join(out, f"{o:06d}") for o in obj_ids}
    if not check:
        taken = [p for p in folders.values() if osp.exists(p) and (osp.isfile(p) or os.listdir(p))]
        if taken and not force:
            raise FileExistsError(f"render_train: {', '.join(taken)} exist(s); pass force=True (--force) to replace")
    if host:
        from .shade_host import NumpyDepthRenderer, NumpyShadedRenderer

        ren_rgb, ren_depth = NumpyShadedRenderer(W, H, ambient=ambient, shading=shading, ssaa=ssaa), NumpyDepthRenderer(W, H)
    else:
        from .bop_eval import _cuda_device
        from .render import HipDepthRenderer, HipShadedRenderer

        dev = _cuda_device(device)
        ren_rgb, ren_depth = HipShadedRenderer(W, H, device=dev, ambient=ambient, shading=shading, ssaa=ssaa), HipDepthRenderer(W, H, device=dev)
    for o in obj_ids:  # every model is read before anything is written or removed
        kw = load_model(models_dir, o)
        ren_rgb.add_object(o, **kw)
        ren_depth.add_object(o, kw["verts"], kw["faces"])
    Rs, ts, levels = object_views(radii, min_views, mode, azimuth_range, elev_range)
    if not len(Rs):
        raise ValueError("render_train: no view inside the azimuth and elevation ranges")
    images, differences = {}, []
    with tempfile.TemporaryDirectory() as scratch:
        for o in obj_ids:
            folder, seen = folders[o], set()
            if not check:
                if osp.isdir(folder):
                    shutil.rmtree(folder)
                elif osp.exists(folder):
                    os.remove(folder)
                for sub in ("rgb", "depth"):
                    os.makedirs(osp.join(folder, sub))
            for rel, content in object_files(o, Rs, ts, levels, cam, ren_rgb, ren_depth):
                if isinstance(content, dict):
                    content = _json_bytes(content, osp.join(scratch, "scene.json"))
                path = osp.join(folder, rel)
                seen.add(rel)
                if not check:
                    with open(path, "wb") as f:
                        f.write(content)
                elif not osp.isfile(path):
                    differences.append(f"{path}: missing")
                else:
                    with open(path, "rb") as f:
                        if f.read() != content:
                            differences.append(f"{path}: differs")
            if check:
                for sub in ("rgb", "depth"):
                    if osp.isdir(osp.join(folder, sub)):
                        differences += [f"{osp.join(folder, sub, n)}: not a file of this render" for n in sorted(os.listdir(osp.join(folder, sub)))
                                        if osp.join(sub, n) not in seen]
            images[o] = len(Rs)
    return dict(out=out, images=images, differences=differences)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m unopose_amd.render_train", description="Render every object model from a sphere of viewpoints and write the "
                                 "result as a BOP split (the toolkit's render_train_imgs.py) with the HIP rasterisers: Phong shading, textures, supersampling.")
    ap.add_argument("--data-dir", required=True, help="the folder that holds the dataset folder")
    ap.add_argument("--dataset", required=True)
    ap.add_argument("--obj-ids", type=int, nargs="*", default=None, help="default: every obj_XXXXXX.ply of the models folder")
    ap.add_argument("--radii", type=float, nargs="+", required=True, help="radii of the view spheres, in the models' units (mm)")
    ap.add_argument("--min-views", type=int, default=1000, help="points on the whole sphere at least; the sampler decides the number")
    ap.add_argument("--mode", choices=("hinterstoisser", "fibonacci"), default="hinterstoisser")
    ap.add_argument("--azimuth-range", type=float, nargs=2, default=(0.0, TWO_PI), metavar=("A0", "A1"), help="radians, both ends included")
    ap.add_argument("--elev-range", type=float, nargs=2, default=(-0.25 * TWO_PI, 0.25 * TWO_PI), metavar=("E0", "E1"), help="radians, both ends included")
    ap.add_argument("--ssaa", type=int, choices=(1, 2, 3, 4), default=4, help="supersampling factor of the colour render")
    ap.add_argument("--shading", choices=("phong", "flat"), default="phong")
    ap.add_argument("--ambient", type=float, default=0.5)
    ap.add_argument("--models", default="models", help="the models folder inside the dataset folder")
    ap.add_argument("--out", default=None, help="default: <data-dir>/<dataset>/train_render")
    ap.add_argument("--host", action="store_true", help="the numpy forms of the kernels, for comparison")
    ap.add_argument("--force", action="store_true", help="replace existing object folders")
    ap.add_argument("--check", action="store_true", help="compare with the files on disk, write nothing, exit 1 on a difference")
    a = ap.parse_args(argv)
    try:
        res = render_train(a.data_dir, a.dataset, a.radii, obj_ids=a.obj_ids or None, min_views=a.min_views, mode=a.mode, azimuth_range=tuple(a.azimuth_range),
                           elev_range=tuple(a.elev_range), ssaa=a.ssaa, shading=a.shading, ambient=a.ambient, models=a.models, out=a.out, host=a.host,
                           force=a.force, check=a.check)
    except FileExistsError as e:
        print(e, file=sys.stderr)
        return 2
    n = sum(res["images"].values())
    if a.check:
        for d in res["differences"]:
            print(d)
        print("%d images of %d objects compared with %s: %s" % (n, len(res["images"]), res["out"], "%d differences" % len(res["differences"]) if res["differences"] else "equal"))
        return 1 if res["differences"] else 0
    print("%d images of %d objects -> %s" % (n, len(res["images"]), res["out"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
