"""Seeded BOP-layout folders at a realistic size (480 x 640, "lm" layout) for the provider's device path: the input of
tests/test_device_prep_gpu.py and of scripts/provider_rate.py.  Unlike tests/bop_synth.py's tiny scenes these make the provider's
1.2-radius filter act.  Per detection: an elliptical object (radii 30-150 px) at 0.8 m with a depth slope, in front of a background
at 1.4 m; the detector's mask is 6 px larger than the object, so a ring of background leaks into it; 3 % of the depth pixels are
holes.  Every object id has one reference view (its own ellipse, radii 30-150 px, at 0.8 m).  The reference's size is independent of
the detection's, so the filter's threshold ranges from "removes the background ring" (thousands of points) to "nothing survives"
(a small reference for a large detection: the detection is dropped after its reference draw was made)."""
import json
import os
import os.path as osp

import numpy as np

from unopose_amd.provider import rle_counts_to_string, rle_encode

H, W = 480, 640
K = [572.4, 0.0, 325.3, 0.0, 573.6, 242.0, 0.0, 0.0, 1.0]
N_OBJ = 15  # "lm": object ids 1..15
REF_SCENE, QUERY_SCENE = 1, 2
CFG = dict(ref_targets_name="test_ref_targets.json", rgb_mask_flag=True, img_size=224, n_sample_observed_point=2048,
           n_sample_template_point=5000, minimum_n_point=8, seg_filter_score=0.25, obj_idxs=None)


def _write_png(path, arr):
    from PIL import Image

    os.makedirs(osp.dirname(path), exist_ok=True)
    Image.fromarray(arr).save(path, compress_level=1)


def _ellipse(cy, cx, ry, rx):
    yy, xx = np.mgrid[0:H, 0:W]
    return ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0


def _surface(rs, cy, cx):
    """object depth in mm: 0.8 m at the centre, a slope of up to 0.4 mm per pixel, 1 mm of noise"""
    yy, xx = np.mgrid[0:H, 0:W]
    sx, sy = rs.uniform(-0.4, 0.4, size=2)
    return 800.0 + sx * (xx - cx) + sy * (yy - cy) + rs.randint(-1, 2, size=(H, W))


def _image(rs, objects):
    """objects: [(cy, cx, ry, rx)] painted in order -> colour, depth (uint16 mm), object masks"""
    rgb = rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    depth = (1400.0 + rs.randint(-2, 3, size=(H, W))).astype(np.uint16)
    masks = []
    for cy, cx, ry, rx in objects:
        m = _ellipse(cy, cx, ry, rx)
        depth[m] = _surface(rs, cy, cx)[m].astype(np.uint16)
        masks.append(m)
    depth[rs.rand(H, W) < 0.03] = 0
    return rgb, depth, masks


def _placement(rs):
    ry, rx = rs.uniform(30, 150, size=2)
    return rs.uniform(ry, H - ry), rs.uniform(rx, W - rx), ry, rx


def build(root, n_images=16, dets_per_image=(5, 15), seed=0):
    """Writes the dataset under `root` and returns (provider cfg dict, detections path)."""
    rs = np.random.RandomState(seed)
    test = osp.join(root, "lm", "test")
    cam, gt = {}, {}
    folder = osp.join(test, f"{REF_SCENE:06d}")
    for obj_id in range(1, N_OBJ + 1):  # reference view of object i: image i of the reference scene
        rgb, depth, masks = _image(rs, [_placement(rs)])
        _write_png(osp.join(folder, "rgb", f"{obj_id:06d}.png"), rgb)
        _write_png(osp.join(folder, "depth", f"{obj_id:06d}.png"), depth)
        # visible = measured: a hole inside the reference's mask would enter its cloud as a point at the camera centre
        _write_png(osp.join(folder, "mask_visib", f"{obj_id:06d}_{0:06d}.png"), ((masks[0] & (depth > 0)) * 255).astype(np.uint8))
        ang = 0.2 * obj_id
        cam[str(obj_id)] = {"cam_K": K, "depth_scale": 1.0}
        gt[str(obj_id)] = [{"cam_R_m2c": [float(np.cos(ang)), float(-np.sin(ang)), 0.0, float(np.sin(ang)), float(np.cos(ang)), 0.0, 0.0, 0.0, 1.0],
                            "cam_t_m2c": [5.0 * obj_id, -3.0, 800.0], "obj_id": obj_id}]
    json.dump(cam, open(osp.join(folder, "scene_camera.json"), "w"))
    json.dump(gt, open(osp.join(folder, "scene_gt.json"), "w"))

    cam, dets, targets = {}, [], []
    folder = osp.join(test, f"{QUERY_SCENE:06d}")
    for im_id in range(n_images):
        n = int(rs.randint(dets_per_image[0], dets_per_image[1] + 1))
        objects = [_placement(rs) for _ in range(n)]
        rgb, depth, _ = _image(rs, objects)
        _write_png(osp.join(folder, "rgb", f"{im_id:06d}.png"), rgb)
        _write_png(osp.join(folder, "depth", f"{im_id:06d}.png"), depth)
        cam[str(im_id)] = {"cam_K": K, "depth_scale": 1.0}
        for j, (cy, cx, ry, rx) in enumerate(objects):
            obj_id = int(rs.randint(1, N_OBJ + 1))
            seg = rle_encode(_ellipse(cy, cx, ry + 6, rx + 6))  # the detector's mask: 6 px larger than the object
            if j % 2:
                seg = {"size": seg["size"], "counts": rle_counts_to_string(seg["counts"])}
            dets.append(dict(scene_id=QUERY_SCENE, image_id=im_id, category_id=obj_id, score=float(rs.uniform(0.3, 0.95)), time=0.1,
                             bbox=[int(cx - rx), int(cy - ry), int(2 * rx), int(2 * ry)], segmentation=seg))
            if not any(t["im_id"] == im_id and t["obj_id"] == obj_id for t in targets):
                targets.append(dict(scene_id=QUERY_SCENE, im_id=im_id, obj_id=obj_id, ref_scene_id=REF_SCENE, ref_im_id=obj_id))
    json.dump(cam, open(osp.join(folder, "scene_camera.json"), "w"))
    json.dump(targets, open(osp.join(root, "lm", CFG["ref_targets_name"]), "w"))
    det_path = osp.join(root, "detections.json")
    json.dump(dets, open(det_path, "w"))
    return dict(CFG, data_dir=root), det_path
