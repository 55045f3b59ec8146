"""The dataset folder behind tests/golden/coco_gt.json (made by tests/golden/make_coco_gt_golden.py with the toolkit's functions): the
ten ground truths of tests/gt_info_case.py as files -- scene_gt.json (object ids), scene_gt_info.json, mask/, mask_visib/ -- so that
`unopose_amd.coco_gt` runs on what the toolkit's script ran on."""
import json
import os
import os.path as osp

import numpy as np

GOLD = osp.join(osp.dirname(osp.abspath(__file__)), "golden")


def fixture():
    with open(osp.join(GOLD, "coco_gt.json")) as f:
        return json.load(f)


def build(root):
    """-> (fixture, dataset name, split); the folder is <root>/<name>/<split>/<scene:06d>/."""
    from PIL import Image

    fx = fixture()
    with open(osp.join(GOLD, "gt_info.json")) as f:
        info = json.load(f)["gt_info"]
    z = np.load(osp.join(GOLD, "gt_info_masks.npz"))
    for sid, ims in fx["scene_gt"].items():
        folder = osp.join(root, fx["dataset"], fx["split"], f"{int(sid):06d}")
        for sub in ("mask", "mask_visib"):
            os.makedirs(osp.join(folder, sub))
        with open(osp.join(folder, "scene_gt.json"), "w") as f:
            json.dump({iid: [dict(obj_id=o) for o in objs] for iid, objs in ims.items()}, f)
        with open(osp.join(folder, "scene_gt_info.json"), "w") as f:
            json.dump({iid: info[f"{sid}/{iid}"] for iid in ims}, f)
        for iid, objs in ims.items():
            for gid in range(len(objs)):
                for sub, key in (("mask", "mask"), ("mask_visib", "visib")):
                    Image.fromarray(z[f"{key}_{sid}_{iid}_{gid}"].astype(np.uint8) * 255).save(osp.join(folder, sub, f"{int(iid):06d}_{gid:06d}.png"))
    return fx, fx["dataset"], fx["split"]
