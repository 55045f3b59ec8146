"""Expected `scene_gt_coco.json` / `scene_gt_coco_modal.json` for the ground truths of tests/gt_info_case.py from the REFERENCE's vendored
bop_toolkit:
    python tests/golden/make_coco_gt_golden.py <reference checkout>   ->  tests/golden/coco_gt.json
* `bop_toolkit_lib.pycoco_utils` is imported with an empty stand-in registered for `skimage` / `skimage.measure` (only its polygon functions
  use them);
* per scene and bbox type the loop body of third_party/bop_toolkit/scripts/calc_gt_coco.py -- its own lines, read from the checkout and
  executed here, not restated (the script itself cannot run: it uses `np.bool` and hard-coded parameters) -- on the masks of
  tests/golden/gt_info_masks.npz and the fractions of tests/golden/gt_info.json;
* `pycoco_utils.rle_to_binary_mask` of every count list it wrote, for the decoder's tests.
The generator asserts that a skip before a kept annotation, an `ignore: true` and a leading-0 count list all occur, so the fixture cannot
quietly lose one.  The fixture holds data only."""
import json
import os
import sys
import textwrap
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True
if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "third_party", "bop_toolkit")):
    sys.exit(__doc__)
REFERENCE = sys.argv[1]
sys.path.insert(0, os.path.join(REFERENCE, "third_party", "bop_toolkit"))
for stub in ("skimage", "skimage.measure"):
    sys.modules.setdefault(stub, types.ModuleType(stub))
sys.modules["skimage"].measure = sys.modules["skimage.measure"]

from bop_toolkit_lib import pycoco_utils  # noqa: E402
from gt_info_case import LAYOUT  # noqa: E402

DATASET, SPLIT = "gtcase", "test"


def toolkit_scene(scene_id, scene_gt, scene_gt_info, masks, bbox_type, size, obj_ids):
    """coco_scene_output as scripts/calc_gt_coco.py fills it for one scene: the script's own statements from "Go through each view" to the
    write, run on these names."""
    lines = open(os.path.join(REFERENCE, "third_party", "bop_toolkit", "scripts", "calc_gt_coco.py")).read().splitlines()
    first = next(i for i, line in enumerate(lines) if "Go through each view in scene_gt" in line)
    last = next(i for i, line in enumerate(lines) if i > first and "with open(coco_gt_path" in line)
    root = os.path.join("/data", DATASET, SPLIT, "{scene_id:06d}")
    dp_split = dict(rgb_tpath=os.path.join(root, "rgb", "{im_id:06d}.png"), mask_tpath=os.path.join(root, "mask", "{im_id:06d}_{gt_id:06d}.png"),
                    mask_visib_tpath=os.path.join(root, "mask_visib", "{im_id:06d}_{gt_id:06d}.png"), im_size=tuple(size))
    head = next(i for i, line in enumerate(lines) if line.startswith("CATEGORIES = ["))
    tail = next(i for i, line in enumerate(lines) if i > head and line == "}")
    import datetime

    names = dict(dataset_name=DATASET, split=SPLIT, dp_model=dict(obj_ids=obj_ids), datetime=datetime)
    exec("\n".join(lines[head:tail + 1]), names)  # CATEGORIES and INFO, as the script forms them
    coco = {"info": names["INFO"], "licenses": [], "categories": names["CATEGORIES"], "images": [], "annotations": []}
    scope = dict(scene_gt=scene_gt, scene_gt_info=scene_gt_info, scene_id=scene_id, dp_split=dp_split, bbox_type=bbox_type, p=dict(bbox_type=bbox_type),
                 coco_gt_path=os.path.join(root.format(scene_id=scene_id), "scene_gt_coco.json"), coco_scene_output=coco, segmentation_id=1,
                 pycoco_utils=pycoco_utils, os=os, np=types.SimpleNamespace(bool=bool),
                 inout=types.SimpleNamespace(load_depth=lambda path: masks[path].astype(np.uint8) * 255))
    exec(textwrap.dedent("\n".join(lines[first:last])), scope)
    return coco


def main():
    gold = json.load(open(os.path.join(HERE, "gt_info.json")))
    z = np.load(os.path.join(HERE, "gt_info_masks.npz"))
    W, H = gold["size"]
    obj_ids = sorted({o for _, objects in LAYOUT.values() for o, *_ in objects})
    scene_gt, scene_gt_info, masks = {}, {}, {}
    for (sid, iid), (_, objects) in LAYOUT.items():
        scene_gt.setdefault(sid, {})[iid] = [dict(obj_id=o) for o, *_ in objects]
        scene_gt_info.setdefault(sid, {})[iid] = gold["gt_info"][f"{sid}/{iid}"]
        for gid in range(len(objects)):
            base = os.path.join("/data", DATASET, SPLIT, f"{sid:06d}")
            masks[os.path.join(base, "mask", f"{iid:06d}_{gid:06d}.png")] = z[f"mask_{sid}_{iid}_{gid}"]
            masks[os.path.join(base, "mask_visib", f"{iid:06d}_{gid:06d}.png")] = z[f"visib_{sid}_{iid}_{gid}"]
    assert sum(len(g) for ims in scene_gt.values() for g in ims.values()) == 10
    out = dict(dataset=DATASET, split=SPLIT, size=[W, H], obj_ids=obj_ids, coco={}, decoded=[],
               scene_gt={str(sid): {str(iid): [g["obj_id"] for g in gts] for iid, gts in ims.items()} for sid, ims in scene_gt.items()})
    for bbox_type in ("amodal", "modal"):
        out["coco"][bbox_type] = {str(sid): toolkit_scene(sid, scene_gt[sid], scene_gt_info[sid], masks, bbox_type, (W, H), obj_ids) for sid in scene_gt}
    out = json.loads(json.dumps(out, default=lambda v: v.item()))  # numpy scalars -> the values json.dump writes

    anns = [a for sid in out["coco"]["amodal"] for a in out["coco"]["amodal"][sid]["annotations"]]
    n_gt = {sid: sum(len(g) for g in ims.values()) for sid, ims in scene_gt.items()}
    assert any(len(out["coco"]["amodal"][str(sid)]["annotations"]) < n for sid, n in n_gt.items()), "a ground truth is skipped"
    kept = [(a["image_id"], a["id"]) for a in out["coco"]["amodal"]["1"]["annotations"]]
    assert [i for _, i in kept] == list(range(1, len(kept) + 1)) and len(kept) < n_gt[1], "ids do not advance on a skip"
    skipped_first = [gid for gid in range(len(scene_gt[1][0])) if not z[f"visib_1_0_{gid}"].any()]
    assert skipped_first and any(im == 1 for im, _ in kept), "a skip (image 0) before a kept annotation (image 1)"
    assert any(a["ignore"] is True for a in anns) and any(a["ignore"] is False for a in anns), "ignore: true and false"
    assert any(a["segmentation"]["counts"][0] == 0 for a in anns), "a leading-0 count list"
    assert any(a["bbox"] != m["bbox"] for a, m in zip(anns, (x for sid in out["coco"]["modal"] for x in out["coco"]["modal"][sid]["annotations"]))), \
        "amodal and modal boxes differ somewhere"
    for a in anns:
        mask = pycoco_utils.rle_to_binary_mask(a["segmentation"])
        out["decoded"].append(dict(size=a["segmentation"]["size"], counts=a["segmentation"]["counts"],
                                   rows=["".join("1" if v else "0" for v in row) for row in mask]))
    json.dump(out, open(os.path.join(HERE, "coco_gt.json"), "w"), indent=0)
    for bbox_type, scenes in out["coco"].items():
        for sid, coco in scenes.items():
            print(bbox_type, sid, [(a["id"], a["image_id"], a["category_id"], a["area"], a["bbox"], a["ignore"], len(a["segmentation"]["counts"]))
                                   for a in coco["annotations"]])


if __name__ == "__main__":
    main()
