"""Expected ground-truth info, masks and recalls for tests/gt_info_case.py from the REFERENCE's vendored bop_toolkit_lib and scripts:
    python tests/golden/make_gt_info_golden.py <reference checkout>   ->  tests/golden/gt_info.json, tests/golden/gt_info_masks.npz
* per ground truth the loop body of lib/pysixd/scripts/calc_gt_info.py:110-171 with the toolkit's `misc.depth_im_to_dist_im_fast`,
  `visibility.estimate_visib_mask_gt` and `misc.calc_2d_bbox`, on canvas maps rendered by tests/raster_np.py (the toolkit's OpenGL renderers
  are not needed: both sides see the same depth), and the two masks as calc_gt_masks.py:92-108 forms them;
* per scoring case of `gt_info_case.recall_cases` the recall at every MSSD threshold: `pose_error.mssd`, the validity rule of
  scripts/eval_calc_scores.py -- its own lines, read from the checkout and executed here, not restated --, `pose_matching.match_poses_scene`
  and `score.calc_localization_scores`.
The generator asserts that the scenes contain every situation the tests rely on, so the fixture cannot quietly lose one."""
import json
import os
import sys
import textwrap

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True
if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "third_party", "bop_toolkit")):
    sys.exit(__doc__)
REFERENCE = sys.argv[1]
sys.path.insert(0, os.path.join(REFERENCE, "third_party", "bop_toolkit"))

from bop_toolkit_lib import misc, pose_error, pose_matching, score, visibility  # noqa: E402
from gt_info_case import DELTA, make_models, make_scenes, recall_cases  # noqa: E402
from raster_np import NumpyRenderer  # noqa: E402

W, H = 36, 24


def toolkit_gt_info(depth, canvas, K):
    """calc_gt_info.py's arithmetic for one ground truth, with the toolkit's functions."""
    depth_gt = canvas[H:2 * H, W:2 * W]
    dist_gt, dist_im = misc.depth_im_to_dist_im_fast(depth_gt, K), misc.depth_im_to_dist_im_fast(depth, K)
    visib_gt = visibility.estimate_visib_mask_gt(dist_im, dist_gt, DELTA, visib_mode="bop19")
    large, mask = canvas > 0, dist_gt > 0
    n_all, n_valid, n_visib = int(np.sum(large)), int(np.sum(dist_im[mask] > 0)), int(visib_gt.sum())
    bbox, bbox_visib = [-1, -1, -1, -1], [-1, -1, -1, -1]
    if n_visib > 0:
        ys, xs = large.nonzero()
        bbox = [int(e) for e in misc.calc_2d_bbox(xs - W, ys - H, (W, H))]
        ys, xs = visib_gt.nonzero()
        bbox_visib = [int(e) for e in misc.calc_2d_bbox(xs, ys, (W, H))]
    info = dict(px_count_all=n_all, px_count_valid=n_valid, px_count_visib=n_visib, visib_fract=float(n_visib / float(n_all)) if n_all > 0 else 0.0,
                bbox_obj=bbox, bbox_visib=bbox_visib)
    return info, mask, visib_gt


def toolkit_validity(scene_gt, scene_gt_info, scene_targets, visib_gt_min):
    """scene_gt_valid as scripts/eval_calc_scores.py fills it: the script's own statements between its two comments, run on these names."""
    lines = open(os.path.join(REFERENCE, "third_party", "bop_toolkit", "scripts", "eval_calc_scores.py")).read().splitlines()
    first = next(i for i, line in enumerate(lines) if "Keep GT poses only for the selected targets" in line)
    last = next(i for i, line in enumerate(lines) if i > first and "Load pre-calculated errors" in line)
    scope = dict(scene_gt=scene_gt, scene_gt_info=scene_gt_info, scene_targets=scene_targets, p=dict(visib_gt_min=visib_gt_min))
    exec(textwrap.dedent("\n".join(lines[first:last])), scope)
    return scope["scene_gt_valid"]


def toolkit_recalls(case, models):
    """Recall at every MSSD threshold, and which ground truths were valid."""
    scene_errs, est_id = {}, 0
    for (sid, iid), objs in case["targets"].items():
        for obj_id, inst_count in objs.items():  # eval_calc_errors.py with n_top = -1: the inst_count best-scored estimates
            rows = sorted((r for r in case["results"] if (r["scene_id"], r["im_id"], r["obj_id"]) == (sid, iid, obj_id)), key=lambda r: -r["score"])
            for r in rows[:inst_count]:
                m = models[obj_id]
                syms = [dict(R=s["R"], t=s["t"].reshape(3, 1)) for s in m["symmetries"]]
                errs = {gid: [float(pose_error.mssd(r["R"], r["t"].reshape(3, 1), g["R"], g["t"].reshape(3, 1), m["pts"], syms) / m["diameter"])]
                        for gid, g in enumerate(case["scene_gt"][sid][iid]) if g["obj_id"] == obj_id}
                scene_errs.setdefault(sid, []).append(dict(im_id=iid, obj_id=obj_id, est_id=est_id, score=r["score"], errors=errs))
                est_id += 1
    valid = {}
    for sid in case["scene_gt"]:
        scene_targets = {iid: {o: dict(inst_count=c) for o, c in objs.items()} for (s, iid), objs in case["targets"].items() if s == sid}
        valid[sid] = toolkit_validity(case["scene_gt"][sid], case["gt_info"][sid], scene_targets, case["visib_gt_min"])
    recalls = []
    for th in np.arange(0.05, 0.51, 0.05):
        matches = []
        for sid in case["scene_gt"]:
            matches += pose_matching.match_poses_scene(sid, case["scene_gt"][sid], valid[sid], scene_errs.get(sid, []), [th], -1)
        recalls.append(float(score.calc_localization_scores(list(case["scene_gt"]), list(models), matches, -1, do_print=False)["recall"]))
    return recalls, {f"{sid}/{iid}": [bool(v) for v in flags] for sid, ims in valid.items() for iid, flags in ims.items()}


def main():
    models = make_models()
    ren = NumpyRenderer(3 * W, 3 * H)
    for obj_id, m in models.items():
        ren.add_object(obj_id, m["verts"], m["faces"])
    scene_gt, cameras, depth_images, canvases = make_scenes(lambda *a: ren.render_object(*a)["depth"], W, H)
    gt_info, masks = {}, {}
    for (sid, iid, gid), canvas in canvases.items():
        info, mask, visib = toolkit_gt_info(depth_images[sid][iid], canvas, cameras[sid][iid])
        gt_info.setdefault(sid, {}).setdefault(iid, []).append(info)
        masks[f"mask_{sid}_{iid}_{gid}"], masks[f"visib_{sid}_{iid}_{gid}"] = mask, visib

    # every situation the tests rely on is there
    e = {k: gt_info[k[0]][k[1]][k[2]] for k in canvases}
    in_image = lambda k: int((canvases[k][H:2 * H, W:2 * W] > 0).sum())  # noqa: E731
    assert e[(1, 0, 1)]["px_count_all"] > in_image((1, 0, 1)) > 0 and max(e[(1, 0, 1)]["bbox_obj"][:2]) < 0, "truncated at the left and the upper border"
    assert in_image((1, 0, 2)) == 0 and e[(1, 0, 2)]["px_count_all"] > 0 and e[(1, 0, 2)]["px_count_visib"] == 0, "outside the image, on the canvas"
    assert e[(1, 0, 2)]["bbox_obj"] == [-1, -1, -1, -1]
    assert e[(1, 0, 3)]["px_count_all"] == 0 and e[(1, 0, 3)]["visib_fract"] == 0.0, "off the canvas"
    assert e[(1, 0, 0)]["px_count_valid"] < e[(1, 0, 0)]["px_count_visib"] == e[(1, 0, 0)]["px_count_all"], "holes: visible, not valid"
    assert 0.1 < e[(1, 1, 0)]["visib_fract"] < 1 and 0.1 < e[(2, 0, 1)]["visib_fract"] < 1, "partly occluded"
    assert 0 < e[(1, 1, 1)]["visib_fract"] < 0.1, "visible to less than a tenth"
    assert e[(1, 1, 2)]["px_count_visib"] == 0 and e[(1, 1, 2)]["px_count_all"] > 0 and e[(1, 1, 2)]["bbox_visib"] == [-1, -1, -1, -1], "fully occluded"
    assert e[(2, 0, 0)]["visib_fract"] == e[(2, 0, 2)]["visib_fract"] > e[(2, 0, 1)]["visib_fract"], "two equally visible instances"
    assert not np.array_equal(cameras[1][0], cameras[1][1]), "two intrinsics"

    out = dict(size=[W, H], delta=DELTA, gt_info={f"{sid}/{iid}": v for sid, ims in gt_info.items() for iid, v in ims.items()}, recalls={}, valid={})
    for name, case in recall_cases(scene_gt, cameras, gt_info).items():
        out["recalls"][name], out["valid"][name] = toolkit_recalls(case, models)
    assert out["recalls"]["issue"] == [0.0] * 10
    assert out["valid"]["scenes_k1"]["2/0"] == [True, False, False], "the tie keeps ground-truth order"
    json.dump(out, open(os.path.join(HERE, "gt_info.json"), "w"), indent=0)
    np.savez_compressed(os.path.join(HERE, "gt_info_masks.npz"), **masks)
    for k, v in out["gt_info"].items():
        print(k, [(i["px_count_all"], i["px_count_valid"], i["px_count_visib"], round(i["visib_fract"], 3), i["bbox_obj"], i["bbox_visib"]) for i in v])
    print(out["recalls"])
    print(out["valid"])


if __name__ == "__main__":
    main()
