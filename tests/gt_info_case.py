"""Scenes for the ground-truth visibility (unopose_amd/gt_info.py, csrc/gtinfo.hip), shared by tests/golden/make_gt_info_golden.py (the
toolkit's functions on them) and the tests.  Every situation `calc_gt_info.py` distinguishes is in them: an object truncated by the image
border, one partly occluded, one visible to less than a tenth, one fully occluded, one outside the image but on the 3x canvas, one off
the canvas, holes in the test depth over an object, two instances with exactly equal visibility, two images with different intrinsics.
Geometry is given in pixels of a W x H image, so the same scenes exist at every size; the test depth is put together from the crops of
the canvas renders, so any renderer of the canvas (tests/raster_np.py, the HIP rasteriser) serves."""
import numpy as np

from bop_eval_case import icosphere

DELTA = 15.0
BACKGROUND = 1400.0


def make_models():
    sv, sf = icosphere()
    models = {}
    for obj_id, axes in ((1, (100.0, 90.0, 80.0)), (2, (75.0, 105.0, 85.0))):
        verts = sv * np.asarray(axes)
        d = np.linalg.norm(verts[:, None] - verts[None], axis=2).max()
        models[obj_id] = dict(pts=verts, verts=verts, faces=sf, diameter=float(d), symmetries=[dict(R=np.eye(3), t=np.zeros(3))])
    return models


def cameras_for(W, H):
    """Two intrinsics for a W x H image: an object 100 mm across its half axis at 800 mm is about W / 7 pixels in radius."""
    f = 40.0 * W / 36.0
    K1 = np.array([[f, 0, (W - 1) / 2.0 - 0.3], [0, f * 1.02, (H - 1) / 2.0 + 0.2], [0, 0, 1.0]])
    K2 = np.array([[f * 1.07, 0, (W - 1) / 2.0 + 1.3], [0, f * 0.95, (H - 1) / 2.0 - 0.8], [0, 0, 1.0]])
    return K1, K2


# image -> (which camera, [(obj_id, u / W, v / H, z, what the test depth does to it)])
#   "seen": in the test depth as rendered; "holes": in it, the upper half of its silhouette without a measurement; ("behind", c): in it, but
#   an occluder 250 mm nearer than its centre covers its silhouette from the column c of its bounding box on (0 = all of it, 1 = all but its first
#   column, 0.5 = its right half); "absent": not in the test depth (outside the image anyway)
LAYOUT = {
    (1, 0): (0, [(1, 0.62, 0.50, 800.0, "holes"), (2, 0.03, 0.12, 820.0, "seen"), (1, -0.50, 0.50, 800.0, "absent"), (2, -3.0, 0.5, 800.0, "absent")]),
    (1, 1): (1, [(1, 0.25, 0.50, 800.0, ("behind", 0.5)), (1, 0.62, 0.50, 800.0, ("behind", 1)), (2, 0.86, 0.50, 900.0, ("behind", 0))]),
    (2, 0): (0, [(1, 0.21, 0.50, 800.0, "seen"), (1, 0.50, 0.50, 800.0, ("behind", 0.5)), (1, 0.79, 0.50, 800.0, "seen")]),
}


def make_scenes(render, W=36, H=24, seed=3, images=None):
    """render(obj_id, R, t, fx, fy, cx, cy) -> the (3H, 3W) canvas depth (the principal point already moved by the caller: cx + W, cy + H).
    -> scene_gt, cameras, depth_images, canvases {(scene_id, im_id, gt_id): canvas depth}.  `images`: only these (scene_id, im_id)."""
    rs = np.random.RandomState(seed)
    Ks = cameras_for(W, H)
    scene_gt, cameras, depth_images, canvases = {}, {}, {}, {}
    for (sid, iid), (cam, objects) in LAYOUT.items():
        if images is not None and (sid, iid) not in images:
            continue
        K = Ks[cam]
        gts, z, slabs = [], np.full((H, W), np.inf), []
        for gid, (obj_id, u, v, dist, how) in enumerate(objects):
            ang = 0.4 * gid + 0.3 * iid
            R = np.array([[np.cos(ang), -np.sin(ang), 0.0], [np.sin(ang), np.cos(ang), 0.0], [0.0, 0.0, 1.0]])
            t = np.array([(u * W - K[0, 2]) / K[0, 0] * dist, (v * H - K[1, 2]) / K[1, 1] * dist, dist])
            gts.append(dict(obj_id=obj_id, R=R, t=t))
            canvas = np.asarray(render(obj_id, R, t, K[0, 0], K[1, 1], K[0, 2] + W, K[1, 2] + H), np.float32)
            assert canvas.shape == (3 * H, 3 * W)
            canvases[(sid, iid, gid)] = canvas
            d = canvas[H:2 * H, W:2 * W].astype(np.float64)
            if how == "absent" or not (d > 0).any():
                continue
            z = np.where((d > 0) & (d < z), d, z)
            ys, xs = (d > 0).nonzero()
            if how == "holes":
                slabs.append(((d > 0) & (np.arange(H)[:, None] < (ys.min() + ys.max() + 1) // 2), 0.0))
            elif how != "seen":
                first = xs.min() + (1 if how[1] == 1 else int(round(how[1] * (xs.max() - xs.min() + 1))))
                slabs.append(((d > 0) & (np.arange(W)[None, :] >= first), dist - 250.0))
        z = np.where(np.isinf(z), BACKGROUND, z)
        z = z + np.round(rs.randn(H, W))  # 1 mm of noise, far below the visibility tolerance
        for where, value in slabs:
            z[where] = value
        scene_gt.setdefault(sid, {})[iid] = gts
        cameras.setdefault(sid, {})[iid] = K
        depth_images.setdefault(sid, {})[iid] = z.astype(np.float32)
    return scene_gt, cameras, depth_images, canvases


def pose_results(scene_gt, spoil=()):
    """One estimate per ground truth, at its pose, scores falling with the ground-truth index; the (scene_id, im_id, gt_id) in `spoil` are
    moved by half a metre."""
    out = []
    for sid, ims in scene_gt.items():
        for iid, gts in ims.items():
            for gid, g in enumerate(gts):
                t = g["t"] + (np.array([500.0, 0.0, 0.0]) if (sid, iid, gid) in spoil else 0.0)
                out.append(dict(scene_id=sid, im_id=iid, obj_id=g["obj_id"], score=0.9 - 0.1 * gid, R=g["R"], t=t, time=0.1))
    return out


def recall_cases(scene_gt, cameras, gt_info):
    """The scoring cases whose toolkit recalls the fixture records: name -> dict(scene_gt, cameras, results, targets, gt_info, visib_gt_min).
    "issue": one image, two ground truths of object 1, inst_count 1, the estimate equals the LESS visible one -- the toolkit scores 0,
    counting every ground truth scores 0.5.  The others run on the fixture's scenes with the computed `gt_info`."""
    K = cameras_for(36, 24)[0]
    two = {7: {0: [dict(obj_id=1, R=np.eye(3), t=np.array([0.0, 0.0, 800.0])), dict(obj_id=1, R=np.eye(3), t=np.array([200.0, 0.0, 800.0]))]}}
    hand = {7: {0: [dict(visib_fract=0.05), dict(visib_fract=0.9)]}}
    one = [dict(scene_id=7, im_id=0, obj_id=1, score=0.5, R=np.eye(3), t=np.array([0.0, 0.0, 800.0]), time=0.1)]
    count = lambda n: {(sid, iid): {o: n for o in {g["obj_id"] for g in gts}} for sid, ims in scene_gt.items() for iid, gts in ims.items()}  # noqa: E731
    spoil = [(1, 1, 0), (2, 0, 2)]
    return {
        "issue": dict(scene_gt=two, cameras={7: {0: K}}, results=one, targets={(7, 0): {1: 1}}, gt_info=hand, visib_gt_min=-1),
        "issue_min": dict(scene_gt=two, cameras={7: {0: K}}, results=one, targets={(7, 0): {1: 1}}, gt_info=hand, visib_gt_min=0.1),
        "scenes_k1": dict(scene_gt=scene_gt, cameras=cameras, results=pose_results(scene_gt, spoil), targets=count(1), gt_info=gt_info, visib_gt_min=-1),
        "scenes_k2": dict(scene_gt=scene_gt, cameras=cameras, results=pose_results(scene_gt, spoil), targets=count(2), gt_info=gt_info, visib_gt_min=-1),
        "scenes_min": dict(scene_gt=scene_gt, cameras=cameras, results=pose_results(scene_gt, spoil), targets=count(3), gt_info=gt_info, visib_gt_min=0.1),
    }


def extend_bop_scenes(root, name="lm"):
    """What a `bop_scenes.build` folder lacks for `gt_info.write_gt_info` and `bop_eval.score_csv` on its reference scene: models_eval/ (an
    ellipsoid per object id), a second instance of the object, 70 or 210 mm farther and to the side, in every odd image of the scene's scene_gt.json, a targets file over
    the scene with inst_count 1 (so the visibility rule has something to decide) and a result file with one estimate per ground truth.
    -> (csv path, scene id)."""
    import json
    import os
    import os.path as osp

    import bop_scenes
    from bop_score_case import write_ply

    sv, sf = icosphere()
    base, info = osp.join(root, name), {}
    for obj_id in range(1, bop_scenes.N_OBJ + 1):
        verts = sv * np.array([40.0 + 3 * obj_id, 70.0 - 2 * obj_id, 50.0 + obj_id])
        write_ply(osp.join(base, "models_eval", f"obj_{obj_id:06d}.ply"), verts, sf)
        info[str(obj_id)] = dict(diameter=float(np.linalg.norm(verts[:, None] - verts[None], axis=2).max()))
    json.dump(info, open(osp.join(base, "models_eval", "models_info.json"), "w"))
    sid = bop_scenes.REF_SCENE
    gt_path = osp.join(base, "test", f"{sid:06d}", "scene_gt.json")
    gt = json.load(open(gt_path))
    for iid, gts in gt.items():
        if int(iid) % 2:
            t = gts[0]["cam_t_m2c"]
            gts.append(dict(gts[0], cam_t_m2c=[t[0] + 30.0 * int(iid), t[1] + 40.0, t[2] + 70.0 * (int(iid) % 4)]))
    json.dump(gt, open(gt_path, "w"))
    json.dump([dict(scene_id=sid, im_id=int(iid), obj_id=gts[0]["obj_id"], inst_count=1) for iid, gts in gt.items()],
              open(osp.join(base, "test_targets_bop19.json"), "w"))
    csv = osp.join(root, "out", "results.csv")
    os.makedirs(osp.dirname(csv), exist_ok=True)
    with open(csv, "w") as f:
        f.write("scene_id,im_id,obj_id,score,R,t,time\n")
        for iid, gts in gt.items():
            for gid, g in enumerate(gts):  # the farther instance is found better than the nearer one
                t = np.asarray(g["cam_t_m2c"]) + (np.array([8.0, 0.0, 0.0]) if gid == 0 else 0.0)
                f.write(",".join((str(sid), iid, str(g["obj_id"]), repr(0.5 + 0.2 * gid), " ".join(repr(float(v)) for v in g["cam_R_m2c"]),
                                  " ".join(repr(float(v)) for v in t), "0.1")) + "\n")
    return csv, sid
