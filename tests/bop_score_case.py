"""The large synthetic scoring problem of the device scorer's tests (tests/test_bop_score_gpu.py, tests/test_bop_score_cpu.py,
scripts/bop_score_rate.py) and a writer that lays such a problem out as a BOP dataset folder.

`make_large_case()`: 480 x 640 images, 3 scenes x 10 images with two different K; three objects -- 1 without symmetry, 2 with a
two-fold symmetry, 3 with a five-fold axis that does NOT pass through the model origin, i.e. four discrete symmetries with non-zero
translations beside the identity; image (7, 2) holds two instances of object 1 (n_top = 2 and the greedy matching matter); one
estimate lies behind the camera (empty render); one ground truth and its estimate lie wholly outside the image (n_union = 0, VSD
error 1.0); the test depth is the z-buffer of the ground truths over an empty or planar background, with an occluder slab, 1 mm
noise and dropped (0) pixels, as `bop_eval_case.make_vsd_case` builds it.  More than 200 (estimate, ground truth) pairs when every
estimate is scored (n_top = -1 without targets).  `large_case_facts` is the host-route check that the problem is graded."""
import json
import os
import os.path as osp

import numpy as np

from bop_eval_case import icosphere, rot

W, H = 640, 480
K_A = np.array([[572.4, 0, 325.3], [0, 573.6, 242.0], [0, 0, 1.0]])
K_B = np.array([[1066.8, 0, 312.9], [0, 1067.5, 241.3], [0, 0, 1.0]])
SYM3_AXIS_POINT = np.array([12.0, -7.0, 4.0])  # a point of object 3's symmetry axis: off the origin, so its symmetries translate
TWO_INSTANCES = (7, 2)                          # (scene, image) with two instances of object 1
BEHIND = (7, 0, 2)                              # (scene, image, object) whose first estimate lies behind the camera
OUTSIDE = (8, 3, 1)                             # (scene, image, object) whose ground truth and estimate lie outside the image
ITODD_DELTA_PAIR = 6                            # index of the pair scored with vsd_delta = 5 in the counts test


def _models():
    sv, sf = icosphere()
    models = {}
    v = sv * np.array([40.0, 55.0, 70.0])
    v = v + 0.15 * np.array([40.0, 55.0, 70.0]) * np.sin(3.0 * sv[:, [1, 2, 0]])
    models[1] = dict(verts=v, syms=[dict(R=np.eye(3), t=np.zeros(3))])
    models[2] = dict(verts=sv * np.array([65.0, 65.0, 32.0]), syms=[dict(R=np.eye(3), t=np.zeros(3)), dict(R=rot([0, 0, 1], np.pi), t=np.zeros(3))])
    # object 3: the icosphere keeps the icosahedron's five-fold axis through vertex 0; stretching along that axis and a pear-shaped bulge
    # (a function of the height along it) keep the five-fold rotations and nothing else; the axis passes through SYM3_AXIS_POINT
    d = sv[0] / np.linalg.norm(sv[0])
    h = sv @ d
    v = 45.0 * (sv - np.outer(h, d)) * (1.0 + 0.25 * h)[:, None] + 75.0 * np.outer(h, d) + SYM3_AXIS_POINT
    syms = [dict(R=np.eye(3), t=np.zeros(3))]
    for k in range(1, 5):
        R = rot(d, 2.0 * np.pi * k / 5.0)
        syms.append(dict(R=R, t=SYM3_AXIS_POINT - R @ SYM3_AXIS_POINT))
    models[3] = dict(verts=v, syms=syms)
    out = {}
    for obj_id, m in models.items():
        diam = np.linalg.norm(m["verts"][:, None] - m["verts"][None], axis=2).max()
        out[obj_id] = dict(pts=m["verts"], verts=m["verts"], faces=sf, diameter=float(diam), symmetries=m["syms"])
    return out


def make_large_case(seed=23, images_per_scene=10, extra_estimates=0):
    """-> models, scene_gt, cameras, results, im_width, depth_images, (W, H).  `extra_estimates`: that many more low-scored estimates
    per ground truth (the timing script's larger variant); the tests use 0."""
    from raster_np import render_depth

    rs = np.random.RandomState(seed)
    models = _models()
    scene_gt, cameras, depth_images, results = {}, {}, {}, []
    for sid in (6, 7, 8):
        scene_gt[sid], cameras[sid], depth_images[sid] = {}, {}, {}
        K = K_B if sid == 8 else K_A
        spread = 0.45 if sid == 8 else 1.0  # the longer lens sees a narrower field
        for iid in range(images_per_scene):
            cameras[sid][iid] = K
            objs = [1, 2, 3] + ([1] if (sid, iid) == TWO_INSTANCES or rs.rand() < 0.35 else [])
            gts, z = [], np.full((H, W), np.inf)
            for k, obj_id in enumerate(objs):
                R = rot(rs.randn(3), rs.rand() * 3)
                t = np.array([((k - 1.5) * 150.0 + rs.uniform(-25, 25)) * spread, rs.uniform(-110, 110) * spread, rs.uniform(650, 1000)])
                if (sid, iid, obj_id) == OUTSIDE and k == 0:
                    t = np.array([2600.0, 300.0, 800.0])
                gts.append(dict(obj_id=obj_id, R=R, t=t, valid=not (sid == 6 and iid == 4 and obj_id == 2)))
                d = render_depth(models[obj_id]["verts"], models[obj_id]["faces"], R, t, K[0, 0], K[1, 1], K[0, 2], K[1, 2], H, W).astype(np.float64)
                z = np.where((d > 0) & (d < z), d, z)
                if rs.rand() < 0.08 and (sid, iid, obj_id) not in (BEHIND, OUTSIDE):
                    continue  # a missed object
                for e in range(1 + (rs.rand() < 0.7) + (rs.rand() < 0.4) + extra_estimates):
                    level = rs.choice([0.0, 0.01, 0.03, 0.08, 0.3])
                    Re = R @ rot(rs.randn(3), level * 2.0)
                    syms = models[obj_id]["symmetries"]
                    if len(syms) > 1 and rs.rand() < 0.6:  # a symmetric twin: Re o S, te stays
                        s = syms[rs.randint(1, len(syms))]
                        Re, te0 = Re @ s["R"], Re @ s["t"]
                    else:
                        te0 = np.zeros(3)
                    te = t + te0 + rs.randn(3) * level * 150
                    if (sid, iid, obj_id) == BEHIND and e == 0:
                        te = te * np.array([1.0, 1.0, -1.0])
                    results.append(dict(scene_id=sid, im_id=iid, obj_id=obj_id, score=float(rs.rand()) * (1.0 if e == 0 else 0.6), R=Re, t=te, time=0.1))
            back = 1700.0 if sid == 7 else 0.0
            z = np.where(np.isinf(z), back, z)
            if iid % 3 == 2:  # an occluder slab 130 mm in front of the second object, over the left part of its silhouette
                u0 = int(K[0, 0] * gts[1]["t"][0] / gts[1]["t"][2] + K[0, 2])
                z[:, max(0, u0 - 60):max(0, u0)] = gts[1]["t"][2] - 130.0
            z = np.where(z > 0, z + rs.randn(H, W), 0.0)
            z[rs.rand(H, W) < 0.02] = 0.0
            scene_gt[sid][iid] = gts
            depth_images[sid][iid] = z.astype(np.float32)
    return models, scene_gt, cameras, results, float(W), depth_images, (W, H)


def large_case_facts(out):
    """What an `average_recall` result of the large case must show for the equality tests to mean something: recalls strictly between
    0 and 1 and growing with the threshold for every error, and VSD recalls that differ between the tightest and the loosest tau."""
    facts = {}
    for k in ("recalls_mssd", "recalls_mspd"):
        r = out[k]
        facts[k] = 0.0 < r[0] < r[-1] < 1.0 and len(set(r)) >= 4
    v = np.asarray(out["recalls_vsd"])
    facts["recalls_vsd"] = bool(0.0 < v.min() < v.max() < 1.0 and len(np.unique(v)) >= 8 and v[0, 0] < v[-1, -1])
    return facts


# ---- the same problem as a BOP dataset folder ------------------------------------------------------------------------------------
def write_ply(path, verts, faces, binary=True, vertex_type="float"):
    """Vertices (with normals, as BOP's models_eval files carry them) and triangular faces, ASCII or binary little-endian."""
    verts, faces = np.asarray(verts, np.float64), np.asarray(faces, np.int32)
    normals = verts / np.maximum(np.linalg.norm(verts, axis=1, keepdims=True), 1e-9)
    head = ["ply", "format %s 1.0" % ("binary_little_endian" if binary else "ascii"), "comment written by tests/bop_score_case.py",
            "element vertex %d" % len(verts)]
    head += ["property %s %s" % (vertex_type, k) for k in ("x", "y", "z", "nx", "ny", "nz")]
    head += ["element face %d" % len(faces), "property list uchar int vertex_indices", "end_header"]
    os.makedirs(osp.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        if binary:
            f.write(np.concatenate([verts, normals], axis=1).astype("<f4" if vertex_type == "float" else "<f8").tobytes())
            rec = np.zeros(len(faces), dtype=[("n", "u1"), ("v", "<i4", (3,))])
            rec["n"], rec["v"] = 3, faces
            f.write(rec.tobytes())
        else:
            for v, n in zip(verts, normals):
                f.write((" ".join(repr(float(x)) for x in (*v, *n)) + "\n").encode("ascii"))
            for tri in faces:
                f.write(("3 %d %d %d\n" % tuple(tri)).encode("ascii"))


def write_dataset(root, case, name="synth", split="test", depth_scale=0.1, skip_image=(6, 1), skip_object=(7, 3, 2), continuous_object=None):
    """Lays `case` (the tuple of `make_large_case` / `make_vsd_case`) out under <root>/<name>: models_eval/*.ply (object 1 ASCII, the
    others binary) + models_info.json, <split>/<scene>/scene_gt.json, scene_camera.json and depth/*.png (uint16, mm / depth_scale),
    test_targets_bop19.json with the instance counts -- WITHOUT image `skip_image` and without object `skip_object[2]` in image
    `skip_object[:2]`, which therefore must not be scored -- and results.csv.  -> (csv path, targets as load_dataset returns them)."""
    from PIL import Image

    models, scene_gt, cameras, results, _, depth_images, _ = case
    base = osp.join(root, name)
    info = {}
    for obj_id, m in models.items():
        write_ply(osp.join(base, "models_eval", f"obj_{obj_id:06d}.ply"), m["verts"], m["faces"], binary=obj_id != 1)
        info[str(obj_id)] = dict(diameter=m["diameter"])
        if len(m["symmetries"]) > 1:
            info[str(obj_id)]["symmetries_discrete"] = [np.block([[s["R"], s["t"].reshape(3, 1)], [np.zeros((1, 3)), np.ones((1, 1))]]).reshape(-1).tolist()
                                                        for s in m["symmetries"][1:]]
        if obj_id == continuous_object:
            info[str(obj_id)]["symmetries_continuous"] = [dict(axis=[0, 0, 1], offset=[0, 0, 0])]
    json.dump(info, open(osp.join(base, "models_eval", "models_info.json"), "w"))
    targets, listed = {}, []
    for sid, ims in scene_gt.items():
        folder = osp.join(base, split, f"{sid:06d}")
        os.makedirs(osp.join(folder, "depth"), exist_ok=True)
        cam, gt = {}, {}
        for iid, gts in ims.items():
            cam[str(iid)] = dict(cam_K=np.asarray(cameras[sid][iid]).reshape(-1).tolist(), depth_scale=depth_scale)
            gt[str(iid)] = [dict(cam_R_m2c=np.asarray(g["R"]).reshape(-1).tolist(), cam_t_m2c=np.asarray(g["t"]).reshape(-1).tolist(), obj_id=g["obj_id"])
                            for g in gts]
            Image.fromarray(np.clip(np.rint(depth_images[sid][iid] / depth_scale), 0, 65535).astype(np.uint16)).save(
                osp.join(folder, "depth", f"{iid:06d}.png"))
            if (sid, iid) == tuple(skip_image):
                continue
            for obj_id in sorted({g["obj_id"] for g in gts}):
                if (sid, iid, obj_id) == tuple(skip_object):
                    continue
                n = sum(g["obj_id"] == obj_id for g in gts)
                targets.setdefault((sid, iid), {})[obj_id] = n
                listed.append(dict(scene_id=sid, im_id=iid, obj_id=obj_id, inst_count=n))
        json.dump(cam, open(osp.join(folder, "scene_camera.json"), "w"))
        json.dump(gt, open(osp.join(folder, "scene_gt.json"), "w"))
    json.dump(listed, open(osp.join(base, "test_targets_bop19.json"), "w"))
    csv = osp.join(root, "out", "results.csv")
    os.makedirs(osp.dirname(csv), exist_ok=True)
    with open(csv, "w") as f:
        f.write("scene_id,im_id,obj_id,score,R,t,time\n")
        for r in results:
            f.write(",".join((str(r["scene_id"]), str(r["im_id"]), str(r["obj_id"]), repr(r["score"]), " ".join(repr(float(v)) for v in r["R"].reshape(-1)),
                              " ".join(repr(float(v)) for v in r["t"]), "0.1")) + "\n")
    return csv, targets
