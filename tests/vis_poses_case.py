"""Scenes for the pose visualisation (unopose_amd/ops/vis.py, csrc/vis.hip, csrc/raster_color.hip), shared by
tests/golden/make_vis_poses_golden.py (the toolkit's `vis_object_poses` on them) and the tests.  Meshes and cameras are those of
tests/gt_info_case.py; geometry is given in pixels of a W x H image, so the same scenes exist on every canvas.  In the scene "main": an
occluding pair, two poses at exactly equal depth (the same mesh under two colours in one pose), a pose that draws nothing, a box that
touches the image border, overlapping boxes, photo pixels of 255 under a bright render and a box line, captured depth without a
measurement, and rendered depth on both sides of delta around the captured one.  "plain" is an image with a single pose and no depth holes."""
import numpy as np

from gt_info_case import BACKGROUND, cameras_for, make_models

DELTA = 15.0
SIZES = ((36, 24), (37, 23))
# obj_id -> (mesh of gt_info_case.make_models, surface colour or None for per-vertex colours)
OBJECTS = {1: (1, (0.95, 0.35, 0.1)), 2: (2, None), 3: (1, (0.1, 0.9, 1.0)), 4: (2, (1.0, 1.0, 1.0))}
# scene -> (camera, [(obj_id, u / W, v / H, z)]); pose order is drawing order
LAYOUT = {
    "main": (0, [(1, 0.36, 0.52, 800.0), (2, 0.50, 0.48, 700.0), (3, 0.36, 0.52, 800.0), (2, 0.5, 0.5, -800.0), (4, 0.04, 0.10, 760.0),
                 (4, 0.80, 0.55, 900.0)]),
    "plain": (1, [(2, 0.55, 0.45, 650.0)]),
}


def vertex_colors(verts):
    """Per-vertex colours in [0, 1] that vary over the mesh."""
    v = np.asarray(verts, np.float64)
    c = 0.5 + 0.5 * np.sin(v / np.abs(v).max() * np.array([2.0, 3.0, 5.0]) + np.array([0.3, 1.1, 2.0]))
    return np.clip(c, 0.0, 1.0)


def add_objects(renderer):
    """The objects of OBJECTS into a renderer with add_object(obj_id, verts, faces, colors=, surf_color=)."""
    meshes = make_models()
    for obj_id, (mesh, surf) in OBJECTS.items():
        m = meshes[mesh]
        if surf is None:
            renderer.add_object(obj_id, m["verts"], m["faces"], colors=vertex_colors(m["verts"]))
        else:
            renderer.add_object(obj_id, m["verts"], m["faces"], surf_color=surf)
    return renderer


def scene_poses(name, W, H):
    """-> K, [dict(obj_id, R, t)]."""
    cam, objects = LAYOUT[name]
    K = cameras_for(W, H)[cam]
    poses = []
    for k, (obj_id, u, v, dist) in enumerate(objects):
        ang = 0.5 * k + 0.2
        R = np.array([[np.cos(ang), -np.sin(ang), 0.0], [np.sin(ang), np.cos(ang), 0.0], [0.0, 0.0, 1.0]])
        if obj_id == 3:  # the twin of pose 0: same mesh, same pose, another colour
            R = poses[0]["R"]
        poses.append(dict(obj_id=obj_id, R=R, t=np.array([(u * W - K[0, 2]) / K[0, 0] * abs(dist), (v * H - K[1, 2]) / K[1, 1] * abs(dist), dist])))
    return K, poses


def make_scene(name, render_object, W=36, H=24, seed=5):
    """render_object(obj_id, R, t, fx, fy, cx, cy) -> {"rgb", "depth"} (any renderer of the toolkit's interface with `add_objects` done).
    -> dict(K, poses, rgbs (P,H,W,3) uint8, depths (P,H,W) float32, photo (H,W,3) uint8, depth (H,W) float32 in mm)."""
    rs = np.random.RandomState(seed + len(name))
    K, poses = scene_poses(name, W, H)
    outs = [render_object(p["obj_id"], p["R"], p["t"], K[0, 0], K[1, 1], K[0, 2], K[1, 2]) for p in poses]
    rgbs, depths = np.stack([o["rgb"] for o in outs]).astype(np.uint8), np.stack([o["depth"] for o in outs]).astype(np.float32)
    near = np.where(depths > 0, depths, np.inf).min(axis=0)
    captured = np.where(np.isinf(near), BACKGROUND, near).astype(np.float64)
    captured += np.where(np.arange(W)[None, :] < W // 2, 30.0, -30.0) + np.round(rs.randn(H, W))  # the render 30 mm in front of / behind the scene
    photo = rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    if name == "main":
        captured[rs.rand(H, W) < 0.08] = 0.0  # no measurement
        ys, xs = (rgbs[1] > 0).any(axis=2).nonzero()  # the photo is white over the bounding box of pose 1
        photo[ys.min():ys.max() + 1, xs.min():xs.max() + 1] = 255
    return dict(K=K, poses=poses, rgbs=rgbs, depths=depths, photo=photo, depth=captured.astype(np.float32))


def scene_facts(s):
    """What the scene "main" must contain for the tests to mean something -> {fact: bool}."""
    rgbs, depths, photo, depth = s["rgbs"], s["depths"], s["photo"], s["depth"]
    P, H, W, _ = rgbs.shape
    drawn = (rgbs > 0).any(axis=3)
    box = lambda p: (lambda ys, xs: (xs.min(), ys.min(), xs.max(), ys.max()))(*drawn[p].nonzero())  # noqa: E731
    overlap = lambda a, b: a[0] <= b[2] and b[0] <= a[2] and a[1] <= b[3] and b[1] <= a[3]  # noqa: E731
    both = (depths[0] > 0) & (depths[1] > 0)
    near = np.where(depths > 0, depths, np.inf).min(axis=0)
    near = np.where(np.isinf(near), 0, near)
    valid = (near > 0) & (depth > 0)
    diff = near - depth
    b1 = box(1)
    line = np.zeros((H, W), bool)
    line[b1[1]:b1[3] + 1, [b1[0], b1[2]]] = True
    line[[b1[1], b1[3]], b1[0]:b1[2] + 1] = True
    return {
        "occluding pair": bool(both.any() and (depths[1][both] < depths[0][both]).any()),
        "equal depth": bool(np.array_equal(depths[0], depths[2]) and (depths[0] > 0).sum() > 20 and not np.array_equal(rgbs[0], rgbs[2])),
        "draws nothing": bool(not drawn[3].any() and not (depths[3] > 0).any()),
        "border": bool(box(4)[0] == 0 and box(4)[1] == 0),
        "overlapping boxes": bool(overlap(box(0), box(1))),
        "saturation": bool((line & drawn[1] & (photo == 255).all(axis=2) & (0.5 * 255 + 0.5 * rgbs[1].max(axis=2) + 76 > 255)).any()),
        "invalid depth": bool(((depth == 0) & (near > 0)).any()),
        "both sides of delta": bool((diff[valid] < DELTA).any() and (diff[valid] >= DELTA).any() and (diff[valid] < 0).any()),
    }
