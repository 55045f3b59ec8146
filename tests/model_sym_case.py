"""Models with known rotation groups for the symmetry search (unopose_amd/model_sym.py), as surface lattices built so that a true symmetry
maps the vertex set onto itself (deviation ~ 1e-16 d), a brute-force statement of the deviation, and a small dataset folder.

| model                                           | vertices | group order incl. identity | continuous axes |
| box 40 x 60 x 90, grid 10                       | 230      | 4                          | 0               |
| square prism 50 x 50 x 90                       | 232      | 8                          | 0               |
| cube 60^3                                       | 218      | 24                         | 0               |
| tetrahedron, edges in 8 steps                   | 130      | 12                         | 0               |
| cylinder r 30, h 70, 96 per ring                | 1346     | 2 (one flip)               | 1               |
| cone, same rings                                | 962      | 1                          | 1               |
| the box sheared by quadratic terms (asymmetric) | 230      | 1                          | 0               |
Half the ring spacing of the cylinder is 0.011 d, under the default tolerance 0.02 d: hence 96 points per ring."""
import json
import math
import os
import os.path as osp

import numpy as np

TOL, AXES, MAX_ORDER = 0.02, 1024, 6


def box(sx, sy, sz, grid=10.0):
    ax = [np.arange(-s / 2.0, s / 2.0 + 1e-9, grid) for s in (sx, sy, sz)]
    g = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3)
    on = (np.abs(np.abs(g) - np.array([sx, sy, sz]) / 2.0) < 1e-9).any(axis=1)
    return g[on]


def sheared_box():
    p = box(40, 60, 90)
    x, y, z = p.T
    return np.stack([x + 0.004 * y * y + 0.002 * z * z, y + 0.003 * z * x + 0.002 * z * z, z + 0.005 * x * y + 0.004 * x * x], axis=1)


def tetrahedron(steps=8, scale=40.0):
    corners = scale * np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]])
    pts = set()
    for f in ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)):
        for i in range(steps + 1):
            for j in range(steps + 1 - i):
                q = (i * corners[f[0]] + j * corners[f[1]] + (steps - i - j) * corners[f[2]]) / steps  # integers / 8: exact
                pts.add(tuple(float(v) for v in q))
    return np.array(sorted(pts))


def _ring(r, z, n=96):
    a = 2.0 * math.pi * np.arange(n) / n
    return np.stack([r * np.cos(a), r * np.sin(a), np.full(n, z)], axis=1)


def cylinder(r=30.0, h=70.0, n=96):
    rings = [_ring(r, z, n) for z in np.arange(-h / 2.0, h / 2.0 + 1e-9, 10.0)]
    for z in (-h / 2.0, h / 2.0):
        rings += [_ring(r * k / 4.0, z, n) for k in (1, 2, 3)] + [np.array([[0.0, 0.0, z]])]
    return np.concatenate(rings)


def cone(r=30.0, h=70.0, n=96):
    rings = [_ring(r * (1.0 - k / 7.0), h * k / 7.0, n) for k in range(7)] + [np.array([[0.0, 0.0, h]])]
    rings += [_ring(r * k / 4.0, 0.0, n) for k in (1, 2, 3)] + [np.array([[0.0, 0.0, 0.0]])]
    return np.concatenate(rings)


# name -> (builder, vertices, group order with the identity, continuous axes)
MODELS = {
    "box": (lambda: box(40, 60, 90), 230, 4, 0),
    "prism": (lambda: box(50, 50, 90), 232, 8, 0),
    "cube": (lambda: box(60, 60, 60), 218, 24, 0),
    "tetrahedron": (tetrahedron, 130, 12, 0),
    "cylinder": (cylinder, 1346, 2, 1),
    "cone": (cone, 962, 1, 1),
    "sheared_box": (sheared_box, 230, 1, 0),
}
POLYHEDRA = ("box", "prism", "cube", "tetrahedron", "sheared_box")


def random_rotation(seed):
    q, r = np.linalg.qr(np.random.default_rng(seed).standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else -q


def posed(pts, seed=11):
    """The model after a random rotation and a translation of tens of units."""
    rng = np.random.default_rng(seed + 1000)
    return pts @ random_rotation(seed).T + rng.uniform(20.0, 60.0, 3) * rng.choice([-1.0, 1.0], 3)


def noisy(pts, sigma=0.02, seed=3):
    """The model as a scan or a remeshing would leave it: Gaussian noise on every coordinate, so that no symmetry is exact."""
    return pts + np.random.default_rng(seed).normal(0.0, sigma, pts.shape)


def noisy_facts(res, pts, tol=TOL):
    """(group order with the identity, continuous axes) of a result on a noisy model: every listed transform is a rotation that deviates by at
    most tol d; the set is closed only as exactly as the noise lets the axes be found, so a product must match a member to 0.02."""
    from unopose_amd.model_info import extent_host
    from unopose_amd.model_sym import sym_deviation_host

    assert res["report"]["status"] == "ok"
    mats = np.array([np.asarray(m).reshape(4, 4) for m in res["symmetries_discrete"]]).reshape(-1, 4, 4)
    if len(mats):
        assert (sym_deviation_host(pts, mats) <= tol * extent_host(pts)[2]).all()
    if not res["symmetries_continuous"]:
        group = [np.eye(3)] + [T[:3, :3] for T in mats]
        for a in group:
            assert np.abs(a.T @ a - np.eye(3)).max() <= 1e-12 and np.linalg.det(a) > 0
            for b in group:
                assert min(np.abs(a @ b - g).max() for g in group) <= 0.02
    return len(mats) + 1, len(res["symmetries_continuous"])


def model(name, pose):
    pts = MODELS[name][0]()
    return posed(pts) if pose else pts


def brute_deviation(pts, T):
    """The two-sided deviation of ONE 4 x 4 transform by a double loop in plain Python floats with numpy's matrix product: independent of the
    specification's order of operations, so equal to it to rounding only."""
    p = np.asarray(pts, np.float64)
    T = np.asarray(T, np.float64).reshape(4, 4)
    worst = 0.0
    for M in (T, np.linalg.inv(T)):
        q = p @ M[:3, :3].T + M[:3, 3]
        for a in q:
            worst = max(worst, min(math.dist(a, b) for b in p))
    return worst


def group_facts(res, pts, tol=TOL):
    """What a `find_symmetries` result must show whatever the model: rotations that fix the centre, deviate by at most tol d and form a set
    closed under composition -> (group order with the identity, continuous axes)."""
    from unopose_amd.model_info import extent_host

    d, c = extent_host(pts)[2], np.asarray(res["report"]["centre"]) if "centre" in res["report"] else None
    mats = [np.asarray(m).reshape(4, 4) for m in res["symmetries_discrete"]]
    for T in mats:
        R = T[:3, :3]
        assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-12 and np.linalg.det(R) > 0
        assert np.abs(R @ c + T[:3, 3] - c).max() <= 1e-9 * max(1.0, np.abs(c).max())
        assert np.abs(R - np.eye(3)).max() > 1e-3, "the identity is listed"
        assert (T[3] == [0.0, 0.0, 0.0, 1.0]).all()
    if not res["symmetries_continuous"]:
        group = [np.eye(3)] + [T[:3, :3] for T in mats]
        for a in group:
            for b in group:
                assert min(np.abs(a @ b - g).max() for g in group) <= 1e-6
    for s in res["symmetries_continuous"]:
        assert abs(np.linalg.norm(s["axis"]) - 1.0) <= 1e-12 and np.allclose(s["offset"], c, atol=0, rtol=0)
    assert len(res["report"]["symmetries"]) == len(mats)
    return len(mats) + 1, len(res["symmetries_continuous"]), d


def write_dataset(root, name="sym", split="test"):
    """<root>/<name>: models_eval with object 1 = the box and object 2 = the sheared box (no models_info.json), one scene with one image that
    shows both, the targets, and out/results.csv whose box estimate is the ground truth composed with a half-turn about the box's z axis and
    whose sheared-box estimate is slightly off.  -> (csv path, the box's diameter)."""
    from bop_score_case import write_ply
    from PIL import Image

    from unopose_amd.model_info import extent_host

    base = osp.join(root, name)
    clouds = {1: box(40, 60, 90), 2: sheared_box()}
    for o, p in clouds.items():
        write_ply(osp.join(base, "models_eval", f"obj_{o:06d}.ply"), p, np.array([[0, 1, 2]]), binary=True, vertex_type="double")
    K = [600.0, 0.0, 160.0, 0.0, 600.0, 120.0, 0.0, 0.0, 1.0]
    gts = {1: (random_rotation(3), np.array([-60.0, 10.0, 700.0])), 2: (random_rotation(4), np.array([70.0, -20.0, 800.0]))}
    folder = osp.join(base, split, "000001")
    os.makedirs(osp.join(folder, "depth"), exist_ok=True)
    Image.fromarray(np.full((240, 320), 7000, np.uint16)).save(osp.join(folder, "depth", "000000.png"))
    json.dump({"0": dict(cam_K=K, depth_scale=0.1)}, open(osp.join(folder, "scene_camera.json"), "w"))
    json.dump({"0": [dict(cam_R_m2c=R.reshape(-1).tolist(), cam_t_m2c=t.tolist(), obj_id=o) for o, (R, t) in gts.items()]},
              open(osp.join(folder, "scene_gt.json"), "w"))
    json.dump([dict(scene_id=1, im_id=0, obj_id=o, inst_count=1) for o in gts], open(osp.join(base, "test_targets_bop19.json"), "w"))
    est = {1: (gts[1][0] @ np.diag([-1.0, -1.0, 1.0]), gts[1][1]), 2: (gts[2][0], gts[2][1] + np.array([1.0, -2.0, 3.0]))}
    csv = osp.join(root, "out", "results.csv")
    os.makedirs(osp.dirname(csv), exist_ok=True)
    with open(csv, "w") as f:
        f.write("scene_id,im_id,obj_id,score,R,t,time\n")
        for o, (R, t) in est.items():
            f.write(",".join(("1", "0", str(o), "1.0", " ".join(repr(float(v)) for v in R.reshape(-1)), " ".join(repr(float(v)) for v in t), "0.1")) + "\n")
    return csv, extent_host(clouds[1])[2]
