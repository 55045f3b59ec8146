"""Expected views and scene files for `unopose_amd.view_sampler` / `unopose_amd.render_train` from the REFERENCE's vendored bop_toolkit_lib:
    python tests/golden/make_render_train_golden.py <reference checkout>
        ->  tests/golden/render_train_views.npz, tests/golden/render_train_scene_camera.json, tests/golden/render_train_scene_gt.json
* `view_sampler.sample_views` for every case of CASES: hinterstoisser at 12, 42 and 162 points and fibonacci at 9 and 10 (raised to 11) over
  the whole sphere, the upper hemisphere of both modes, and ranges whose four bounds ARE the azimuth and the elevation of sampled points, so
  that only a closed interval keeps those points.  Stored per case: the arguments, R (n,3,3), t (n,3), the level list (of the unfiltered
  points) and the counts;
* the text `inout.save_scene_camera` / `inout.save_scene_gt` write for the first three views of the 42-point sphere at 400 mm, put together
  as scripts/render_train_imgs.py:185-191 puts them together.
`imageio`, `png` and `cv2` (file formats `inout` imports and these calls never use) are stand-in modules.  Arrays and JSON only.
The generator asserts that the cases contain what the tests rely on, so the fixture cannot quietly lose it."""
import math
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "third_party", "bop_toolkit")):
    sys.exit(__doc__)
sys.path.insert(0, os.path.join(sys.argv[1], "third_party", "bop_toolkit"))
for absent in ("imageio", "png", "cv2"):
    try:
        __import__(absent)
    except ImportError:
        sys.modules[absent] = types.ModuleType(absent)

from bop_toolkit_lib import inout, view_sampler  # noqa: E402

FULL_AZ, FULL_EL = (0.0, 2.0 * math.pi), (-0.5 * math.pi, 0.5 * math.pi)
JSON_K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
JSON_DEPTH_SCALE, JSON_OBJ_ID, JSON_RADIUS = 0.1, 5, 400.0


def angles(pt):
    """Azimuth and elevation as sample_views computes them."""
    az = math.atan2(pt[1], pt[0])
    if az < 0:
        az += 2.0 * math.pi
    el = math.acos(np.linalg.norm([pt[0], pt[1], 0]) / np.linalg.norm(pt))
    return az, (-el if pt[2] < 0 else el)


def on_sample_bounds(n, radius):
    """Ranges whose bounds are angles of the sphere's own points: from the 2nd to the 2nd-last distinct elevation above the equator band, and
    between two sampled azimuths."""
    pts, _ = view_sampler.hinter_sampling(n, radius=radius)
    az, el = zip(*(angles(p) for p in pts))
    els, azs = sorted(set(el)), sorted(set(az))
    return (azs[1], azs[-3]), (els[2], els[-2])


def main():
    az42, el42 = on_sample_bounds(42, 400.0)
    cases = dict(
        hinter12=(12, 1.0, FULL_AZ, FULL_EL, "hinterstoisser"), hinter42=(42, 400.0, FULL_AZ, FULL_EL, "hinterstoisser"),
        hinter162=(162, 650.0, FULL_AZ, FULL_EL, "hinterstoisser"), fib9=(9, 500.0, FULL_AZ, FULL_EL, "fibonacci"),
        fib10=(10, 1.0, FULL_AZ, FULL_EL, "fibonacci"), hinter162_upper=(162, 650.0, FULL_AZ, (0.0, 0.5 * math.pi), "hinterstoisser"),
        fib9_upper=(9, 500.0, FULL_AZ, (0.0, 0.5 * math.pi), "fibonacci"), hinter42_on_samples=(42, 400.0, az42, el42, "hinterstoisser"))
    out = {"names": np.array(sorted(cases))}
    got = {}
    for name, (n, radius, az, el, mode) in cases.items():
        views, levels = view_sampler.sample_views(n, radius, az, el, mode)
        got[name] = views, levels
        out[name + "_args"] = np.array([n, radius, az[0], az[1], el[0], el[1]], np.float64)
        out[name + "_mode"] = np.array(mode)
        out[name + "_R"] = np.array([v["R"] for v in views], np.float64).reshape(-1, 3, 3)
        out[name + "_t"] = np.array([v["t"] for v in views], np.float64).reshape(-1, 3)
        out[name + "_levels"] = np.array(levels, np.int64)
        print(name, len(views), "views of", len(levels), "points, levels", sorted(set(levels)))

    # what the tests rely on
    count = lambda name: len(got[name][0])  # noqa: E731
    assert [count(k) for k in ("hinter12", "hinter42", "hinter162", "fib9", "fib10")] == [12, 42, 162, 9, 11]
    assert 0 < count("hinter162_upper") < 162 and 0 < count("fib9_upper") < 9
    for name in ("hinter42", "hinter162"):  # both poles: the camera looks along -z / +z, the side vector falls back to (1, 0, 0)
        pts, _ = view_sampler.hinter_sampling(cases[name][0], radius=cases[name][1])
        poles = [i for i, p in enumerate(pts) if p[0] == 0 and p[1] == 0]
        assert len(poles) == 2 and {float(np.sign(pts[i][2])) for i in poles} == {-1.0, 1.0}, name
        out[name + "_poles"] = np.array(poles, np.int64)
        assert all(np.array_equal(out[name + "_R"][i][0], [1.0, 0.0, 0.0]) for i in poles)
    # the closed interval: points sit exactly on each of the four bounds and are kept; an open interval would lose them
    pts, _ = view_sampler.hinter_sampling(42, radius=400.0)
    inside = [angles(p) for p in pts if az42[0] <= angles(p)[0] <= az42[1] and el42[0] <= angles(p)[1] <= el42[1]]
    assert len(inside) == count("hinter42_on_samples") and 0 < len(inside) < 42
    strictly = [a for a in inside if az42[0] < a[0] < az42[1] and el42[0] < a[1] < el42[1]]
    assert len(strictly) < len(inside), "no point on a bound"
    assert any(a[1] == el42[0] for a in inside) and any(a[1] == el42[1] for a in inside), "no point on an elevation bound"
    # under a restricted range the list is still the whole sphere's: longer than the views it is indexed by
    assert len(got["hinter162_upper"][1]) == 162 > count("hinter162_upper")

    # the three-view scene files, as scripts/render_train_imgs.py fills them
    views, levels = view_sampler.sample_views(42, JSON_RADIUS, FULL_AZ, FULL_EL, "hinterstoisser")
    scene_camera, scene_gt = {}, {}
    for im_id, view in enumerate(views[:3]):
        scene_camera[im_id] = {"cam_K": JSON_K.copy(), "depth_scale": JSON_DEPTH_SCALE, "view_level": int(levels[im_id])}
        scene_gt[im_id] = [{"cam_R_m2c": view["R"], "cam_t_m2c": view["t"], "obj_id": int(JSON_OBJ_ID)}]
    inout.save_scene_camera(os.path.join(HERE, "render_train_scene_camera.json"), scene_camera)
    inout.save_scene_gt(os.path.join(HERE, "render_train_scene_gt.json"), scene_gt)
    out["json_K"], out["json_args"] = JSON_K, np.array([JSON_DEPTH_SCALE, JSON_OBJ_ID, JSON_RADIUS])
    np.savez_compressed(os.path.join(HERE, "render_train_views.npz"), **out)
    print(open(os.path.join(HERE, "render_train_scene_gt.json")).read())


if __name__ == "__main__":
    main()
