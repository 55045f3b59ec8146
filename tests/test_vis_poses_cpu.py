"""CPU: the pose visualisation's host side -- the numpy mirrors of the colour rasteriser and of the composition (tests/raster_rgb_np.py, what
the HIP kernels are compared with on the GPU) against bop_toolkit's own `vis_object_poses` (tests/golden/vis_poses.npz, written by
tests/golden/make_vis_poses_golden.py) and against closed-form shading, the PLY reader with vertex colours, and the command's plan."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "vis_poses.npz")


def test_mirror_composition_and_depth_difference_equal_the_toolkit():
    from raster_rgb_np import NumpyColorRenderer, compose
    from vis_poses_case import DELTA, LAYOUT, add_objects, make_scene, scene_facts

    gold = np.load(GOLD)
    ren = add_objects(NumpyColorRenderer(36, 24))
    for name in LAYOUT:
        s = make_scene(name, ren.render_object, 36, 24)
        if name == "main":
            assert all(scene_facts(s).values()), scene_facts(s)
        for resolve in (True, False):
            vis, boxes, ren_depth, diff, stats = compose(s["rgbs"], s["depths"], s["photo"], s["depth"], resolve, DELTA)
            assert np.array_equal(vis, gold[f"{name}_rgb_{int(resolve)}"]), (name, resolve)
            assert np.array_equal(diff, gold[f"{name}_diff_{int(resolve)}"]), (name, resolve)
            assert stats["min"] < 0 < DELTA < stats["max"] and stats["min"] < stats["mean"] < stats["max"]
        if name == "main":
            assert boxes[3] is None and boxes[4][:2] == [0, 0] and boxes[0] == boxes[2]
            near = np.where(s["depths"] > 0, s["depths"], np.inf).min(axis=0)
            assert np.array_equal(ren_depth, np.where(np.isinf(near), 0, near).astype(np.float32))


def test_mirror_depth_equals_the_depth_rasteriser_and_the_lowest_face_index_wins():
    from bop_eval_case import icosphere
    from raster_np import render_depth
    from raster_rgb_np import render_rgbd

    sv, sf = icosphere()
    verts = sv * np.array([100.0, 90.0, 80.0])
    args = (np.eye(3), [20.0, -10.0, 800.0], 40.0, 40.8, 17.2, 11.7, 24, 36)
    d, rgb = render_rgbd(verts, sf, *args, surf_color=(0.2, 0.6, 1.0))
    assert np.array_equal(d, render_depth(verts, sf, *args)) and (d > 0).sum() > 40
    assert ((rgb > 0).any(axis=2) == (d > 0)).all()
    # every face twice, the copy on vertices of another colour: same depth everywhere, the first copy's colour
    cols = np.concatenate([np.tile([1.0, 0.0, 0.0], (len(verts), 1)), np.tile([0.0, 1.0, 0.0], (len(verts), 1))])
    d2, rgb2 = render_rgbd(np.concatenate([verts, verts]), np.concatenate([sf, sf + len(verts)]), *args, colors=cols)
    assert np.array_equal(d2, d) and (rgb2[..., 0][d > 0] > 0).all() and (rgb2[..., 1:] == 0).all()
    d3, rgb3 = render_rgbd(np.concatenate([verts, verts]), np.concatenate([sf + len(verts), sf]), *args, colors=cols)
    assert np.array_equal(d3, d) and (rgb3[..., 1][d > 0] > 0).all() and (rgb3[..., [0, 2]] == 0).all()


def plane(angle, half=200.0):
    """A square in the plane through the origin whose normal makes `angle` with the z axis (turned about x), as two triangles."""
    c, s = np.cos(angle), np.sin(angle)
    corners = np.array([[-half, -half, 0.0], [half, -half, 0.0], [half, half, 0.0], [-half, half, 0.0]])
    return corners @ np.array([[1.0, 0, 0], [0, c, -s], [0, s, c]]).T, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def test_flat_shading_against_the_closed_form():
    """Light at the camera: at the principal point the fragment lies on the optical axis, so the cosine is that of the plane's tilt.  Tilted to
    cosine 0.25 the weight is 0.5 + 0.25; the byte may differ from round(0.75 c 255) by 1 (float32 rounding of the cosine next to a .5 tie).
    Facing the camera the cosine is z / |Pc| >= 0.5 over this field of view, the weight saturates at 1 and the colour comes out as given."""
    from raster_rgb_np import render_rgbd

    color = np.array([0.9, 0.5, 0.2])
    verts, faces = plane(np.arccos(0.25))
    d, rgb = render_rgbd(verts, faces, np.eye(3), [0.0, 0.0, 800.0], 40.0, 40.0, 18.0, 12.0, 24, 36, surf_color=color)
    assert d[12, 18] == 800.0
    assert np.abs(rgb[12, 18].astype(int) - np.round(0.75 * color * 255)).max() <= 1, rgb[12, 18]
    verts, faces = plane(0.0, half=500.0)
    d, rgb = render_rgbd(verts, faces, np.eye(3), [0.0, 0.0, 800.0], 40.0, 40.0, 18.0, 12.0, 24, 36, surf_color=color)
    assert np.allclose(d, 800.0, rtol=1e-6, atol=0) and (rgb == (color * 255 + 0.5).astype(int)).all()
    # ambient alone: a weight that does not saturate dims the colour
    d, dim = render_rgbd(verts, faces, np.eye(3), [0.0, 0.0, 800.0], 40.0, 40.0, 18.0, 12.0, 24, 36, surf_color=color, ambient=0.0)
    assert (dim[12, 18] == rgb[12, 18]).all() and (dim[0, 0] < rgb[0, 0]).all()


def test_undefined_cases_of_the_depth_difference_image_follow_our_rule():
    from raster_rgb_np import depth_diff_image

    ren = np.zeros((4, 6), np.float32)
    ren[1:3, 1:4] = 500.0
    image, stats = depth_diff_image(ren, np.zeros((4, 6), np.float32))  # no valid pixel
    assert stats is None and (image == 0).all()
    image, stats = depth_diff_image(ren, np.where(ren > 0, 493.0, 0.0))  # one positive shifted value: range 0
    assert stats == dict(min=7.0, max=7.0, mean=7.0)
    assert (image[1:3, 1:4] == [255, 51, 51]).all() and image.sum() == 6 * (255 + 51 + 51)
    image, stats = depth_diff_image(np.full((4, 6), 500.0, np.float32), np.full((4, 6), 480.0, np.float32))  # every shifted value 0
    assert stats == dict(min=20.0, max=20.0, mean=20.0) and (image == [0, 51, 51]).all()


def write_colour_ply(path, verts, faces, colors, binary, kind="uchar"):
    head = ["ply", "format %s 1.0" % ("binary_little_endian" if binary else "ascii"), "element vertex %d" % len(verts)]
    head += ["property float %s" % k for k in "xyz"]
    if colors is not None:
        head += ["property %s %s" % (kind, k) for k in ("red", "green", "blue")]
    head += ["element face %d" % len(faces), "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        if binary:
            fields = [(k, "<f4") for k in "xyz"] + ([(k, "u1" if kind == "uchar" else "<f4") for k in "rgb"] if colors is not None else [])
            rec = np.zeros(len(verts), dtype=fields)
            for i, k in enumerate("xyz"):
                rec[k] = verts[:, i]
            if colors is not None:
                for i, k in enumerate("rgb"):
                    rec[k] = colors[:, i]
            f.write(rec.tobytes())
            frec = np.zeros(len(faces), dtype=[("n", "u1"), ("v", "<i4", (3,))])
            frec["n"], frec["v"] = 3, faces
            f.write(frec.tobytes())
        else:
            for i, v in enumerate(verts):
                row = [repr(float(x)) for x in v] + ([str(c) for c in colors[i]] if colors is not None else [])
                f.write((" ".join(row) + "\n").encode("ascii"))
            for tri in faces:
                f.write(("3 %d %d %d\n" % tuple(tri)).encode("ascii"))


@pytest.mark.parametrize("binary", [False, True])
def test_ply_reader_with_vertex_colours(tmp_path, binary):
    from bop_eval_case import icosphere
    from unopose_amd import bop_eval

    sv, sf = icosphere()
    verts = (sv * 50.0).astype(np.float32).astype(np.float64)
    cols = np.random.RandomState(1).randint(0, 256, size=(len(verts), 3))
    path = str(tmp_path / "c.ply")
    write_colour_ply(path, verts, sf, cols, binary)
    got = bop_eval.read_ply_colors(path)
    assert np.array_equal(got["pts"], verts) and np.array_equal(got["faces"], sf) and np.array_equal(got["colors"], cols / 255.0)
    plain = bop_eval.read_ply(path)
    assert sorted(plain) == ["faces", "pts"] and np.array_equal(plain["pts"], verts) and np.array_equal(plain["faces"], sf)
    write_colour_ply(path, verts, sf, cols / 255.0 * 1.25, binary, kind="float")  # floating-point colours are clipped to [0, 1]
    got = bop_eval.read_ply_colors(path)["colors"]
    assert got.max() == 1.0 and np.allclose(got, np.clip(cols / 255.0 * 1.25, 0, 1), atol=1e-6)
    write_colour_ply(path, verts, sf, None, binary)
    got = bop_eval.read_ply_colors(path)
    assert got["colors"] is None and np.array_equal(got["pts"], verts) and sorted(bop_eval.read_ply(path)) == ["faces", "pts"]


def test_palette_paths_and_plan(tmp_path):
    from unopose_amd import vis_poses

    pal = vis_poses.palette([5, 1, 9])
    assert sorted(pal) == [1, 5, 9] and len(set(pal.values())) == 3 and all(0 <= c <= 1 and max(v) == 1.0 for v in pal.values() for c in v)
    assert vis_poses.output_paths("o", "lmo", "test", 2, 31, "png") == ("o/lmo/test/000002/000031.png", "o/lmo/test/000002/000031_depth_diff.png")
    assert vis_poses.default_out_dir("/a/b/r.csv") == "/a/b/vis"
    root = tmp_path / "data"
    (root / "lmo").mkdir(parents=True)
    (root / "lmo" / "test_targets_bop19.json").write_text(json.dumps(
        [dict(scene_id=2, im_id=i, obj_id=o, inst_count=1) for i in (3, 4, 9) for o in (1, 5)] + [dict(scene_id=7, im_id=3, obj_id=1, inst_count=1)]))
    csv = tmp_path / "out" / "r.csv"
    csv.parent.mkdir()
    row = "%d,%d,1,0.5,1 0 0 0 1 0 0 0 1,0 0 800,0.1\n"
    csv.write_text("scene_id,im_id,obj_id,score,R,t,time\n" + row % (2, 3) + row % (2, 3) + row % (2, 9) + row % (7, 3) + row % (8, 1))
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    base = [sys.executable, "-m", "unopose_amd.vis_poses", "--data-dir", str(root), "--dataset", "lmo", "--split", "test", "--print-plan"]
    r = subprocess.run(base, capture_output=True, text=True, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    plan = json.loads(r.stdout.strip().splitlines()[-1])
    assert plan["mode"] == "gt" and plan["n_images"] == 4 and plan["n_estimates"] is None and plan["out_dir"] == "vis_gt_poses" and plan["ext"] == "jpg"
    assert plan["paths"]["split"] == str(root / "lmo" / "test") and plan["first_files"] == [
        "vis_gt_poses/lmo/test/000002/000003.jpg", "vis_gt_poses/lmo/test/000002/000003_depth_diff.jpg"]
    r = subprocess.run(base + ["--results", str(csv), "--scene-ids", "2", "--im-ids", "3", "9", "--ext", "png", "--no-depth-diff", "--n-top", "1"],
                       capture_output=True, text=True, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    plan = json.loads(r.stdout.strip().splitlines()[-1])
    assert plan["mode"] == "est" and plan["n_images"] == 2 and plan["n_estimates"] == 3 and plan["out_dir"] == str(csv.parent / "vis")
    assert plan["first_files"] == [str(csv.parent / "vis" / "lmo" / "test" / "000002" / "000003.png")] and plan["n_top"] == 1


def test_select_poses_follows_the_scorers_selection():
    from unopose_amd import vis_poses

    g = lambda o, z: dict(obj_id=o, R=np.eye(3), t=np.array([0.0, 0.0, z]))  # noqa: E731
    r = lambda sid, iid, o, s: dict(scene_id=sid, im_id=iid, obj_id=o, score=s, R=np.eye(3), t=np.array([0.0, 0.0, 700.0 + s]), time=0.1)  # noqa: E731
    data = dict(scene_gt={1: {0: [g(5, 800.0), g(2, 810.0), g(5, 820.0), g(3, 830.0)], 1: [g(2, 800.0)]}}, cameras={1: {0: np.eye(3), 1: np.eye(3)}},
                targets={(1, 0): {5: 2, 2: 1}})
    gt = vis_poses.select_poses(data)
    assert list(gt) == [(1, 0)] and [p["label"] for p in gt[(1, 0)]] == ["2:1", "5:0", "5:2"]  # object 3 and image 1 are no targets
    rows = [r(1, 0, 5, 0.2), r(1, 0, 5, 0.9), r(1, 0, 5, 0.5), r(1, 0, 2, 0.3), r(1, 0, 2, 0.4), r(1, 0, 3, 0.99), r(1, 1, 2, 0.9)]
    est = vis_poses.select_poses(data, rows, n_top=-1)
    assert [p["label"] for p in est[(1, 0)]] == ["2:0.40", "5:0.90", "5:0.50"]
    assert [p["label"] for p in vis_poses.select_poses(data, rows, n_top=1)[(1, 0)]] == ["2:0.40", "5:0.90"]
    assert vis_poses.select_poses(data, rows, scene_ids=[2]) == {}


def test_cli_plan_is_unchanged_without_vis_and_names_the_folder_with_it(tmp_path):
    BASE = dict(model=dict(cfg=dict(coarse_npoint=196)), dataloader=dict(test=dict(dataset=dict(eval_dataset_name="ycbv", detetion_path="d.json", cfg=dict(img_size=224)))),
                test=dict(amp=dict(enabled=False), instance_batch_size=16, save_results_only=False), misc=dict(output_dir="output/unopose", load_from=""),
                bop_eval=dict(split="test"))
    cfgf = tmp_path / "c.json"
    cfgf.write_text(json.dumps(BASE))
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "unopose_amd.cli", "--config-file", str(cfgf), "--print-plan"]
    plans = []
    for extra in ([], ["--vis"], ["--vis", "shown"], ["--vis", "misc.load_from=/x/ckpt_12.pth"]):
        r = subprocess.run(cmd + extra + ["misc.load_from=/x/ckpt_12.pth"], capture_output=True, text=True, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stderr
        plans.append(json.loads(r.stdout.strip().splitlines()[-1]))
    assert plans[0] == dict(save_path="output/unopose/inference_ckpt_12/ycbv/result_ycbv-test.csv", dataset="ycbv", checkpoint="/x/ckpt_12.pth", amp=False,
                            instance_batch_size=16, num_gpus=1, device_prep=False, eval=False)
    assert plans[1] == dict(plans[0], vis_dir="output/unopose/inference_ckpt_12/ycbv/vis") == plans[3]
    assert plans[2] == dict(plans[0], vis_dir="shown")
