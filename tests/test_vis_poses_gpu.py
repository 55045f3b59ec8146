"""GPU: the HIP colour rasteriser (csrc/raster_color.hip through render.HipColorRenderer), the composition kernels (csrc/vis.hip through
ops.compose_poses) and the command `unopose_amd.vis_poses`, bit for bit against the numpy mirrors of tests/raster_rgb_np.py -- which
tests/test_vis_poses_cpu.py pins to bop_toolkit's own `vis_object_poses` -- and against tests/golden/vis_poses.npz directly."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((36, 24), (37, 23))


@functools.lru_cache(maxsize=None)
def mesh(colored):
    """Mesh 1 of gt_info_case with a degenerate face (a repeated vertex) and a zero-area sliver in front, and either one surface colour
    or per-vertex colours."""
    from gt_info_case import make_models
    from vis_poses_case import vertex_colors

    m = make_models()[1]
    verts = np.concatenate([m["verts"], [[0.0, 0.0, -150.0], [10.0, 0.0, -150.0], [20.0, 0.0, -150.0]]])
    n = len(m["verts"])
    faces = np.concatenate([[[0, 0, 5], [n, n + 1, n + 2]], m["faces"]]).astype(np.int32)
    return verts, faces, (vertex_colors(verts) if colored else None), (None if colored else (0.95, 0.35, 0.1))


@functools.lru_cache(maxsize=None)
def poses(W, H):
    """Five poses: inside the image, turned, at the left and upper border (partly outside), behind the camera, far to the right (half outside)."""
    from vis_poses_case import scene_poses

    K, ps = scene_poses("main", W, H)
    ps = [ps[0], ps[1], ps[4], ps[3], dict(ps[5], t=ps[5]["t"] + np.array([150.0, 0.0, 0.0]))]
    return [K[0, 0], K[1, 1], K[0, 2], K[1, 2]], np.stack([p["R"] for p in ps]), np.stack([p["t"] for p in ps])


@functools.lru_cache(maxsize=None)
def mirror_renders(W, H, colored):
    from raster_rgb_np import render_rgbd

    verts, faces, cols, surf = mesh(colored)
    k4, Rs, ts = poses(W, H)
    out = [render_rgbd(verts, faces, R, t, *k4, H, W, colors=cols, surf_color=surf or (0.5, 0.5, 0.5)) for R, t in zip(Rs, ts)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


@pytest.mark.parametrize("colored", [False, True])
@pytest.mark.parametrize("P", [1, 5])
@pytest.mark.parametrize("size", SIZES)
def test_colour_rasteriser_equals_the_numpy_mirror_bit_for_bit(size, P, colored):
    from unopose_amd.render import HipColorRenderer, HipDepthRenderer

    W, H = size
    verts, faces, cols, surf = mesh(colored)
    k4, Rs, ts = poses(W, H)
    want_d, want_rgb = mirror_renders(W, H, colored)
    ren, plain = HipColorRenderer(W, H), HipDepthRenderer(W, H)
    ren.add_object(7, verts, faces, colors=cols, surf_color=surf)
    plain.add_object(7, verts, faces)
    d, rgb = ren.render_batch(7, Rs[:P], ts[:P], k4)
    d, rgb = d.cpu().numpy(), rgb.cpu().numpy()
    assert d.shape == (P, H, W) and rgb.shape == (P, H, W, 3) and rgb.dtype == np.uint8
    assert np.array_equal(d, want_d[:P]) and np.array_equal(rgb, want_rgb[:P])
    assert np.array_equal(d, plain.render_batch(7, Rs[:P], ts[:P], k4).cpu().numpy())
    assert (d[0] > 0).sum() > 30 and ((rgb[0] > 0).any(axis=2) == (d[0] > 0)).all()
    if P == 5:
        assert 0 < (d[2] > 0).sum() and (d[2][0] > 0).any() and (d[2][:, 0] > 0).any()  # cut by the upper and the left border
        assert (d[3] == 0).all() and (rgb[3] == 0).all()                                 # behind the camera
        assert (d[4][:, W - 1] > 0).any()                                                # cut by the right border
        if colored:
            assert len(np.unique(rgb[0].reshape(-1, 3), axis=0)) > 20  # interpolated, not one colour per face


def test_duplicated_face_lower_index_wins_on_every_run():
    """Every face twice on vertices of another colour: equal depth at every pixel, so only the key's lower half decides."""
    from gt_info_case import make_models
    from raster_rgb_np import render_rgbd
    from unopose_amd.render import HipColorRenderer

    W, H = 37, 23
    m = make_models()[2]
    v, f, n = np.concatenate([m["verts"], m["verts"]]), m["faces"], len(m["verts"])
    cols = np.concatenate([np.tile([1.0, 0.2, 0.0], (n, 1)), np.tile([0.0, 0.2, 1.0], (n, 1))])
    k4, Rs, ts = poses(W, H)
    ren = HipColorRenderer(W, H)
    for obj_id, faces in ((1, np.concatenate([f, f + n])), (2, np.concatenate([f + n, f]))):
        ren.add_object(obj_id, v, faces, colors=cols)
        want = [render_rgbd(v, faces, R, t, *k4, H, W, colors=cols) for R, t in zip(Rs[:2], ts[:2])]
        first = ren.render_batch(obj_id, Rs[:2], ts[:2], k4)
        again = ren.render_batch(obj_id, Rs[:2], ts[:2], k4)
        for got in (first, again):
            assert np.array_equal(got[0].cpu().numpy(), np.stack([w[0] for w in want])) and np.array_equal(got[1].cpu().numpy(), np.stack([w[1] for w in want]))
        rgb = first[1].cpu().numpy()
        drawn = first[0].cpu().numpy() > 0
        assert drawn.sum() > 60 and (rgb[..., 0 if obj_id == 1 else 2][drawn] > 0).all() and (rgb[..., 2 if obj_id == 1 else 0] == 0).all()


def test_render_into_a_stack_and_argument_checks():
    import torch

    from unopose_amd.render import HipColorRenderer

    W, H = 36, 24
    verts, faces, cols, surf = mesh(False)
    k4, Rs, ts = poses(W, H)
    want_d, want_rgb = mirror_renders(W, H, False)
    ren = HipColorRenderer(W, H)
    ren.add_object(1, verts, faces, surf_color=surf)
    depths = torch.full((5, H, W), -1.0, device="cuda")
    rgbs = torch.full((5, H, W, 3), 9, dtype=torch.uint8, device="cuda")
    ren.render_batch(1, Rs[:2], ts[:2], k4, out=(depths[:2], rgbs[:2]))
    ren.render_batch(1, Rs[2:], ts[2:], k4, out=(depths[2:], rgbs[2:]))
    assert np.array_equal(depths.cpu().numpy(), want_d) and np.array_equal(rgbs.cpu().numpy(), want_rgb)
    one = ren.render_object(1, Rs[0], ts[0], *k4)
    assert np.array_equal(one["depth"], want_d[0]) and np.array_equal(one["rgb"], want_rgb[0])
    with pytest.raises(RuntimeError, match="out must hold"):
        ren.render_batch(1, Rs[:2], ts[:2], k4, out=(depths[:3], rgbs[:2]))
    with pytest.raises(ValueError):
        ren.add_object(2, verts, faces, colors=np.zeros((len(verts), 3)), surf_color=surf)
    with pytest.raises(ValueError):
        ren.add_object(2, verts, faces, colors=np.full((len(verts), 3), 1.5))
    from unopose_amd._lib import call, ptr, stream_ptr

    v, f = ren.models[1][:2]
    keys = torch.empty(H * W, dtype=torch.int64, device="cuda")
    Rt, K4 = torch.zeros(1, 12, device="cuda"), torch.ones(1, 4, device="cuda")
    for bad in (dict(P=0), dict(H=0), dict(F=0), dict(P=65536)):  # nothing is launched on bad sizes
        a = dict(dict(P=1, H=H, W=W, F=f.shape[0]), **bad)
        with pytest.raises(RuntimeError, match="render_color: bad sizes"):
            call("unopose_render_color", ptr(v), v.shape[0], ptr(f), a["F"], None, 0.5, 0.5, 0.5, 0.5, ptr(Rt), ptr(K4), a["P"], a["H"], a["W"], ptr(keys),
                 ptr(depths), ptr(rgbs), stream_ptr())
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def scene(name, W, H):
    """The scene rendered by the HIP rasteriser (equal to the mirror's renders, asserted here once)."""
    from raster_rgb_np import NumpyColorRenderer
    from unopose_amd.render import HipColorRenderer
    from vis_poses_case import add_objects, make_scene

    s = make_scene(name, add_objects(HipColorRenderer(W, H)).render_object, W, H)
    m = make_scene(name, add_objects(NumpyColorRenderer(W, H)).render_object, W, H)
    for k in ("rgbs", "depths", "photo", "depth"):
        assert np.array_equal(s[k], m[k]), k
    return s


def on_gpu(*arrays):
    import torch

    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


@pytest.mark.parametrize("resolve", [True, False])
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", ["main", "plain"])
def test_composition_equals_the_mirror_and_the_toolkit(name, size, resolve):
    from raster_rgb_np import compose
    from unopose_amd.ops import compose_poses
    from vis_poses_case import DELTA

    W, H = size
    s = scene(name, W, H)
    want = compose(s["rgbs"], s["depths"], s["photo"], s["depth"], resolve, DELTA)
    vis, boxes, ren_depth, diff, stats = compose_poses(*on_gpu(s["rgbs"], s["depths"], s["photo"], s["depth"]), resolve_visib=resolve, delta=DELTA)
    assert np.array_equal(vis.cpu().numpy(), want[0]) and boxes == want[1] and np.array_equal(ren_depth.cpu().numpy(), want[2])
    assert np.array_equal(diff.cpu().numpy(), want[3])
    # minimum and maximum have no order; the mean is a float64 sum of at most H W float32 values in another order: relative 2^-53 H W
    assert stats["min"] == want[4]["min"] and stats["max"] == want[4]["max"] and abs(stats["mean"] - want[4]["mean"]) <= 1e-12 * max(abs(stats["min"]), stats["max"])
    if (W, H) == (36, 24):
        gold = np.load(os.path.join(ROOT, "tests", "golden", "vis_poses.npz"))
        assert np.array_equal(vis.cpu().numpy(), gold[f"{name}_rgb_{int(resolve)}"]) and np.array_equal(diff.cpu().numpy(), gold[f"{name}_diff_{int(resolve)}"])
    no_depth = compose_poses(*on_gpu(s["rgbs"], s["depths"], s["photo"]), resolve_visib=resolve)
    assert np.array_equal(no_depth[0].cpu().numpy(), want[0]) and no_depth[3] is None and no_depth[4] is None


def test_depth_difference_where_the_toolkit_is_undefined_and_cpu_tensors():
    import torch

    from raster_rgb_np import compose
    from unopose_amd.ops import compose_poses

    W, H = 37, 23
    s = scene("plain", W, H)
    ren = np.where(s["depths"] > 0, s["depths"], np.inf).min(axis=0)
    ren = np.where(np.isinf(ren), 0, ren).astype(np.float32)
    cases = {"no valid pixel": np.zeros((H, W), np.float32), "one positive value": np.where(ren > 0, ren - 7.0, 0).astype(np.float32)}
    for what, captured in cases.items():
        want = compose(s["rgbs"], s["depths"], s["photo"], captured)
        got = compose_poses(*on_gpu(s["rgbs"], s["depths"], s["photo"], captured))
        assert np.array_equal(got[3].cpu().numpy(), want[3]), what
        if what == "no valid pixel":
            assert got[4] is None and want[4] is None and (got[3] == 0).all()
        else:
            assert got[4]["min"] > 6.99 and got[4] == pytest.approx(want[4], rel=1e-12) and (got[3].cpu().numpy()[ren > 0] == [255, 51, 51]).all()
    # a render over the whole image, the same difference everywhere: every shifted value is 0
    rgbs, depths = np.full((1, H, W, 3), 200, np.uint8), np.full((1, H, W), 500.0, np.float32)
    got = compose_poses(*on_gpu(rgbs, depths, s["photo"], np.full((H, W), 480.0, np.float32)))
    assert (got[3].cpu().numpy() == [0, 51, 51]).all() and got[4] == dict(min=20.0, max=20.0, mean=20.0) and got[1] == [[0, 0, W - 1, H - 1]]
    with pytest.raises(RuntimeError, match="CPU not supported"):
        compose_poses(torch.from_numpy(rgbs), torch.from_numpy(depths), torch.from_numpy(s["photo"]))
    with pytest.raises(RuntimeError, match="photo"):
        compose_poses(*on_gpu(rgbs, depths, s["photo"][:-1]))


def write_bop_folder(root):
    """The scenes of gt_info_case as a BOP dataset folder with colour images -> (csv path, name)."""
    from PIL import Image

    from bop_score_case import write_dataset
    from gt_info_case import make_models, make_scenes, pose_results
    from raster_np import NumpyRenderer

    W, H = 36, 24
    models = make_models()
    canvas = NumpyRenderer(3 * W, 3 * H)
    for o, m in models.items():
        canvas.add_object(o, m["verts"], m["faces"])
    scene_gt, cameras, depth_images, _ = make_scenes(lambda *a: canvas.render_object(*a)["depth"], W, H)
    results = pose_results(scene_gt, spoil=[(1, 1, 0)])
    results += [dict(r, score=r["score"] - 0.5, t=r["t"] + np.array([0.0, 40.0, 30.0])) for r in results[:3]]  # lower-scored seconds: not drawn
    csv, _ = write_dataset(root, (models, scene_gt, cameras, results, None, depth_images, None), name="synth", skip_image=(-1, -1), skip_object=(-1, -1, -1))
    rs = np.random.RandomState(8)
    for sid, ims in scene_gt.items():
        os.makedirs(os.path.join(root, "synth", "test", f"{sid:06d}", "rgb"))
        for iid in ims:
            Image.fromarray(rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8)).save(os.path.join(root, "synth", "test", f"{sid:06d}", "rgb", f"{iid:06d}.png"))
    return csv


def test_vis_poses_end_to_end_equals_the_mirror(tmp_path):
    from PIL import Image

    from raster_rgb_np import NumpyColorRenderer, compose
    from unopose_amd import bop_eval, vis_poses
    from unopose_amd.provider import SceneFiles
    from unopose_amd.render import HipColorRenderer

    root = str(tmp_path)
    csv = write_bop_folder(root)
    data = bop_eval.load_dataset(root, "synth", "test")
    W, H = data["im_size"]
    mirror, hip = NumpyColorRenderer(W, H), HipColorRenderer(W, H)
    for o, m in data["models"].items():
        for r in (mirror, hip):
            r.add_object(o, m["verts"], m["faces"], surf_color=vis_poses.palette(data["models"])[o])
    for results, out in ((None, str(tmp_path / "gt")), (csv, None)):
        assert vis_poses.main(["--data-dir", root, "--dataset", "synth", "--split", "test", "--ext", "png", "--no-text"] + (["--results", csv] if results else ["--out", out])) == 0
        out = out or os.path.join(os.path.dirname(csv), "vis")
        by_image = vis_poses.select_poses(data, None if results is None else bop_eval.read_results(csv), -1)
        assert len(by_image) == 3 and (results is None or sum(len(p) for p in by_image.values()) < len(bop_eval.read_results(csv)))
        for (sid, iid), poses_ in by_image.items():
            K = data["cameras"][sid][iid]
            k4 = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
            photo = SceneFiles().colour(os.path.join(root, "synth", "test"), sid, iid)
            want = None
            for ren in (mirror, hip):  # the mirror's renders, then the HIP renderer's toolkit interface, through the mirror's composition
                outs = [ren.render_object(p["obj_id"], p["R"], p["t"], *k4) for p in poses_]
                got = compose(np.stack([o["rgb"] for o in outs]), np.stack([o["depth"] for o in outs]), photo, data["depth_images"][sid][iid], True, 15.0)
                assert want is None or (np.array_equal(got[0], want[0]) and np.array_equal(got[3], want[3]))
                want = got
            rgb_path, diff_path = vis_poses.output_paths(out, "synth", "test", sid, iid, "png")
            assert np.array_equal(np.array(Image.open(rgb_path)), want[0]) and np.array_equal(np.array(Image.open(diff_path)), want[3]), (sid, iid)
            assert (want[0] != photo // 2).any() and want[3].any()
    # captions change pixels and nothing else fails; JPEG is written at the default
    files = vis_poses.vis_dataset(root, "synth", "test", scene_ids=[2], out_dir=str(tmp_path / "txt"))
    assert [os.path.relpath(f, str(tmp_path / "txt")) for f in files] == ["synth/test/000002/000000.jpg", "synth/test/000002/000000_depth_diff.jpg"]
    assert all(os.path.getsize(f) > 0 for f in files)
