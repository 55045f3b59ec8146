"""CPU: the view sampler against bop_toolkit's own views (tests/golden/render_train_views.npz, written by
tests/golden/make_render_train_golden.py), the scene files' text against the toolkit's, the model reader, the host form of the shaded
rasteriser against the mirror it shares its visibility and flat shading with, and `render_train --host` on a synthetic dataset folder."""
import functools
import os
import os.path as osp

import numpy as np
import pytest

GOLDEN = osp.join(osp.dirname(osp.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(osp.join(GOLDEN, "render_train_views.npz")) as z:
        return {k: z[k] for k in z.files}


def sampled(name):
    from unopose_amd.view_sampler import sample_views

    z = fixture()
    a = z[name + "_args"]
    views, levels = sample_views(int(a[0]), a[1], (a[2], a[3]), (a[4], a[5]), str(z[name + "_mode"]))
    return views, levels, a[1]


CASES = ("hinter12", "hinter42", "hinter162", "fib9", "fib10", "hinter162_upper", "fib9_upper", "hinter42_on_samples")


def test_fixture_holds_every_case():
    assert sorted(fixture()["names"].tolist()) == sorted(CASES)


@pytest.mark.parametrize("name", CASES)
def test_sample_views_reproduces_the_toolkit(name):
    """Count, order and levels exactly; R and t / radius within 1e-9 (float64, a dozen operations per value: a real difference -- another
    order, another look-at frame -- is larger by orders of magnitude)."""
    z = fixture()
    views, levels, radius = sampled(name)
    want_R, want_t = z[name + "_R"], z[name + "_t"]
    assert len(views) == len(want_R)
    assert [int(v) for v in levels] == z[name + "_levels"].tolist()
    R = np.array([v["R"] for v in views]).reshape(-1, 3, 3)
    t = np.array([v["t"] for v in views]).reshape(-1, 3)
    assert all(v["R"].shape == (3, 3) and v["t"].shape == (3, 1) for v in views)
    assert np.abs(R - want_R).max() <= 1e-9 and np.abs(t - want_t).max() * (1.0 / radius) <= 1e-9


def test_counts_and_the_closed_interval():
    assert [len(sampled(k)[0]) for k in ("hinter12", "hinter42", "hinter162", "fib9", "fib10")] == [12, 42, 162, 9, 11]  # even n: the next odd
    views, levels, _ = sampled("hinter162_upper")
    assert len(levels) == 162 > len(views) == 89  # the level list is the whole sphere's
    # the bounds of this case are angles of sampled points: an open interval would lose views
    z = fixture()
    a = z["hinter42_on_samples_args"]
    from unopose_amd.view_sampler import sample_views

    shrunk = sample_views(42, a[1], (np.nextafter(a[2], 7.0), np.nextafter(a[3], 0.0)), (np.nextafter(a[4], 2.0), np.nextafter(a[5], -2.0)))[0]
    assert len(shrunk) < len(sampled("hinter42_on_samples")[0]) == 30
    with pytest.raises(ValueError):
        sample_views(12, mode="spiral")


@pytest.mark.parametrize("name", ["hinter42", "hinter162"])
def test_pole_views_take_the_side_fallback(name):
    """A camera on the z axis looks along -z or +z: forward x up vanishes and the side vector is (1, 0, 0), the first row of R."""
    z = fixture()
    views, _, radius = sampled(name)
    poles = z[name + "_poles"].tolist()
    assert len(poles) == 2
    for i in poles:
        R, t = views[i]["R"], views[i]["t"].reshape(3)
        assert np.array_equal(R[0], [1.0, 0.0, 0.0]) and abs(abs(R[2, 2]) - 1.0) < 1e-12
        assert np.abs(R - z[name + "_R"][i]).max() <= 1e-9 and np.abs(t - [0.0, 0.0, radius]).max() / radius < 1e-9
    assert {float(np.sign(views[i]["R"][2, 2])) for i in poles} == {-1.0, 1.0}


def test_scene_files_equal_the_toolkits_text(tmp_path):
    """The first three views of the 42-point sphere through `render_train.object_files`' dictionaries and the writer gt_info uses."""
    from unopose_amd import render_train as rt
    from unopose_amd.view_sampler import sample_views

    z = fixture()
    depth_scale, obj_id, radius = z["json_args"].tolist()
    views, levels = sample_views(42, radius)
    Rs, ts = np.array([v["R"] for v in views[:3]]), np.array([v["t"].reshape(3) for v in views[:3]])
    cam = dict(K=z["json_K"], depth_scale=depth_scale, im_size=(4, 3))

    class Blank:
        def render_batch(self, obj_id, Rs, ts, k4):
            return np.zeros((len(Rs), 3, 4, 3), np.uint8) if self.rgb else np.zeros((len(Rs), 3, 4), np.float32)

    rgb, depth = Blank(), Blank()
    rgb.rgb, depth.rgb = True, False
    files = dict(rt.object_files(int(obj_id), Rs, ts, [int(v) for v in levels[:3]], cam, rgb, depth))
    for name in ("scene_camera.json", "scene_gt.json"):
        got = rt._json_bytes(files[name], str(tmp_path / name))
        assert got == open(osp.join(GOLDEN, "render_train_" + name), "rb").read(), name
    assert sorted(files) == sorted([f"{d}/{i:06d}.png" for d in ("rgb", "depth") for i in range(3)] + ["scene_camera.json", "scene_gt.json"])


# ---- the model reader ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binary", [True, False])
@pytest.mark.parametrize("with_normals,with_colors,with_uv", [(True, True, True), (False, False, False), (True, False, True), (False, True, False)])
def test_read_ply_model_round_trip(tmp_path, binary, with_normals, with_colors, with_uv):
    from gt_info_case import make_models
    from render_train_case import analytic_normals, sphere_uv, write_model_ply
    from unopose_amd.bop_eval import read_ply, read_ply_colors, read_ply_model, vertex_normals

    m = make_models()[2]
    v, f = m["verts"], m["faces"]
    normals = analytic_normals(v, (75.0, 105.0, 85.0)) if with_normals else None
    cols = np.random.RandomState(1).randint(0, 256, size=(len(v), 3)) if with_colors else None
    uv = sphere_uv(v) if with_uv else None
    path = str(tmp_path / "m.ply")
    write_model_ply(path, v, f, normals=normals, colors=cols, uv=uv, texture_file="tex_1.png" if with_uv else None, binary=binary)
    got = read_ply_model(path)
    as32 = lambda a: np.asarray(a, np.float32).astype(np.float64)  # noqa: E731
    assert np.array_equal(got["pts"], as32(v)) and np.array_equal(got["faces"], f) and got["faces"].dtype == np.int32
    assert got["normals_computed"] == (not with_normals)
    if with_normals:
        assert np.array_equal(got["normals"], as32(normals))
    else:
        assert np.array_equal(got["normals"], vertex_normals(as32(v), f))
    assert (got["colors"] is None) if not with_colors else np.array_equal(got["colors"], cols / 255.0)
    assert (got["texture_uv"] is None) if not with_uv else np.array_equal(got["texture_uv"], as32(uv))
    assert got["texture_file"] == ("tex_1.png" if with_uv else None)
    # the two older readers see the same file as before
    assert np.array_equal(read_ply(path)["pts"], got["pts"]) and sorted(read_ply(path)) == ["faces", "pts"]
    assert sorted(read_ply_colors(path)) == ["colors", "faces", "pts"]


@pytest.mark.parametrize("binary", [True, False])
def test_read_ply_model_rejects_per_face_texture_coordinates(tmp_path, binary):
    from gt_info_case import make_models
    from render_train_case import write_model_ply
    from unopose_amd.bop_eval import read_ply_model

    m = make_models()[1]
    path = str(tmp_path / "m.ply")
    write_model_ply(path, m["verts"], m["faces"], binary=binary, face_texcoord=True)
    with pytest.raises(ValueError, match="texture coordinates per face"):
        read_ply_model(path)


def test_vertex_normals_on_a_sphere_and_a_cube():
    """Unit length everywhere.  Cube (12 triangles): a corner's normal is the sum of its three faces' axis normals, each weighted by the
    area of that face's triangles at the corner (one: 1/2, both: 1) -- computed here from the triangulation, exact up to rounding.  Sphere
    (the 42-vertex icosphere): the radial direction; the triangles around a vertex differ in area by under a quarter and tilt against the
    radius by about half an edge's angle (0.55 / 2 rad), so the weighted sum leaves the radius by less than 0.25 * 0.28 = 0.07 rad; at the
    twelve 5-fold vertices the ring is symmetric and the normal is radial to rounding.  (Measured: under 1e-4 rad at every vertex.)"""
    from bop_eval_case import icosphere
    from unopose_amd.bop_eval import vertex_normals

    corners = np.array([[x, y, z] for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (-1.0, 1.0)]) * [30.0, 30.0, 30.0]
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]  # outward winding
    faces = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))])
    n = vertex_normals(corners, faces)
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 1e-12
    want = np.zeros((8, 3))
    for tri in faces:
        axis = np.cross(corners[tri[1]] - corners[tri[0]], corners[tri[2]] - corners[tri[0]])
        axis = axis / np.linalg.norm(axis)
        assert np.abs(axis).max() == 1.0 and np.allclose(axis @ corners[tri[0]], 30.0)  # an axis normal, outward
        want[tri] += 0.5 * axis
    assert len(set(np.abs(want).sum(axis=1).tolist())) > 1  # corners with three, four and five triangles
    want /= np.linalg.norm(want, axis=1, keepdims=True)
    assert np.abs(n - want).max() < 1e-12
    assert len({tuple(np.round(np.abs(r), 6)) for r in n}) > 1  # not all corners are the diagonal: the weights matter

    v, f = icosphere()
    n = vertex_normals(v * 50.0, f)
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 1e-12
    angle = np.arccos(np.clip((n * v).sum(axis=1), -1, 1))
    print("largest angle to the radius: %.4f rad" % angle.max())
    assert angle.max() < 0.07 and angle[:12].max() < 1e-7
    lone = vertex_normals(np.concatenate([v, [[9.0, 9.0, 9.0]]]), f)
    assert np.array_equal(lone[-1], [0.0, 0.0, 0.0])  # no face: the zero vector, which the shader reads as "ambient only"


# ---- the host rasteriser -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("colour", ["colors", "surf"])
def test_host_flat_1x_equals_the_colour_mirror_and_the_depth_mirror(colour):
    from raster_np import render_depth as depth_mirror
    from raster_shade_np import flat_reference, render_shaded
    from render_train_case import SURF, colour_kwargs, views
    from unopose_amd.shade_host import render_depth

    W, H = 37, 29
    kw = colour_kwargs(colour)
    k4, Rs, ts = views(W, H)
    for R, t in zip(Rs, ts):
        want = flat_reference(kw["verts"], kw["faces"], R, t, k4, H, W, colors=kw.get("colors"), surf_color=SURF)
        got = render_shaded(R=R, t=t, fx=k4[0], fy=k4[1], cx=k4[2], cy=k4[3], H=H, W=W, shading="flat", ssaa=1, **kw)
        assert np.array_equal(got, want) and (got > 0).sum() > 50
        assert np.array_equal(render_depth(kw["verts"], kw["faces"], R, t, *k4, H, W), depth_mirror(kw["verts"], kw["faces"], R, t, *k4, H, W))


def test_host_shading_rules():
    """Phong on the tricky model: the coplanar duplicates lose to the originals, a zero normal leaves the ambient term, texture coordinates on
    and beyond the edges stay inside the texture, supersampling is the mean of the sample bytes."""
    from raster_shade_np import render_shaded
    from render_train_case import colour_kwargs, tricky_model, views

    W, H = 40, 32
    k4, Rs, ts = views(W, H)
    common = dict(R=Rs[0], t=ts[0], fx=k4[0], fy=k4[1], cx=k4[2], cy=k4[3], H=H, W=W)
    m = tricky_model()
    rgb = render_shaded(ssaa=1, **common, **colour_kwargs("colors"))
    drawn = (rgb > 0).any(axis=2)
    assert drawn.sum() > 250 and not ((rgb[..., 2] > 0) & (rgb[..., 0] == 0) & (rgb[..., 1] == 0)).any()  # no pure blue: the duplicates lost
    tex = render_shaded(ssaa=1, ambient=1.0, **common, **colour_kwargs("texture"))  # full ambient: weight 1, a lit pixel IS its texel
    texels = {tuple(c) for c in m["texture"].reshape(-1, 3).tolist()}
    lit = tex[(tex > 0).any(axis=2)]
    assert len(lit) == drawn.sum() and {tuple(c) for c in lit.tolist()} <= texels and len({tuple(c) for c in lit.tolist()}) > 15
    for s in (2, 3, 4):
        img = render_shaded(ssaa=s, samples=True, **common, **colour_kwargs("colors"))
        small = render_shaded(ssaa=s, **common, **colour_kwargs("colors"))
        mean = img.reshape(H, s, W, s, 3).astype(np.float64).sum(axis=(1, 3)) / (s * s)
        assert np.abs(small - mean).max() <= 0.5 + 1e-6 and 0 < (small > 0).any(axis=2).sum()
    amb = dict(colour_kwargs("surf"), normals=np.zeros_like(m["normals"]))
    only = render_shaded(ssaa=1, ambient=0.25, **common, **amb)
    assert set(np.unique(only[..., 0]).tolist()) == {0, int(np.float32(0.25) * np.float32(0.95) * np.float32(255) + np.float32(0.5))}


# ---- the tool ------------------------------------------------------------------------------------------------------------------------
def test_render_train_host_writes_checks_and_refuses(tmp_path, capsys):
    from PIL import Image

    from render_train_case import CAMERA, RENDER_ARGS, write_dataset
    from unopose_amd import render_train as rt
    from unopose_amd.provider import load_json

    write_dataset(str(tmp_path))
    args = ["--data-dir", str(tmp_path), "--dataset", "synth", "--host"] + RENDER_ARGS
    assert rt.main(args) == 0
    out = tmp_path / "synth" / "train_render"
    assert sorted(os.listdir(out)) == ["000001", "000002"]
    for obj_id in (1, 2):
        folder = out / f"{obj_id:06d}"
        assert sorted(os.listdir(folder)) == ["depth", "rgb", "scene_camera.json", "scene_gt.json"]
        names = [f"{i:06d}.png" for i in range(12)]
        assert sorted(os.listdir(folder / "rgb")) == names and sorted(os.listdir(folder / "depth")) == names
        cam, gt = load_json(str(folder / "scene_camera.json")), load_json(str(folder / "scene_gt.json"))
        assert sorted(cam, key=int) == [str(i) for i in range(12)] == sorted(gt, key=int)
        assert cam["3"]["depth_scale"] == CAMERA["depth_scale"] and cam["3"]["view_level"] == 0 and cam["3"]["cam_K"][0] == CAMERA["fx"]
        assert gt["3"][0]["obj_id"] == obj_id and len(gt["3"][0]["cam_R_m2c"]) == 9 and len(gt["3"][0]["cam_t_m2c"]) == 3
        rgb, depth = np.asarray(Image.open(folder / "rgb" / "000003.png")), np.asarray(Image.open(folder / "depth" / "000003.png"))
        assert rgb.shape == (32, 40, 3) and rgb.dtype == np.uint8 and depth.shape == (32, 40) and depth.dtype.itemsize >= 2
        seen = depth > 0
        assert 150 < seen.sum() < 800 and abs(float(depth[seen].min()) * CAMERA["depth_scale"] - 330.0) < 25.0  # 420 mm minus about 90 mm of object
        assert ((rgb > 0).any(axis=2) & ~seen).sum() < seen.sum() // 3 and (rgb > 0).any(axis=2)[seen].mean() > 0.9  # rgb is smoothed at the rim
    one = np.asarray(Image.open(out / "000001" / "rgb" / "000000.png")).reshape(-1, 3)
    assert len(np.unique(one, axis=0)) > 12  # textured and shaded
    capsys.readouterr()
    assert rt.main(args + ["--check"]) == 0
    assert rt.main(args) == 2 and "exist" in capsys.readouterr().err  # refuses without --force
    victim = out / "000002" / "rgb" / "000007.png"
    data = bytearray(victim.read_bytes())
    data[len(data) // 2] ^= 0x01
    victim.write_bytes(bytes(data))
    assert rt.main(args + ["--check"]) == 1
    assert "000007.png: differs" in capsys.readouterr().out and victim.read_bytes() == bytes(data)  # nothing was written
    assert rt.main(args + ["--force"]) == 0 and rt.main(args + ["--check"]) == 0
    (out / "000001" / "depth" / "000099.png").write_bytes(b"x")
    assert rt.main(args + ["--check"]) == 1 and "not a file of this render" in capsys.readouterr().out
