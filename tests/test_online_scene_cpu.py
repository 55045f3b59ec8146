"""CPU: the scene stage of the online training pairs (unopose_amd/provider_online.py, part 4): the draw, the configuration, and the numpy
pixel rule `sense_views_host` -- its identity case, the background's geometry, the noise's statistics, and the distortion of dilated pairs
that the stage exists to remove."""
import json

import numpy as np
import pytest

import online_pairs_case as case
import scene_case
from unopose_amd import provider_online as P
from unopose_amd.provider import Window, lift_depth


def test_recipe_is_the_same_with_the_stage_on_or_off_and_the_scene_draw_is_pure():
    state = np.random.get_state()
    plain, staged = P.draw_recipe(5, 1, 9, 3, case.MODELS, case.CFG), P.draw_recipe(5, 1, 9, 3, case.MODELS, scene_case.CFG)
    assert set(plain) == set(staged) and all(np.array_equal(plain[k], staged[k]) and plain[k].dtype == staged[k].dtype for k in plain)
    a, b = P.draw_scene(5, 1, 9, 3, plain, case.MODELS, scene_case.CFG), P.draw_scene(5, 1, 9, 3, plain, case.MODELS, scene_case.CFG)
    after = np.random.get_state()
    assert all(np.array_equal(s, t) for s, t in zip(state, after) if isinstance(s, np.ndarray)) and state[2:] == after[2:]
    assert all(np.array_equal(a[k], b[k]) for k in a) and all(len(v) == 3 for v in a.values())
    for other in (P.draw_scene(5, 0, 9, 3, plain, case.MODELS, scene_case.CFG), P.draw_scene(5, 1, 10, 3, plain, case.MODELS, scene_case.CFG),
                  P.draw_scene(6, 1, 9, 3, plain, case.MODELS, scene_case.CFG), P.draw_scene(5, 1, 9, 3, plain, case.MODELS, scene_case.CFG, chunk=1)):
        assert not np.array_equal(a["keys"], other["keys"]) and not np.array_equal(a["n"], other["n"]) and not np.array_equal(a["tex_key"], other["tex_key"])
    assert np.array_equal(P.draw_scene(5, 1, 9, 2, plain, case.MODELS, scene_case.CFG)["p0"], a["p0"][:2])  # candidate k does not depend on their number
    assert P.SCENE_CHUNK0 > P.AUG_CHUNK >= P.online_cfg(scene_case.CFG)["max_chunks"]  # a stream no recipe or augmentation chunk uses
    with pytest.raises(ValueError):
        P.draw_scene(5, 1, 9, 3, plain, case.MODELS, case.CFG)  # the stage is not configured


def test_planes_follow_the_plane_rule():
    sc_cfg = P.online_cfg(scene_case.CFG)["scene"]
    r = P.draw_recipe(1, 0, 0, 40, case.MODELS, scene_case.CFG)
    s = P.draw_scene(1, 0, 0, 40, r, case.MODELS, scene_case.CFG)
    assert s["plane"].all() and s["keys"].dtype == np.uint64 and len(np.unique(s["keys"])) == 80
    for k in range(40):
        m = case.MODELS[int(r["obj"][k])]
        centre = r["R_q"][k] @ m["centre"] + r["t_q"][k]
        n, p0, u, v = s["n"][k], s["p0"][k], s["u"][k], s["v"][k]
        assert np.abs(np.cross(p0, centre)).max() < 1e-9 * np.dot(centre, centre)  # on the ray through the model centre
        gap = (p0[2] - centre[2]) / m["diameter"] - 0.5
        assert sc_cfg["plane_gap"][0] - 1e-12 <= gap <= sc_cfg["plane_gap"][1] + 1e-12
        frame = np.stack([u, v, n])
        assert np.abs(frame @ frame.T - np.eye(3)).max() < 1e-12  # unit normal, two in-plane unit axes
        assert n[2] < 0 and np.degrees(np.arccos(-n[2])) <= sc_cfg["plane_tilt"] + 1e-9
        assert s["cell"][k] == sc_cfg["texture_cell"] * m["diameter"]
    tilt = np.degrees(np.arccos(-s["n"][:, 2]))
    assert tilt.min() < 10 and tilt.max() > 25  # uniform in [0, 35]
    off = P.draw_scene(1, 0, 0, 4, r, case.MODELS, dict(case.CFG, online=dict(case.CFG["online"], scene=dict(background="none"))))
    assert not off["plane"].any() and np.array_equal(off["keys"], s["keys"][:4])  # drawn whatever the configuration says


def test_scene_keys_and_defaults():
    assert P.online_cfg(case.CFG)["scene"] is None and P.ONLINE_DEFAULTS["scene"] is None
    want = dict(background="plane", plane_gap=(0.0, 1.5), plane_tilt=35.0, texture_cell=0.25, noise=(0.0012, 0.0019, 0.4), baseline_m=0.075,
                disparity_steps=8, edge_thres=0.03, edge_drop=0.5, hole_prob=0.01, hole_cell=6)
    assert P.online_cfg(scene_case.CFG)["scene"] == want
    one = P.online_cfg(dict(case.CFG, online=dict(case.CFG["online"], scene=dict(plane_tilt=10.0))))["scene"]
    assert one == dict(want, plane_tilt=10.0)
    for bad in (dict(plane_tilts=10.0), dict(background="sky"), dict(hole_cell=0), dict(edge_drop=1.5), dict(plane_gap=(1.0, 0.5)), dict(noise=(0.1, 0.2)),
                dict(disparity_steps=-1), dict(plane_tilt=90.0)):
        with pytest.raises(ValueError):
            P.online_cfg(dict(case.CFG, online=dict(case.CFG["online"], scene=bad)))
    with pytest.raises(ValueError, match="unknown keys"):
        P.online_cfg(dict(case.CFG, online=dict(case.CFG["online"], scenes={})))


def test_fit_command_line_turns_the_stage_on(tmp_path, capsys):
    from unopose_amd import fit as F

    path = tmp_path / "cfg.json"
    path.write_text(json.dumps({"train": {}, "dataloader": {"train": {"dataset": {"cfg": {}}}}, "misc": {"output_dir": "/somewhere"}, "model": {}}))

    def plan(*argv):
        assert F.main(["--config", str(path), "--print-plan", *argv]) == 0
        return json.loads(capsys.readouterr().out)

    assert plan()["online_scene"] is False and plan("--online-scene")["online_scene"] is True
    assert plan("dataloader.train.online.scene.plane_tilt=20")["online_scene"] is True


def test_descriptors_are_range_checked():
    oc = P.online_cfg(scene_case.CFG)
    rows = P.scene_rows(scene_case.scene(), oc, "query")
    assert rows.shape == (len(case.NAMES), P.SCENE_DESC) and rows.dtype == np.uint64
    P.check_scene_rows(rows, case.H, case.W)
    P.check_scene_rows(P.scene_rows(scene_case.scene(), oc, "off"), case.H, case.W)
    for word, value in ((2, 2), (3, 2 ** 32 + 1), (5, 0), (6, 2 ** 20)):
        bad = rows.copy()
        bad[3, word] = value
        with pytest.raises(ValueError):
            P.check_scene_rows(bad, case.H, case.W)
    for word, value in ((26, 1e-9), (26, 0.0), (27, np.inf), (8, -1.0), (28, 0.0), (16, np.nan)):
        bad = rows.copy()
        bad.view(np.float64)[3, word] = value
        with pytest.raises(ValueError):
            P.check_scene_rows(bad, case.H, case.W)
    with pytest.raises(ValueError):
        P.check_scene_rows(rows[:, :-1], case.H, case.W)
    with pytest.raises(ValueError):
        P.sense_views_host(np.zeros((2, 4, 4), np.float32), np.zeros((2, 4, 4, 3), np.uint8), rows[:3])


def test_nothing_on_is_the_identity():
    depth, rgb, _ = scene_case.canvases()
    cfg = dict(case.CFG, online=dict(case.CFG["online"], scene=dict(background="none", noise=[0, 0, 0], disparity_steps=0, edge_drop=0, hole_prob=0)))
    oc = P.online_cfg(cfg)
    sc = P.draw_scene(7, 0, 3, len(case.NAMES), case.chunk()[1], case.MODELS, cfg)
    desc = np.concatenate([P.scene_rows(sc, oc, "query"), P.scene_rows(sc, oc, "reference")])
    out_d, out_c = P.sense_views_host(depth, rgb, desc)
    assert out_d.dtype == np.float32 and out_c.dtype == np.uint8 and np.array_equal(out_d.view(np.uint32), depth.view(np.uint32)) and np.array_equal(out_c, rgb)
    off = np.concatenate([P.scene_rows(scene_case.scene(), P.online_cfg(scene_case.CFG), "off")] * 2)
    out_d, out_c = P.sense_views_host(depth, rgb, off)
    assert np.array_equal(out_d.view(np.uint32), depth.view(np.uint32)) and np.array_equal(out_c, rgb)
    items, _ = P.items_from_views_host(*case.chunk(), cfg, with_intermediates=True, scene=sc)
    for mine, ref in zip(items, case.mirror()[0]):  # and so is the item rule with such a scene
        assert (mine is None) == (ref is None)
        if mine is not None:
            assert all(np.array_equal(np.asarray(mine[k]), np.asarray(ref[k])) for k in ref)


def test_background_lies_on_its_plane_behind_everything_else():
    """Before noise: the float64 depth of every background pixel, lifted along its ray, satisfies n . P = n . p0 to 1e-9 m; with everything
    but the plane off the stored depth is that value rounded once, and pixels with a render keep their bits."""
    depth, rgb, _ = scene_case.canvases()
    C = len(case.NAMES)
    oc = P.online_cfg(scene_case.CFG_QUIET)
    desc = P.scene_rows(scene_case.scene(), oc, "query")
    out_d, out_c, info = P.sense_views_host(depth[:C], rgb[:C], desc, with_intermediates=True)
    f, cx, cy = oc["focal"], case.W / 2.0, case.H / 2.0
    seen = 0
    for k, name in enumerate(case.NAMES):
        bg, z = info[k]["background"], info[k]["z"]
        assert not (bg & (depth[k] > 0)).any(), name
        assert np.array_equal(out_d[k][~bg].view(np.uint32), depth[k][~bg].view(np.uint32)) and np.array_equal(out_c[k][~bg], rgb[k][~bg]), name
        if not scene_case.scene()["plane"][k]:
            assert not bg.any() and name == scene_case.NO_PLANE
            continue
        n, p0 = scene_case.scene()["n"][k], scene_case.scene()["p0"][k] * 0.001
        ys, xs = np.nonzero(bg)
        pts = np.stack([(xs - cx) / f, (ys - cy) / f, np.ones(len(xs))], axis=1) * z[bg][:, None]
        err = np.abs(pts @ n - n @ p0).max()
        assert len(xs) > 100 and err < 1e-9 and z[bg].min() > 0 and z[bg].max() <= P.SCENE_Z_MAX_M, (name, err)
        assert np.array_equal(out_d[k][bg], (z[bg] * 1000.0).astype(np.float32)), name
        assert out_c[k][bg].std() > 10, name  # a texture, not a flat colour
        seen += 1
        if name == scene_case.STEEP:
            empty = ~bg & ~(depth[k] > 0)
            assert empty[:, 60:].all() and not empty[:, :40].any(), name  # the plane faces away from the rays on the right
        else:
            assert (bg | (depth[k] > 0)).all(), name
    assert seen == C - 1


def test_drop_outs_follow_their_rule():
    """Edge pixels are the pixels with a 4-neighbour inside the canvas that has no depth or a depth further than edge_thres z away; about
    edge_drop of them drop; holes come in whole cells; a dropped pixel keeps its colour."""
    depth, rgb, _ = scene_case.canvases()
    out_d, out_c, info = scene_case.sensed()
    sc = P.online_cfg(scene_case.CFG)["scene"]
    k = len(case.NAMES) + case.NAMES.index("plain")  # a reference: no background, an ellipse on nothing
    z, edge, dropped = info[k]["z"], info[k]["edge"], info[k]["dropped"]
    want = np.zeros_like(edge)
    for y in range(case.H):
        for x in range(case.W):
            if z[y, x] > 0:
                near = [z[yy, xx] for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)) if 0 <= yy < case.H and 0 <= xx < case.W]
                want[y, x] = any(not v > 0 or abs(z[y, x] - v) > sc["edge_thres"] * z[y, x] for v in near)
    assert np.array_equal(edge, want) and edge.sum() > 60
    assert np.array_equal(out_c[k], rgb[k]) and (out_d[k][dropped] == 0).all() and (out_d[k][(z > 0) & ~dropped] > 0).all()
    edges = np.concatenate([i["edge"].ravel() for i in info])
    drops = np.concatenate([i["dropped"].ravel() for i in info])
    share = drops[edges].mean()
    n = edges.sum()
    assert n > 2000 and abs(share - (sc["edge_drop"] + (1 - sc["edge_drop"]) * sc["hole_prob"])) < 5 * 0.5 / np.sqrt(n), (n, share)
    holes = 0
    for i in info:  # away from the edges a drop is a hole: all pixels with depth of its cell
        inner = i["dropped"] & ~i["edge"]
        for y, x in zip(*np.nonzero(inner)):
            cy, cx = y // sc["hole_cell"] * sc["hole_cell"], x // sc["hole_cell"] * sc["hole_cell"]
            cell = (slice(cy, cy + sc["hole_cell"]), slice(cx, cx + sc["hole_cell"]))
            assert i["dropped"][cell][i["z"][cell] > 0].all()
        holes += inner.any()
    assert holes >= 5  # of 28 views with 120 cells each at 0.01


@pytest.mark.parametrize("z_mm", (350.0, 1500.0))
def test_noise_has_unit_variance_and_stays_inside_its_bound(z_mm):
    """Constant depth, quantisation and drop-outs off: (z_out - z) / sigma(z) over 62 500 pixels has a sample standard deviation of 1 within
    5 standard errors 5 / sqrt(2 N) = 0.0141, a mean of 0 within 5 / sqrt(N), and no sample beyond 2 sqrt(3)."""
    cfg = dict(case.CFG, online=dict(case.CFG["online"], canvas=(250, 250), scene=dict(background="none", disparity_steps=0, edge_drop=0, hole_prob=0)))
    oc = P.online_cfg(cfg)
    _, recipe = case.chunk()
    desc = P.scene_rows(P.draw_scene(3, 0, int(z_mm), 1, recipe, case.MODELS, cfg), oc, "reference")  # another view key per depth
    depth = np.full((1, 250, 250), z_mm, np.float32)
    out, _ = P.sense_views_host(depth, np.zeros((1, 250, 250, 3), np.uint8), desc)
    a, b, z0 = oc["scene"]["noise"]
    z = z_mm * 0.001
    unit = (out[0].astype(np.float64) * 0.001 - z).ravel() / (a + b * (z - z0) ** 2)
    n = unit.size
    print("z %.3f m: std %.5f, mean %.5f, max |g| %.4f over %d" % (z, unit.std(ddof=1), unit.mean(), np.abs(unit).max(), n))
    assert n >= 60000 and abs(unit.std(ddof=1) - 1) < 5 / np.sqrt(2 * n) and abs(unit.mean()) < 5 / np.sqrt(n)
    assert np.abs(unit).max() <= 2 * np.sqrt(3.0)
    assert np.abs(unit).max() > 2.5  # a bell, not a narrow band


def test_quantisation_lands_on_disparity_steps():
    cfg = dict(case.CFG, online=dict(case.CFG["online"], scene=dict(background="none", noise=[0, 0, 0], edge_drop=0, hole_prob=0)))
    oc = P.online_cfg(cfg)
    _, recipe = case.chunk()
    desc = P.scene_rows(P.draw_scene(3, 0, 0, 1, recipe, case.MODELS, cfg), oc, "reference")
    depth = np.linspace(150.0, 2500.0, case.H * case.W).astype(np.float32).reshape(1, case.H, case.W)
    out, _ = P.sense_views_host(depth, np.zeros((1, case.H, case.W, 3), np.uint8), desc)
    fb, steps = oc["focal"] * oc["scene"]["baseline_m"], oc["scene"]["disparity_steps"]
    disparity = fb / (out[0].astype(np.float64) * 0.001) * steps
    assert np.abs(disparity - np.rint(disparity)).max() < 1e-4  # float32 storage
    z = depth[0].astype(np.float64) * 0.001
    assert (np.abs(out[0].astype(np.float64) * 0.001 - z) <= z * z / (steps * fb)).all() and (out[0] != depth[0]).mean() > 0.9
    far = np.full((1, case.H, case.W), 2.0e5, np.float32)  # 200 m: less than one step of disparity
    assert not P.sense_views_host(far, np.zeros((1, case.H, case.W, 3), np.uint8), desc)[0].any()


@pytest.mark.parametrize("name", ("dilate_plain", "dilate_edge_occluder"))
def test_a_plane_behind_the_object_removes_the_centroids_pull(name):
    """The distortion the stage starts from.  Without a background the rim of the dilated mask has depth 0: the centroid of `dilate_plain`
    comes out at z = 0.302 m for an object at 0.41 m, and 26 of its 1501 visible pixels are discarded.  With a fronto-parallel plane 40 mm
    behind the object's farthest visible pixel (noise and drop-outs off) every visible object pixel is kept and the centroid's z lies within
    0.02 m of the mean z of the visible object pixels.  (For `dilate_edge_occluder` the rim also takes in occluder pixels at 0.3 m; they
    pull less than the bound allows, so the plane stays where the issue put it.)"""
    k = case.NAMES.index(name)
    vis, qd = scene_case.visible_object(name)
    object_z = qd[vis].astype(np.float64).mean() * 0.001
    before = case.mirror()[1][k]
    items, info = scene_case.mirror(quiet=True)
    after = info[k]
    K = P.camera_matrix(P.online_cfg(scene_case.CFG_QUIET))

    def kept_visible(i):  # the visible object pixels inside the keep sphere
        win = Window.from_extents((case.H, case.W), *i["q_row"][3:7])
        d = lift_depth(i["scene_depth"].astype(np.float64) * 0.001, K, win)[win.crop(vis)] - i["q_mean"]
        return int((np.sqrt((d * d).sum(axis=1)) < 1.2 * i["radius"]).sum())

    print(name, "object z %.4f, %d visible; centroid z before %.4f (%d visible kept), after %.4f (%d visible kept)" % (
        object_z, vis.sum(), before["q_mean"][2], kept_visible(before), after["q_mean"][2], kept_visible(after)))
    assert abs(before["q_mean"][2] - object_z) > 0.07  # today
    if name == "dilate_plain":
        assert kept_visible(before) == vis.sum() - 26
    assert items[k] is not None and np.array_equal(after["q_mask"], before["q_mask"]) and np.array_equal(after["q_row"], before["q_row"])
    assert (after["scene_depth"][after["q_mask"]] > 0).all()  # the rim has a depth now
    assert abs(after["q_mean"][2] - object_z) < 0.02
    assert kept_visible(after) == vis.sum() and after["q_kept"] >= vis.sum()
