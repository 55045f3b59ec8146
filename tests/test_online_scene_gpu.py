"""GPU: the scene stage of the online training pairs on the device (csrc/scene.hip through ops.sense_views and OnlinePairs) against the numpy
rule `provider_online.sense_views_host` -- equal in every depth bit and colour byte, since the rule fixes every operation -- on the hand-made
canvases of online_pairs_case and on real renders; the sensed points against the mesh itself; and `fit --online-scene`."""
import json
import os

import numpy as np
import pytest
import torch

import online_pairs_case as case
import scene_case

pytestmark = pytest.mark.gpu

KEYS = ("pts", "rgb", "rgb_choose", "translation_label", "rotation_label", "tem1_rgb", "tem1_choose", "tem1_pts", "K")


@pytest.fixture(scope="module")
def models_dir(tmp_path_factory):
    import render_train_case

    return os.path.join(render_train_case.write_dataset(str(tmp_path_factory.mktemp("scene"))), "models")


def _source(models_dir, **kw):
    from unopose_amd.provider_online import OnlinePairs

    cfg = dict(kw.pop("base", scene_case.CFG), **kw.pop("cfg", {}))
    return OnlinePairs(models_dir, cfg, "cuda", kw.pop("seed", 5), **kw)


def test_sense_views_equals_the_host_rule_on_all_views_of_the_hand_chunk():
    """28 views of 56 x 72 (W no multiple of 64, 56 no multiple of the hole cell) in one launch: the 14 composed queries with their planes (one
    steep enough to leave part of the canvas empty, one all-zero view without a plane, objects touching every border), then the 14 references."""
    from unopose_amd import ops

    depth, rgb, desc = scene_case.canvases()
    want_d, want_c, info = scene_case.sensed()
    C = len(case.NAMES)
    steep, bare = info[case.NAMES.index(scene_case.STEEP)], case.NAMES.index(scene_case.NO_PLANE)
    assert steep["background"].any() and (~steep["background"] & ~(steep["z"] > 0)).any()  # the cases are what they say
    assert not depth[bare].any() and not want_d[bare].any() and np.array_equal(want_c[bare], rgb[bare])
    touched = np.stack([i["z"] > 0 for i in info[C:]])
    assert touched[:, 0].any() and touched[:, -1].any() and touched[:, :, 0].any() and touched[:, :, -1].any()
    assert sum(i["dropped"].sum() for i in info) > 500 and sum((i["dropped"] & ~i["edge"]).sum() for i in info) > 50
    got_d, got_c = ops.sense_views(torch.tensor(depth, device="cuda"), torch.tensor(rgb, device="cuda"), desc)
    assert got_d.dtype == torch.float32 and got_c.dtype == torch.uint8 and got_d.shape == depth.shape and got_c.shape == rgb.shape
    got_d, got_c = got_d.cpu().numpy(), got_c.cpu().numpy()
    for v in range(2 * C):
        name = ("query " if v < C else "reference ") + case.NAMES[v % C]
        bad = np.flatnonzero(got_d[v].view(np.uint32) != want_d[v].view(np.uint32))
        assert len(bad) == 0, (name, len(bad), got_d[v].ravel()[bad[:4]], want_d[v].ravel()[bad[:4]])
        assert np.array_equal(got_c[v], want_c[v]), name
    assert (want_d != depth).mean() > 0.3 and (want_c != rgb).mean() > 0.2  # the stage did something


def test_pass_through_rows_and_bad_arguments():
    from unopose_amd import ops
    from unopose_amd.provider_online import online_cfg, scene_rows

    depth, rgb, desc = scene_case.canvases()
    d, c = torch.tensor(depth, device="cuda"), torch.tensor(rgb, device="cuda")
    off = np.concatenate([scene_rows(scene_case.scene(), online_cfg(scene_case.CFG), "off")] * 2)
    got_d, got_c = ops.sense_views(d, c, off)
    assert torch.equal(got_d.view(torch.int32), d.view(torch.int32)) and torch.equal(got_c, c) and got_d.data_ptr() != d.data_ptr()
    with pytest.raises(ValueError):
        ops.sense_views(d, c, desc[:5])
    bad = desc.copy()
    bad[0, 5] = 0  # a hole cell of 0 pixels
    with pytest.raises(ValueError):
        ops.sense_views(d, c, bad)
    with pytest.raises(RuntimeError):
        ops.sense_views(d.cpu(), c, desc)
    with pytest.raises(RuntimeError):
        ops.sense_views(d, c[:, :, :, :2], desc)


@pytest.fixture(scope="module")
def hand(models_dir):
    """The hand-made chunk through the device route with the scene -> (source, chunk result, taken list)."""
    views, recipe = case.chunk()
    src = _source(models_dir, augment=False)
    up = lambda *names: torch.from_numpy(np.concatenate([views[n] for n in names])).cuda()  # noqa: E731
    res = src.chunk_device(recipe, (up("q_rgb", "ref_rgb"), up("q_depth", "ref_depth"), up("occ_rgb"), up("occ_depth")), scene=scene_case.scene())
    taken = [(recipe, res, int(k)) for k in np.flatnonzero(res["valid"])]
    return src, res, taken


def test_chunk_with_a_scene_equals_the_host_rule(hand):
    """Everything tests/test_online_pairs_gpu.py compares without the stage, with it: tables, masks, scene canvases, windows, counts, radius,
    points, indices, labels, the atlas and the finished crops."""
    from unopose_amd import ops
    from unopose_amd.provider_online import finish_item
    from unopose_amd.provider_train import AugPlan, collate_pairs_device

    src, res, taken = hand
    items, info = scene_case.mirror()
    _, plain = case.mirror()
    _, recipe = case.chunk()
    C = len(case.NAMES)
    mask, depth, rgb = res["mask"].cpu().numpy(), res["scene_depth"].cpu().numpy(), res["scene_rgb"].cpu().numpy()
    ref_d = scene_case.sensed()[0][C:]
    assert [bool(v) for v in res["valid"]] == [it is not None for it in items] and sum(it is not None for it in items) >= 6
    radius = res["radius"].cpu().numpy()
    for k, name in enumerate(case.NAMES):
        assert np.array_equal(res["table"][k], info[k]["q_row"]) and np.array_equal(res["table"][C + k], info[k]["ref_row"]), name
        assert np.array_equal(res["table"][k], plain[k]["q_row"]), name  # the query's mask and table stay the renders' own
        assert np.array_equal(mask[k] != 0, info[k]["q_mask"]) and np.array_equal(mask[C + k] != 0, info[k]["ref_mask"]), name
        assert np.array_equal(depth[k].view(np.uint32), info[k]["scene_depth"].view(np.uint32)) and np.array_equal(rgb[k], info[k]["scene_rgb"]), name
        assert np.array_equal(depth[C + k].view(np.uint32), ref_d[k].view(np.uint32)), name  # sensed before the item rule read it
        if "q_window" not in info[k]:
            continue
        q, r = res["q_win"][k], res["r_win"][k]
        assert q.as_list() == info[k]["q_window"] and r.as_list() == info[k]["ref_window"], name
        assert np.array_equal(res["q_rows"][k][:q.side], info[k]["q_rows"]) and np.array_equal(res["r_rows"][k][:r.side], info[k]["ref_rows"]), name
        assert list(res["q_counts"][k]) == [info[k]["q_set"], info[k]["q_kept"]] and list(res["r_counts"][k]) == [info[k]["ref_set"]] * 2, name
        assert radius[k] == info[k]["radius"], name
    for _, _, k in taken:
        for key in ("pts", "rgb_choose", "tem1_pts", "tem1_choose"):
            got = res[key][k].cpu()
            assert got.dtype == items[k][key].dtype and torch.equal(got, items[k][key]), (case.NAMES[k], key)
        lab = src._labels(recipe, [k])
        for key in ("translation_label", "rotation_label", "K"):
            assert torch.equal(lab[key][0].cpu(), items[k][key]), (case.NAMES[k], key)
    want = collate_pairs_device([dict(items[k], rgb_plan=AugPlan(), tem1_plan=AugPlan()) for _, _, k in taken], case.S, True)
    got = src.collate_device(3, taken)
    assert set(got) == set(want)
    for key in want:
        assert got[key].dtype == want[key].dtype and torch.equal(got[key].cpu(), want[key]), key
    done = ops.finish_crops(got, "cuda")
    for n, (_, _, k) in enumerate(taken):
        ref = finish_item(items[k], case.S)
        for key in KEYS:
            assert done[key].dtype == ref[key].dtype and torch.equal(done[key][n].cpu(), ref[key]), (case.NAMES[k], key)


def _equal(a, b):
    return tuple(a) == tuple(b) == KEYS and all(a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]) for k in KEYS)


def test_source_with_a_scene_on_real_renders(models_dir):
    dev, host, again = _source(models_dir), _source(models_dir, host=True), _source(models_dir)
    batches = [dev.batch(i) for i in range(3)]
    assert _equal(batches[2], host.batch(2)) and _equal(batches[0], host.batch(0))  # host=False and host=True
    assert _equal(batches[2], again.batch(2)) and _equal(batches[1], dev.batch(1))  # a pure function of (seed, rank, iteration)
    assert not _equal(batches[2], _source(models_dir, rank=1).batch(2)) and not _equal(batches[2], _source(models_dir, seed=6).batch(2))
    assert not torch.equal(batches[0]["pts"], batches[1]["pts"]) and float(batches[2]["rgb"].std()) > 0.1
    off = _source(models_dir, base=case.CFG).batch(2)
    assert not torch.equal(batches[2]["pts"], off["pts"]) and not torch.equal(batches[2]["rgb"], off["rgb"])  # the crops show the background


def test_batch_labels_equal_the_scene_off_batch_and_its_points_differ(models_dir):
    """A batch is the first valid candidates of a recipe the stage does not touch, so its labels are the scene-off batch's whenever the stage
    leaves the valid candidates the same.  Without the dilation it does at these sizes: the queries' masks and tables are the renders' own,
    every mask pixel has a depth on both routes, and a few drop-outs among some hundred window pixels leave the kept points far above 32."""
    cfg = dict(dilate_mask=False)
    on, off = _source(models_dir, cfg=cfg), _source(models_dir, base=case.CFG, cfg=cfg)
    for i in range(3):
        a, b = on.batch(i), off.batch(i)
        for key in ("translation_label", "rotation_label", "K"):
            assert torch.equal(a[key], b[key]), (i, key)
        assert not torch.equal(a["pts"], b["pts"]) and not torch.equal(a["tem1_pts"], b["tem1_pts"]), i


def test_labels_equal_the_scene_off_labels_candidate_by_candidate(models_dir):
    """Poses, labels, coins and keys of a chunk's candidates are the same arrays with the stage on or off, and so are the labels the source
    hands out for every candidate valid on both routes."""
    from unopose_amd.provider_online import draw_recipe, draw_scene

    on, off = _source(models_dir, augment=False), _source(models_dir, base=case.CFG, augment=False)
    a, b = draw_recipe(5, 0, 1, 4, on.models, on.cfg), draw_recipe(5, 0, 1, 4, off.models, off.cfg)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    canv = on.render_chunk(a)
    with_scene = on.chunk_device(a, canv, scene=draw_scene(5, 0, 1, 4, a, on.models, on.cfg))
    without = off.chunk_device(b, canv)
    both = np.flatnonzero(with_scene["valid"] & without["valid"])
    assert len(both) >= 2
    assert np.array_equal(with_scene["table"][:4], without["table"][:4])  # the queries' masks are the renders' own
    for k in both:
        assert all(torch.equal(on._labels(a, [k])[key], off._labels(b, [k])[key]) for key in ("translation_label", "rotation_label", "K"))
        assert not torch.equal(with_scene["pts"][k], without["pts"][k])


def test_sensed_points_lie_within_the_sensors_error_of_the_mesh(tmp_path):
    """Independent of the mirror: the icosphere of tests/test_online_pairs_gpu.py with noise and quantisation on, drop-outs off, no background,
    no dilation.  Every query point lies within [inscribed - e, r + e] of the pose's translation, with e derived from the rule: the noise is
    at most 2 sqrt(3) sigma(z) and the quantisation moves z by at most z^2 / (steps fb) (half a step of disparity moves it by half that; the
    other half covers the ray's slant |r| <= 1.12 at these poses and the second-order term), at z_max = the farthest the sphere reaches."""
    from bop_eval_case import icosphere
    from render_train_case import write_model_ply
    from unopose_amd.provider_online import draw_recipe, draw_scene, online_cfg

    r = 40.0
    v, f = icosphere()
    write_model_ply(str(tmp_path / "obj_000001.ply"), v * r, f, normals=v)
    tri = v[f] * r
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    inscribed = np.abs((tri[:, 0] * n).sum(axis=1) / np.linalg.norm(n, axis=1)).min()
    cfg = dict(shift_range=0.0, online=dict(case.CFG["online"], occluder_prob=0.0, offset=0.2, scene=dict(background="none", edge_drop=0.0, hole_prob=0.0)))
    src = _source(str(tmp_path), cfg=cfg, augment=False)
    recipe = draw_recipe(3, 0, 0, 4, src.models, src.cfg)
    recipe["noise"][:] = 0.0
    recipe["dilate"][:] = False
    assert not recipe["occ"].any() and not recipe["shift"].any()
    canv = src.render_chunk(recipe)
    res = src.chunk_device(recipe, canv, scene=draw_scene(3, 0, 0, 4, recipe, src.models, src.cfg))
    clean = src.chunk_device(recipe, canv)
    assert res["valid"].all()
    sc = online_cfg(src.cfg)["scene"]
    a, b, z0 = sc["noise"]
    fb, steps = src.oc["focal"] * sc["baseline_m"], sc["disparity_steps"]
    for k in range(4):
        centre = recipe["t_q"][k] * 0.001
        z_max = centre[2] + r * 0.001
        e = 2 * np.sqrt(3.0) * (a + b * (z_max - z0) ** 2) + z_max ** 2 / (steps * fb)
        d = np.linalg.norm(res["pts"][k].cpu().numpy().astype(np.float64) - centre, axis=1)
        lo, hi = inscribed * 0.001 - e, r * 0.001 + e
        print("pair %d pts: %.6f .. %.6f inside %.6f .. %.6f (e = %.6f)" % (k, d.min(), d.max(), lo, hi, e))
        assert lo <= d.min() and d.max() <= hi
        assert not torch.equal(res["pts"][k], clean["pts"][k]) and d.max() - d.min() > 1e-3  # sensed: off the mesh by more than its own relief


def test_fit_online_scene_runs(models_dir, tmp_path):
    """`fit --online-models DIR --online-scene` on the small model of tests/test_fit_gpu.py: 2 iterations with finite losses."""
    from oracle.unopose_ref import default_cfg, random_state_dict  # weights only
    from unopose_amd import fit as F
    from unopose_amd.model import default_model_cfg

    torch.save({"model": random_state_dict(default_cfg(), seed=0, tame=0.1)}, tmp_path / "init.pth")
    data = dict(case.CFG, img_size=224, n_sample_observed_point=512, n_sample_template_point=1200)
    online = data.pop("online")
    cfg = {"train": {"max_iter": 2, "checkpointer": {"period": 2, "max_to_keep": 5}, "seed": 3, "log_period": 1, "clip_grad": {"enabled": True, "params": {"max_norm": 35}}},
           "dataloader": {"train": {"batch_size": 2, "dataset": {"cfg": data}, "online": online}}, "model": {"cfg": dict(default_model_cfg(fine_npoint=512))},
           "misc": {"load_from": str(tmp_path / "init.pth")}}
    (tmp_path / "cfg.json").write_text(json.dumps(cfg))
    assert F.main(["--config", str(tmp_path / "cfg.json"), "--online-models", models_dir, "--online-scene", "--output-dir", str(tmp_path / "a")]) == 0
    lines = [json.loads(line) for line in open(tmp_path / "a" / "metrics.json")]
    assert [r["iteration"] for r in lines] == [0, 1] and all(np.isfinite(r["total_loss"]) and np.isfinite(r["total_grad_norm"]) for r in lines)
    assert os.path.exists(tmp_path / "a" / "model_final.pth")
