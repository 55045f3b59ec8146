"""GPU: the online training pairs on the device (csrc/train_items.hip through ops/items.py and provider_online.OnlinePairs) against the host
item rule -- equal exactly, since the rule fixes every operation order -- on the hand-made canvases of online_pairs_case and on real renders;
the geometry of the points against the mesh itself; and `fit --online-models`."""
import json
import os

import numpy as np
import pytest
import torch

import online_pairs_case as case

pytestmark = pytest.mark.gpu

KEYS = ("pts", "rgb", "rgb_choose", "translation_label", "rotation_label", "tem1_rgb", "tem1_choose", "tem1_pts", "K")


@pytest.fixture(scope="module")
def models_dir(tmp_path_factory):
    """Object 1: textured, with normals; object 2: vertex colours, no normals (render_train_case's two small ellipsoids)."""
    import render_train_case

    return os.path.join(render_train_case.write_dataset(str(tmp_path_factory.mktemp("online"))), "models")


def _source(models_dir, **kw):
    from unopose_amd.provider_online import OnlinePairs

    cfg = dict(case.CFG, **kw.pop("cfg", {}))
    return OnlinePairs(models_dir, cfg, "cuda", kw.pop("seed", 5), **kw)


@pytest.fixture(scope="module")
def hand(models_dir):
    """The hand-made chunk uploaded as if rendered, through the device route once -> (source, chunk result, taken list)."""
    views, recipe = case.chunk()
    src = _source(models_dir, augment=False)
    up = lambda *names: torch.from_numpy(np.concatenate([views[n] for n in names])).cuda()  # noqa: E731
    res = src.chunk_device(recipe, (up("q_rgb", "ref_rgb"), up("q_depth", "ref_depth"), up("occ_rgb"), up("occ_depth")))
    taken = [(recipe, res, int(k)) for k in np.flatnonzero(res["valid"])]
    return src, res, taken


def test_view_table_masks_and_scene_equal_the_mirror(hand):
    _, res, _ = hand
    views, recipe = case.chunk()
    _, info = case.mirror()
    C = len(case.NAMES)
    mask, depth, rgb = res["mask"].cpu().numpy(), res["scene_depth"].cpu().numpy(), res["scene_rgb"].cpu().numpy()
    for k, name in enumerate(case.NAMES):
        assert np.array_equal(res["table"][k], info[k]["q_row"]), name
        assert np.array_equal(res["table"][C + k], info[k]["ref_row"]), name
        assert np.array_equal(mask[k] != 0, info[k]["q_mask"]) and np.array_equal(mask[C + k] != 0, info[k]["ref_mask"]), name
        assert np.array_equal(depth[k], info[k]["scene_depth"]) and np.array_equal(rgb[k], info[k]["scene_rgb"]), name
        assert np.array_equal(depth[C + k], views["ref_depth"][k]), name
        assert np.array_equal(rgb[C + k], np.where(info[k]["ref_mask"][:, :, None], views["ref_rgb"][k], 0)), name
    assert set(np.unique(mask)) <= {0, 1}


def test_windows_counts_flags_and_radius_equal_the_mirror(hand):
    _, res, _ = hand
    items, info = case.mirror()
    assert [bool(v) for v in res["valid"]] == [it is not None for it in items]
    radius = res["radius"].cpu().numpy()
    seen = 0
    for k, name in enumerate(case.NAMES):
        if "q_window" not in info[k]:  # no window: invalid by the table alone
            assert res["q_win"][k] is None or info[k]["why"] == "reference window empty", name
            continue
        seen += 1
        q, r = res["q_win"][k], res["r_win"][k]
        assert q.as_list() == info[k]["q_window"] and r.as_list() == info[k]["ref_window"], name
        assert np.array_equal(res["q_rows"][k][:q.side], info[k]["q_rows"]) and np.array_equal(res["r_rows"][k][:r.side], info[k]["ref_rows"]), name
        assert list(res["q_counts"][k]) == [info[k]["q_set"], info[k]["q_kept"]] and list(res["r_counts"][k]) == [info[k]["ref_set"]] * 2, name
        assert radius[k] == info[k]["radius"], name
    assert seen == len(case.VALID) + 1  # the valid pairs and the one with 31 kept points


def test_points_indices_and_labels_equal_the_mirror(hand):
    src, res, taken = hand
    items, _ = case.mirror()
    _, recipe = case.chunk()
    assert [k for _, _, k in taken] == [k for k, it in enumerate(items) if it is not None]
    for _, _, k in taken:
        for key in ("pts", "rgb_choose", "tem1_pts", "tem1_choose"):
            got = res[key][k].cpu()
            assert got.dtype == items[k][key].dtype and torch.equal(got, items[k][key]), (case.NAMES[k], key)
        lab = src._labels(recipe, [k])
        for key in ("translation_label", "rotation_label", "K"):
            assert torch.equal(lab[key][0].cpu(), items[k][key]), (case.NAMES[k], key)


def test_atlas_and_finished_crops_equal_the_mirror(hand):
    from unopose_amd import ops
    from unopose_amd.provider_online import finish_item
    from unopose_amd.provider_train import AugPlan, collate_pairs_device

    src, _, taken = hand
    items, _ = case.mirror()
    mine = [dict(items[k], rgb_plan=AugPlan(), tem1_plan=AugPlan()) for _, _, k in taken]
    want = collate_pairs_device(mine, case.S, True)
    got = src.collate_device(3, taken)
    assert set(got) == set(want)
    for key in want:
        assert got[key].dtype == want[key].dtype and torch.equal(got[key].cpu(), want[key]), key
    done = ops.finish_crops(got, "cuda")
    assert set(done) == set(KEYS)
    for n, (_, _, k) in enumerate(taken):
        ref = finish_item(items[k], case.S)
        for key in KEYS:
            assert done[key].dtype == ref[key].dtype and torch.equal(done[key][n].cpu(), ref[key]), (case.NAMES[k], key)


def test_augmented_crops_equal_apply_on_the_mirrors_crops(hand, models_dir):
    from unopose_amd import ops
    from unopose_amd.provider_online import draw_plans
    from unopose_amd.provider_train import OP_GRAYSCALE, ColorAugmentor

    _, _, taken = hand
    src = _source(models_dir, seed=9)  # augment=True
    items, _ = case.mirror()
    got = src.collate_device(4, taken)
    sizes = [(items[k]["rgb_crop"].shape[:2], items[k]["tem1_crop"].shape[:2]) for _, _, k in taken]
    plans = draw_plans(9, 0, 4, sizes)
    flat = [p[0] for p in plans] + [p[1] for p in plans]
    crops = [items[k]["rgb_crop"] for _, _, k in taken] + [items[k]["tem1_crop"] for _, _, k in taken]
    assert sum(len(p) > 0 for p in flat) > len(flat) // 2 and any(op == OP_GRAYSCALE for p in flat for op, _ in p.ops)
    atlas = ops.color_augment(got["crop_atlas"], None, tuple(got[k] for k in ("crop_desc", "crop_ops", "crop_grids", "crop_noise"))).cpu().numpy()
    aug = ColorAugmentor(0)
    for (y0, h, w), crop, plan in zip(got["crop_desc"][:, :3].tolist(), crops, flat):
        want = aug.apply(crop, plan)
        diff = np.abs(atlas[y0:y0 + h, :w].astype(np.int16) - want.astype(np.int16)).max()
        assert diff <= (1 if any(op == OP_GRAYSCALE for op, _ in plan.ops) else 0)  # ops.finish_crops' documented exception


def _equal(a, b):
    return tuple(a) == tuple(b) == KEYS and all(a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]) for k in KEYS)


def test_source_equals_the_mirror_on_real_renders_and_is_a_pure_function(models_dir):
    dev, host, again = _source(models_dir), _source(models_dir, host=True), _source(models_dir)
    shapes = {"pts": (4, case.N_OBS, 3), "rgb": (4, 3, case.S, case.S), "rgb_choose": (4, case.N_OBS), "translation_label": (4, 3), "rotation_label": (4, 3, 3),
              "tem1_rgb": (4, 3, case.S, case.S), "tem1_choose": (4, case.N_TPL), "tem1_pts": (4, case.N_TPL, 3), "K": (4, 3, 3)}
    first = [dev.batch(i) for i in range(5)]
    b5 = dev.batch(5)
    assert {k: tuple(v.shape) for k, v in b5.items()} == shapes and all(v.is_cuda for v in b5.values())
    assert b5["rgb_choose"].dtype == torch.int64 and b5["pts"].dtype == torch.float32 and int(b5["rgb_choose"].max()) < case.S * case.S
    assert _equal(b5, host.batch(5)) and _equal(first[2], host.batch(2))  # host=False and host=True
    assert _equal(b5, again.batch(5))  # batch(5) without batches 0-4 before it; another object: equal bits
    assert _equal(first[0], dev.batch(0)) and not torch.equal(first[0]["pts"], first[1]["pts"])
    assert not _equal(b5, _source(models_dir, rank=1).batch(5)) and not _equal(b5, _source(models_dir, seed=6).batch(5))
    assert float(b5["rgb"].std()) > 0.1 and float(b5["tem1_rgb"].std()) > 0.1  # pictures, not blanks
    it = dev.iterate(4)  # the prefetching iterator hands out the same batches, from its start iteration
    assert _equal(next(it), first[4]) and _equal(next(it), b5)
    it.close()


def test_batch_is_the_first_valid_candidates_in_order(models_dir):
    from unopose_amd.provider_online import draw_recipe

    cfg = dict(min_visib_fract=0.6, online=dict(case.CFG["online"], occluder_prob=0.8))  # most occluded queries fall below 0.6
    src = _source(models_dir, cfg=cfg, augment=False)
    for iteration in range(4):
        want, flags = [], []
        for chunk in range(8):
            recipe = draw_recipe(5, 0, iteration, 4, src.models, src.cfg, chunk=chunk)
            res = src.chunk_device(recipe, src.render_chunk(recipe))
            flags += [bool(v) for v in res["valid"]]
            want += [recipe["translation_label"][k] for k in np.flatnonzero(res["valid"])]
            if len(want) >= 4:
                break
        print("iteration", iteration, "valid flags", flags)
        if len(want) >= 4 and not all(flags[:[i for i, ok in enumerate(flags) if ok][3]]):  # an invalid candidate stands before the batch's last pair
            break
    else:
        pytest.fail("no iteration with an invalid candidate among the first ones: the thresholds do not bite")
    got = src.batch(iteration)
    assert np.array_equal(got["translation_label"].cpu().numpy(), np.stack(want[:4]))
    with pytest.raises(RuntimeError, match="valid pairs"):
        _source(models_dir, cfg=dict(min_px_count_visib=10 ** 6), augment=False).batch(0)


def test_points_lie_on_the_mesh(tmp_path):
    """Independent of the mirror: an icosphere of radius r, no occluder, no dilation, shift and noise 0.  Every query point, and every
    reference point carried over by the labels, lies between the mesh's inscribed radius and r from the query pose's translation.  The
    depth renderer equals its numpy form bit for bit (tests/test_render_gpu.py grants it no tolerance), so the band is not widened."""
    from bop_eval_case import icosphere
    from render_train_case import write_model_ply
    from unopose_amd.provider_online import draw_recipe

    r = 40.0
    v, f = icosphere()
    write_model_ply(str(tmp_path / "obj_000001.ply"), v * r, f, normals=v)
    tri = v[f] * r
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    inscribed = np.abs((tri[:, 0] * n).sum(axis=1) / np.linalg.norm(n, axis=1)).min()  # the nearest face plane
    assert 0.9 * r < inscribed < r
    cfg = dict(shift_range=0.0, online=dict(case.CFG["online"], occluder_prob=0.0, offset=0.2))
    src = _source(str(tmp_path), cfg=cfg, augment=False)
    assert abs(src.models[1]["diameter"] - 2 * r) < 1e-9
    recipe = draw_recipe(3, 0, 0, 4, src.models, src.cfg)
    recipe["noise"][:] = 0.0
    recipe["dilate"][:] = False
    assert not recipe["occ"].any() and not recipe["shift"].any()
    res = src.chunk_device(recipe, src.render_chunk(recipe))
    assert res["valid"].all()
    lo, hi = inscribed * 0.001, r * 0.001
    for k in range(4):
        centre = recipe["t_q"][k] * 0.001
        d = np.linalg.norm(res["pts"][k].cpu().numpy().astype(np.float64) - centre, axis=1)
        print("pair %d pts: %.9f .. %.9f inside %.9f .. %.9f" % (k, d.min(), d.max(), lo, hi))
        assert lo <= d.min() and d.max() <= hi
        moved = res["tem1_pts"][k].cpu().numpy().astype(np.float64) @ recipe["rotation_label"][k].astype(np.float64).T + recipe["translation_label"][k].astype(np.float64)
        d = np.linalg.norm(moved - centre, axis=1)
        print("pair %d tem1: %.9f .. %.9f" % (k, d.min(), d.max()))
        assert lo <= d.min() and d.max() <= hi


def test_fit_online_models_runs_and_resumes_on_the_same_batches(models_dir, tmp_path, monkeypatch):
    """`fit --online-models` on the small model of tests/test_fit_gpu.py: 4 iterations write checkpoints and metrics with finite losses; a run
    stopped after iteration 1 and resumed is fed the batches of iterations 2 and 3 the uninterrupted run was fed."""
    from oracle.unopose_ref import default_cfg, random_state_dict  # weights only
    from unopose_amd import fit as F
    from unopose_amd.model import default_model_cfg

    torch.save({"model": random_state_dict(default_cfg(), seed=0, tame=0.1)}, tmp_path / "init.pth")
    data = dict(case.CFG, img_size=224, n_sample_observed_point=512, n_sample_template_point=1200)
    online = data.pop("online")
    cfg = {"train": {"max_iter": 4, "checkpointer": {"period": 2, "max_to_keep": 5}, "seed": 3, "log_period": 1, "clip_grad": {"enabled": True, "params": {"max_norm": 35}}},
           "dataloader": {"train": {"batch_size": 2, "dataset": {"cfg": data}, "online": online}}, "model": {"cfg": dict(default_model_cfg(fine_npoint=512))},
           "misc": {"load_from": str(tmp_path / "init.pth")}}
    (tmp_path / "cfg.json").write_text(json.dumps(cfg))
    fed = []
    step = F.train_step_gated

    def recording(model, batch, *a, **kw):
        fed.append({k: v.detach().cpu().clone() for k, v in batch.items()})
        return step(model, batch, *a, **kw)

    monkeypatch.setattr(F, "train_step_gated", recording)
    base = ["--config", str(tmp_path / "cfg.json"), "--online-models", models_dir, "--workers", "5"]
    assert F.main(base + ["--output-dir", str(tmp_path / "a")]) == 0
    whole, fed[:] = list(fed), []
    assert sorted(os.listdir(tmp_path / "a")) == ["last_checkpoint", "metrics.json", "model_0000001.pth", "model_0000003.pth", "model_final.pth"]
    lines = [json.loads(line) for line in open(tmp_path / "a" / "metrics.json")]
    assert [r["iteration"] for r in lines] == [0, 1, 2, 3] and all(np.isfinite(r["total_loss"]) and np.isfinite(r["total_grad_norm"]) for r in lines)
    assert len(whole) == 4 and tuple(whole[0]) == KEYS and whole[0]["rgb"].shape == (2, 3, 224, 224) and whole[0]["tem1_pts"].shape == (2, 1200, 3)
    assert F.main(base + ["--output-dir", str(tmp_path / "b"), "--max-iter", "2"]) == 0
    assert F.main(base + ["--output-dir", str(tmp_path / "b"), "--resume"]) == 0
    assert len(fed) == 4 and torch.load(tmp_path / "b" / "model_final.pth", map_location="cpu")["iteration"] == 3
    for i in range(4):
        assert all(torch.equal(fed[i][k], whole[i][k]) for k in KEYS), i
