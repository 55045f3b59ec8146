"""CPU: the online training pairs' recipe, draw and host item rule (unopose_amd/provider_online.py).  The rule's intermediates are held to the
provider's own expressions (`Window.around`, `lift_depth`, `to_resized`, `dilate_cross`) applied by hand to hand-made canvases."""
import numpy as np
import pytest
import torch

import megapose_synth
import online_pairs_case as case
from unopose_amd import provider_online as P
from unopose_amd import provider_train as T
from unopose_amd.provider import Window, _normalised_crop, lift_depth

KEYS = ("pts", "rgb", "rgb_choose", "translation_label", "rotation_label", "tem1_rgb", "tem1_choose", "tem1_pts", "K")


def _pair(name):
    k = case.NAMES.index(name)
    items, info = case.mirror()
    views, recipe = case.chunk()
    return k, items[k], info[k], views, recipe


def test_cases_are_what_their_names_say():
    items, info = case.mirror()
    assert {n for n, it in zip(case.NAMES, items) if it is not None} == case.VALID
    by = dict(zip(case.NAMES, info))
    assert by["kept_31"]["q_kept"] == 31 and by["kept_31"]["why"] == "kept points" and by["kept_32"]["q_kept"] == 32 and by["kept_32"]["valid"]
    assert by["kept_32"]["q_set"] > 32  # the keep rule, not the mask, decides
    assert by["fewer_than_wanted"]["q_kept"] < case.N_OBS and by["fewer_than_wanted"]["ref_set"] < case.N_TPL
    assert by["exactly_as_many"]["q_kept"] == case.N_OBS and by["exactly_as_many"]["ref_set"] == case.N_TPL
    assert by["plain"]["q_kept"] > case.N_OBS and by["plain"]["ref_set"] > case.N_TPL
    assert by["occluder_all"]["q_row"][1] == 0 and by["occluder_all"]["why"] == "query visibility"
    assert 0 < by["occluder_part"]["q_row"][1] < by["occluder_part"]["q_row"][0]
    assert by["object_outside"]["q_row"][0] == 0 and by["object_outside"]["why"] == "query visibility"
    assert by["reference_outside"]["why"] == "reference empty"
    assert by["top_left_odd"]["q_window"][0] == 0 and by["top_left_odd"]["q_window"][2] == 0 and by["top_left_odd"]["q_row"][4] % 2 == 1
    assert by["bottom_right"]["q_window"][1] == case.H and by["bottom_right"]["q_window"][3] == case.W
    assert by["tall_full_height"]["q_window"][:2] == [0, case.H]
    for n in ("dilate_edge_occluder", "dilate_plain"):
        assert by[n]["q_row"][2] > by[n]["q_row"][1]  # the mask grew


def test_item_dict_matches_the_megapose_provider(tmp_path):
    """Keys (in order), dtypes and per-item shapes of `collate_pairs` over MegaPoseOneRefTrainSet items."""
    cfg = megapose_synth.build(str(tmp_path))
    ds = T.MegaPoseOneRefTrainSet(cfg, num_img_per_epoch=4, color_augmentor=None)
    np.random.seed(3)
    ds.reset()
    ref = T.collate_pairs([ds[0], ds[1]])
    items, _ = case.mirror()
    mine = T.collate_pairs([P.finish_item(it, case.S) for it in items if it is not None][:2])
    assert tuple(mine) == tuple(ref) == KEYS
    sizes = {"pts": (case.N_OBS, 3), "rgb": (3, case.S, case.S), "rgb_choose": (case.N_OBS,), "tem1_rgb": (3, case.S, case.S), "tem1_choose": (case.N_TPL,),
             "tem1_pts": (case.N_TPL, 3)}
    for k in KEYS:
        assert mine[k].dtype == ref[k].dtype, k
        assert mine[k].dim() == ref[k].dim() and mine[k].shape[0] == 2, k
        assert tuple(mine[k].shape[1:]) == sizes.get(k, tuple(ref[k].shape[1:])), k


@pytest.mark.parametrize("name", sorted(case.VALID))
def test_intermediates_equal_the_providers_expressions(name):
    k, item, info, views, recipe = _pair(name)
    K = P.camera_matrix(P.online_cfg(case.CFG))
    rd, qd, cd = views["ref_depth"][k], views["q_depth"][k], views["occ_depth"][k]
    # reference: mask, window, pixels, draw, points, radius
    r_mask = rd > 0
    r_win = Window.around(r_mask)
    assert r_win.as_list() == info["ref_window"]
    r_pix = r_win.crop(r_mask).astype(np.float32).flatten().nonzero()[0]
    sel = P.draw_index(recipe["keys"][k, 0], np.arange(case.N_TPL), len(r_pix), case.N_TPL)
    choose = r_pix[sel]
    tem = lift_depth(rd.astype(np.float64) * 0.001, K, r_win).reshape(-1, 3)[choose]
    mean = np.zeros(3)
    for p in tem:
        mean = mean + p  # draw order
    mean = mean / case.N_TPL
    d = tem - mean
    radius = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).max()
    assert radius == info["radius"]
    assert np.array_equal(item["tem1_choose"].numpy(), r_win.to_resized(choose, case.S))
    spin = recipe["spin"][k]
    spun = np.stack([(tem[:, 0] * spin[0, j] + tem[:, 1] * spin[1, j]) + tem[:, 2] * spin[2, j] for j in range(3)], axis=1)
    assert np.array_equal(item["tem1_pts"].numpy(), spun.astype(np.float32))
    assert np.abs(spun - tem @ spin).max() < 1e-15
    # query: visible, scene, dilation, window, pixels, keep, draw
    visible = (qd > 0) & ((cd == 0) | (qd <= cd))
    assert np.array_equal(visible, info["q_visible"])
    scene = np.where(visible, qd, np.where(cd > 0, cd, 0)).astype(np.float32)
    assert np.array_equal(scene, info["scene_depth"])
    mask = T.dilate_cross(visible, 4) > 0 if recipe["dilate"][k] else visible
    assert np.array_equal(mask, info["q_mask"])
    assert list(info["q_row"][:3]) == [(qd > 0).sum(), visible.sum(), mask.sum()]
    q_win = Window.around(mask)
    assert q_win.as_list() == info["q_window"]
    inside = q_win.crop(mask)
    q_pix = inside.astype(np.float32).flatten().nonzero()[0]
    cloud = lift_depth(scene.astype(np.float64) * 0.001, K, q_win)
    total = np.zeros(3)
    for r in range(inside.shape[0]):  # a row left to right, the rows top to bottom
        row = np.zeros(3)
        for c in np.flatnonzero(inside[r]):
            row = row + cloud[r, c]
        total = total + row
    mean = total / len(q_pix)
    assert np.array_equal(mean, info["q_mean"])
    assert np.abs(mean - cloud.reshape(-1, 3)[q_pix].mean(axis=0)).max() < 1e-12  # the provider's np.mean, up to the order
    pts = cloud.reshape(-1, 3)[q_pix]
    d = pts - mean
    keep = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) < 1.2 * radius
    assert keep.sum() == info["q_kept"]
    q_pix, pts = q_pix[keep], pts[keep]
    sel = P.draw_index(recipe["keys"][k, 1], np.arange(case.N_OBS), len(q_pix), case.N_OBS)
    assert np.array_equal(item["rgb_choose"].numpy(), q_win.to_resized(q_pix[sel], case.S))
    want = pts[sel] + (recipe["shift"][k].reshape(1, 3) + 0.001 * recipe["noise"][k])
    assert np.array_equal(item["pts"].numpy(), want.astype(np.float32))
    # crops: the scene colour in the window, finished as the provider finishes a crop
    scene_rgb = np.where(visible[:, :, None], views["q_rgb"][k], np.where((cd > 0)[:, :, None], views["occ_rgb"][k], 0)).astype(np.uint8)
    assert np.array_equal(item["rgb_crop"], q_win.crop(scene_rgb)) and np.array_equal(item["rgb_cropmask"] != 0, inside)
    done = P.finish_item(item, case.S)
    assert torch.equal(done["rgb"], _normalised_crop(scene_rgb, q_win, case.S, inside))
    assert torch.equal(done["tem1_rgb"], _normalised_crop(views["ref_rgb"][k], r_win, case.S, r_win.crop(r_mask)))


def test_dilation_is_the_clipped_l1_ball():
    """What the kernel computes (any visible pixel within L1 distance 4, inside the image) is `dilate_cross(mask, 4)`, at the edge and beside
    the occluder as well."""
    for name in ("dilate_edge_occluder", "dilate_plain"):
        _, _, info, _, _ = _pair(name)
        vis = info["q_visible"]
        ys, xs = np.nonzero(vis)
        ball = np.zeros_like(vis)
        for dy in range(-4, 5):
            for dx in range(-(4 - abs(dy)), 4 - abs(dy) + 1):
                y, x = ys + dy, xs + dx
                ok = (y >= 0) & (y < case.H) & (x >= 0) & (x < case.W)
                ball[y[ok], x[ok]] = True
        assert np.array_equal(ball, info["q_mask"])
    _, _, info, views, _ = _pair("dilate_edge_occluder")
    k = case.NAMES.index("dilate_edge_occluder")
    grown = info["q_mask"] & ~info["q_visible"]
    assert (grown & (views["occ_depth"][k] > 0)).any() and info["q_row"][6] == case.W  # into the occluder, up to the image edge


def test_draw_index_range_and_repetition():
    for n_have, n_want in ((50, 20), (21, 20), (97, 96), (5000, 64), (2, 1), (1000, 999)):
        for key in (0, 1, 2 ** 64 - 1, 0x123456789ABCDEF):
            s = P.draw_index(key, np.arange(n_want), n_have, n_want)
            assert s.dtype == np.int64 and s.min() >= 0 and s.max() < n_have and len(set(s.tolist())) == n_want
            assert [P.draw_index(key, i, n_have, n_want) for i in range(min(n_want, 5))] == s[:5].tolist()  # no state between the i
    for n_have, n_want in ((7, 20), (20, 20), (1, 3), (64, 64)):
        s = P.draw_index(99, np.arange(n_want), n_have, n_want)
        assert s.min() >= 0 and s.max() < n_have
    assert len(set(P.draw_index(5, np.arange(400), 20, 400).tolist())) == 20  # n_have == n_want and below: with replacement, every index reachable


def test_draw_index_statistics():
    count = np.zeros(50, np.int64)
    for key in range(2000):
        count[P.draw_index(key * 0x9E3779B1 + 12345, np.arange(20), 50, 20)] += 1
    assert count.min() >= 690 and count.max() <= 910, (count.min(), count.max())  # mean 800, five binomial sigma of 21.9
    count = np.zeros(7, np.int64)
    for key in range(2000):
        np.add.at(count, P.draw_index(key * 0x9E3779B1 + 12345, np.arange(20), 7, 20), 1)
    assert count.min() >= 5364 and count.max() <= 6064, (count.min(), count.max())  # mean 5714, five sigma of 70


def test_draw_recipe_is_a_pure_function():
    state = np.random.get_state()
    a = P.draw_recipe(5, 1, 9, 3, case.MODELS, case.CFG)
    b = P.draw_recipe(5, 1, 9, 3, case.MODELS, case.CFG)
    after = np.random.get_state()
    assert all(np.array_equal(s, t) for s, t in zip(state, after) if isinstance(s, np.ndarray)) and state[2:] == after[2:]
    assert all(np.array_equal(a[k], b[k]) for k in a)
    for other in (P.draw_recipe(5, 0, 9, 3, case.MODELS, case.CFG), P.draw_recipe(5, 1, 10, 3, case.MODELS, case.CFG),
                  P.draw_recipe(6, 1, 9, 3, case.MODELS, case.CFG), P.draw_recipe(5, 1, 9, 3, case.MODELS, case.CFG, chunk=1)):
        assert not np.array_equal(a["R_q"], other["R_q"]) and not np.array_equal(a["keys"], other["keys"]) and not np.array_equal(a["noise"], other["noise"])
    assert np.array_equal(P.draw_recipe(5, 1, 9, 2, case.MODELS, case.CFG)["R_q"], a["R_q"][:2])  # pair k does not depend on the number of candidates
    for R in (a["R_ref"], a["R_q"], a["R_occ"], a["spin"]):
        assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-12 and np.abs(np.linalg.det(R) - 1).max() < 1e-12


def test_recipe_poses_follow_the_pose_rule():
    oc = P.online_cfg(case.CFG)
    r = P.draw_recipe(1, 0, 0, 40, case.MODELS, case.CFG)
    f, short = oc["focal"], min(case.H, case.W)
    for k in range(40):
        m = case.MODELS[int(r["obj"][k])]
        c_ref = r["R_ref"][k] @ m["centre"] + r["t_ref"][k]
        assert np.abs(c_ref[:2]).max() < 1e-9  # the reference looks straight at the object
        for c in (c_ref, r["R_q"][k] @ m["centre"] + r["t_q"][k]):
            fill = f * m["diameter"] / (c[2] * short)
            assert oc["fill"][0] - 1e-9 <= fill <= oc["fill"][1] + 1e-9
        c_q = r["R_q"][k] @ m["centre"] + r["t_q"][k]
        u, v = f * c_q[0] / c_q[2], f * c_q[1] / c_q[2]
        assert abs(u) <= oc["offset"] * case.W / 2 + 1e-9 and abs(v) <= oc["offset"] * case.H / 2 + 1e-9
        c_occ = r["R_occ"][k] @ case.MODELS[int(r["occ_obj"][k])]["centre"] + r["t_occ"][k]
        assert 0 < c_occ[2] <= max(0.75 * c_q[2], case.MODELS[int(r["occ_obj"][k])]["diameter"]) + 1e-9  # between camera and object
        assert r["occ_obj"][k] != r["obj"][k]
    assert 0 < r["occ"].sum() < 40 and 0 < r["dilate"].sum() < 40


def test_labels_are_the_float64_product_rounded_once():
    r = P.draw_recipe(2, 0, 4, 6, case.MODELS, case.CFG)
    for k in range(6):
        Tq, Tr, spin = np.eye(4), np.eye(4), np.eye(4)
        Tq[:3, :3], Tq[:3, 3] = r["R_q"][k], r["t_q"][k] * 0.001
        Tr[:3, :3], Tr[:3, 3] = r["R_ref"][k], r["t_ref"][k] * 0.001
        inv = np.eye(4)
        inv[:3, :3], inv[:3, 3] = Tr[:3, :3].T, -(Tr[:3, :3].T @ Tr[:3, 3])
        assert np.abs(inv - np.linalg.inv(Tr)).max() < 1e-12
        spin[:3, :3] = r["spin"][k]
        target = Tq @ inv @ spin
        assert r["rotation_label"].dtype == np.float32 and r["translation_label"].dtype == np.float32
        assert np.array_equal(r["rotation_label"][k], target[:3, :3].astype(np.float32))
        assert np.array_equal(r["translation_label"][k], (target[:3, 3] + r["shift"][k]).astype(np.float32))
        assert np.abs(r["shift"][k]).max() <= case.CFG["shift_range"]
    items, _ = case.mirror()
    _, recipe = case.chunk()
    for k, it in enumerate(items):
        if it is not None:
            assert np.array_equal(it["rotation_label"].numpy(), recipe["rotation_label"][k]) and np.array_equal(it["translation_label"].numpy(), recipe["translation_label"][k])


def test_plans_are_a_pure_function_and_follow_the_coin():
    sizes = [((24, 24), (30, 30)), ((12, 12), (8, 8))] * 10
    a, b = P.draw_plans(3, 0, 7, sizes), P.draw_plans(3, 0, 7, sizes)
    flat = [p for pair in a for p in pair]
    assert [[(o, np.asarray(v).tolist()) for o, v in p.ops] for p in flat] == [[(o, np.asarray(v).tolist()) for o, v in p.ops] for pair in b for p in pair]
    assert all((p.h, p.w) == hw for pair, s in zip(a, sizes) for p, hw in zip(pair, s) if len(p))
    assert 20 <= sum(len(p) > 0 for p in flat) <= 39  # the 0.8 coin over 40 images
    item = next(it for it in case.mirror()[0] if it is not None)
    plans = P.draw_plans(3, 0, 8, [(item["rgb_crop"].shape[:2], item["tem1_crop"].shape[:2])])[0]
    done = P.finish_item(item, case.S, True, plans)
    want = T.ColorAugmentor(0).apply(item["rgb_crop"], plans[0]) * (item["rgb_cropmask"][:, :, None] > 0)
    from unopose_amd.provider import resize_bilinear_u8, to_tensor_normalize

    assert torch.equal(done["rgb"], to_tensor_normalize(resize_bilinear_u8(np.ascontiguousarray(want.astype(np.uint8)), case.S)))
