"""GPU: the device path of the BOP test provider's query side (csrc/prep.hip, ops/prep.py, `BOPTestsetOneRef(..., device=...)`,
`cli --device-prep`) against the host provider, which is itself pinned to the reference by tests/golden/provider_dataset.npz.
The provider's arithmetic is integer (OpenCV's 11-bit bilinear) or float64 rounded once to fp32, so everything here is held to
EQUALITY: key set, dtype, shape, `np.array_equal`.  The one quantity that is not bit-defined -- a point's float64 distance to the
centroid, whose value depends on the order the centroid is summed in -- only enters through a comparison with a threshold; the
realistic-size test asserts on the host values that no point lies within 1e-9 relative of its threshold (summation order moves a
distance by ~1e-15 relative), under which the decision cannot flip."""
import json
import os

import numpy as np
import pytest
import torch

import bop_scenes
import bop_synth
from unopose_amd import provider as P

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEVICE_KEYS = ("pts", "rgb", "rgb_choose")


def assert_items_equal(got, want):
    """`got` from the device provider, `want` from the host provider: every key, dtype, shape and value."""
    assert list(got.keys()) == list(want.keys())
    for k, w in want.items():
        g = got[k]
        if not torch.is_tensor(w):
            assert g == w, k
            continue
        assert g.is_cuda == (k in DEVICE_KEYS), k
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g.cpu().numpy(), w.numpy()), (k, int((g.cpu() != w).sum()))


def states_equal(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def item_or_error(ds, i):
    try:
        return ds[i]
    except ValueError as e:
        return str(e)


# ---- 1. the reference's own items ---------------------------------------------------------------------------------
@pytest.fixture()
def synth(tmp_path):
    cfg, det_path = bop_synth.build(str(tmp_path / "bop"))
    return P.BOPTestsetOneRef(cfg, "ycbv", det_path), P.BOPTestsetOneRef(cfg, "ycbv", det_path, device="cuda")


def test_device_items_match_reference_provider_golden(synth):
    _, dev = synth
    z = np.load(os.path.join(GOLD, "provider_dataset.npz"))
    assert len(dev) == int(z["n_items"]) == 2
    np.random.seed(2024)
    items = [dev[i] for i in range(len(dev))]
    for i, it in enumerate(items):
        keys = {k.split("__", 1)[1] for k in z.files if k.startswith(f"item{i}__")}
        assert keys == set(it.keys()) - {"ref_keys"}
        for k in keys:
            assert it[k].is_cuda == (k in DEVICE_KEYS), k
            got, want = it[k].cpu().numpy(), z[f"item{i}__{k}"]
            assert got.dtype == want.dtype and got.shape == want.shape, k
            assert np.array_equal(got, want), (i, k, np.abs(got.astype(np.float64) - want).max())
    assert items[0]["ref_keys"] == [(10, 5, 2), (49, 7, 5)] and items[1]["ref_keys"] == [(10, 5, 2)]
    assert items[0]["inst_ids"].tolist() == [0, 1]


# ---- 2. the resize kernel against provider._normalised_crop ----------------------------------------------------------
def _windows(S, H, W):
    """sides: S (copy), 2S (area), 2, 3, odd and even sides below and above S up to 480; each placed at a corner of the image
    in turn (so every border is touched by copies, area windows and bilinear windows alike) or inside it"""
    sides = [S, 2 * S, 2, 3, S - 1, S + 1, S - 2 if S > 2 else 4, S + 2, 31, 97, 100, 333, 479, 480, S, 2 * S, 3, 480, 57, 224]
    wins = []
    for j, s in enumerate(sides):
        y0, x0 = [(0, 0), (0, W - s), (H - s, 0), (H - s, W - s), ((H - s) // 2, (W - s) // 3)][j % 5]
        wins.append(P.Window(y0, y0 + s, x0, x0 + s))
    wins.append(P.Window(0, 100, W - 140, W))  # not square: the two axes have their own taps
    return wins


@pytest.mark.parametrize("S", [56, 224, 518])
@pytest.mark.parametrize("masked,bgr,grey", [(True, False, False), (False, False, False), (True, True, False), (False, True, False),
                                             (True, False, True), (False, True, True)])
def test_crop_resize_bit_equal_to_normalised_crop(S, masked, bgr, grey):
    from unopose_amd import ops

    rs = np.random.RandomState(S + 2 * masked + 4 * bgr + 8 * grey)
    H, W = max(2 * S, 480) + 7, max(2 * S, 480) + 40
    img = rs.randint(0, 256, size=(H, W) if grey else (H, W, 3)).astype(np.uint8)
    wins = _windows(S, H, W)
    masks = [rs.rand(w.y1 - w.y0, w.x1 - w.x0) < 0.7 for w in wins]
    for m in masks:
        m[0, 0] = True  # a plan takes no empty mask
    plan = ops.PrepPlan((H, W), wins, masks, S, "cuda")
    got = ops.prep_crop_resize(torch.from_numpy(img).cuda(), plan, bgr=bgr, use_mask=masked).cpu()
    for d, (w, m) in enumerate(zip(wins, masks)):
        want = P._normalised_crop(img, w, S, m if masked else None, bgr)
        assert got[d].dtype == want.dtype and got[d].shape == want.shape
        assert torch.equal(got[d], want), (w.as_list(), int((got[d] != want).sum()))


def test_normalisation_table_is_the_providers_values():
    from unopose_amd import ops

    lut = ops.prep_norm_table("cuda").cpu().reshape(3, 256)
    img = np.repeat(np.arange(256, dtype=np.uint8).reshape(16, 16, 1), 3, axis=2)
    want = P.to_tensor_normalize(img).reshape(3, 256)  # all 256 x 3 values, through a full-size call of the provider's function
    assert torch.equal(lut, want)


# ---- 3. realistic size, radius filter active --------------------------------------------------------------------------
def _watch_filter(ds, log):
    """Record, for every detection of the HOST provider that reaches the radius filter: points, survivors, the smallest relative gap
    between a distance and the threshold, and whether the detection was dropped.  No random number is consumed here."""
    ref_of, get = ds._reference_instance, ds.get_instance
    last = {}

    def reference(*a):
        last["ref"] = ref_of(*a)
        return last["ref"]

    def instance(det):
        last["ref"] = None
        out = get(det)
        if last["ref"] is not None:
            K, scale = ds.files.camera(ds.data_folder, det["scene_id"], det["image_id"])
            depth = ds.files.depth_m(ds.data_folder, det["scene_id"], det["image_id"], scale)
            valid = np.logical_and(P.rle_decode(det["segmentation"]) > 0, depth > 0)
            win = P.Window.around(valid)
            cloud = P.lift_depth(depth, K, win).reshape(-1, 3)[np.flatnonzero(win.crop(valid))]
            dist = np.linalg.norm(cloud - np.mean(cloud, axis=0)[None, :], axis=1)
            ref_pts = last["ref"][2]
            thr = 1.2 * np.max(np.linalg.norm(ref_pts - np.mean(ref_pts, axis=0).reshape(1, 3), axis=1))
            log.append((len(dist), int(np.sum(dist < thr)), float(np.min(np.abs(dist - thr)) / thr), out is None))
        return out

    ds._reference_instance, ds.get_instance = reference, instance


def test_realistic_scenes_with_active_radius_filter(tmp_path):
    cfg, det_path = bop_scenes.build(str(tmp_path / "bop"), n_images=16, seed=0)
    host, dev = P.BOPTestsetOneRef(cfg, "lm", det_path), P.BOPTestsetOneRef(cfg, "lm", det_path, device="cuda")
    log = []
    _watch_filter(host, log)
    np.random.seed(31)
    want = [item_or_error(host, i) for i in range(len(host))]
    state = np.random.get_state()
    # precondition of equality, on the host values, no scene left out: no distance within 1e-9 relative of its threshold
    points, kept, gap, dropped = (np.array(c) for c in zip(*log))
    print(f"{len(log)} filtered detections; closest distance to a threshold {gap.min():.3g} relative; most points removed "
          f"{(points - kept).max()}; dropped after the reference draw {int(dropped.sum())}")
    assert len(host) == 16 and gap.min() > 1e-9
    assert (points - kept).max() > 1000  # the filter removes thousands of points somewhere ...
    assert dropped.any() and (kept[dropped] < cfg["minimum_n_point"]).all()  # ... and leaves nothing of some detection
    np.random.seed(31)
    for i, w in enumerate(want):
        g = item_or_error(dev, i)
        if isinstance(w, str):
            assert g == w
        else:
            assert_items_equal(g, w)
    assert states_equal(np.random.get_state(), state)


# ---- 4. control flow ----------------------------------------------------------------------------------------------------
def _both(synth, index, seed):
    host, dev = synth
    np.random.seed(seed)
    want = item_or_error(host, index)
    state = np.random.get_state()
    np.random.seed(seed)
    got = item_or_error(dev, index)
    assert states_equal(np.random.get_state(), state)
    if isinstance(want, str):
        assert got == want
    else:
        assert_items_equal(got, want)
    return want


def test_best_detection_kept_when_all_scores_low_on_the_device(synth):
    for ds in synth:
        ds.dets[ds.det_keys[1]][0]["score"] = 0.05
    want = _both(synth, 1, 0)
    assert want["pts"].shape[0] == 1 and want["inst_ids"].tolist() == [0]


def test_detection_without_reference_target(synth):
    for ds in synth:
        del ds.test_ref_target["48_1_5"]
    want = _both(synth, 0, 1)
    assert want["inst_ids"].tolist() == [0]


def test_detection_with_too_few_valid_pixels(synth):
    tiny = np.zeros((bop_synth.H, bop_synth.W), bool)
    tiny[40:42, 40:43] = True  # 6 pixels: not more than minimum_n_point = 8
    for ds in synth:
        ds.dets[ds.det_keys[0]][0]["segmentation"] = P.rle_encode(tiny)
    want = _both(synth, 0, 2)
    assert want["inst_ids"].tolist() == [1]
    for ds in synth:  # and the image's only detection: nothing qualifies, on either path
        ds.dets[ds.det_keys[1]][0]["segmentation"] = P.rle_encode(tiny)
    assert "no qulified instance" in _both(synth, 1, 3)


def test_unfiltered_items_leave_the_same_random_state(synth):
    for index, seed in ((0, 5), (1, 6), (0, 7)):
        _both(synth, index, seed)


# ---- 5. end to end -------------------------------------------------------------------------------------------------------
@torch.no_grad()
def test_cli_device_prep_writes_the_same_lines(tmp_path):
    from unopose_amd import cli
    from unopose_amd.model import UNOPose, default_model_cfg
    from unopose_amd.synthetic import trained_like_

    dcfg, det_path = bop_synth.build(str(tmp_path / "bop"))
    mcfg = default_model_cfg(fine_npoint=256, feature_extraction=dict(img_size=dcfg["img_size"]))
    torch.manual_seed(3)
    model = trained_like_(UNOPose(mcfg))
    ckpt = str(tmp_path / "model_final.pth")
    torch.save({"model": model.state_dict(), "iteration": 7}, ckpt)
    cfg = dict(model=dict(cfg=dict(mcfg)), dataloader=dict(test=dict(dataset=dict(cfg=dcfg, eval_dataset_name="ycbv", detetion_path=det_path))),
               test=dict(amp=dict(enabled=False), instance_batch_size=2), misc=dict(output_dir=str(tmp_path / "out"), load_from=""), bop_eval=dict(split="test"))
    cfgf = tmp_path / "cfg.json"
    cfgf.write_text(json.dumps(cfg))
    path = tmp_path / "out" / "inference_model_final" / "ycbv" / "result_t_ycbv-test.csv"

    def run(*flags):
        np.random.seed(11)
        torch.manual_seed(5)  # the coarse stage draws inside forward
        assert cli.main(["--config-file", str(cfgf), *flags, f"misc.load_from={ckpt}", "misc.exp_name=_t"]) == 0
        lines = path.read_text().splitlines()
        path.unlink()
        return [",".join(line.strip().split(",")[:-1]) for line in lines]  # last field = wall-clock time

    for flags in ((), ("--pipeline", "--ref-cache")):
        want = run(*flags)
        got = run(*flags, "--device-prep")
        assert len(want) >= 3 and got == want, flags


# ---- 6. hygiene -------------------------------------------------------------------------------------------------------------
def _guarded(shape, dtype, fill):
    n = int(np.prod(shape))
    buf = torch.full((n + 64,), fill, dtype=dtype, device="cuda")
    return buf, buf[:n].view(shape)


def test_outputs_fully_written_and_guards_untouched():
    from unopose_amd import ops

    rs = np.random.RandomState(9)
    H, W, S, n = 120, 160, 56, 300
    img = rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    depth = rs.uniform(0.5, 1.5, size=(H, W))
    K = np.array([[110.0, 0, 80.5], [0, 112.0, 59.5], [0, 0, 1]])
    wins = [P.Window(0, 56, 0, 56), P.Window(8, 120, 48, 160), P.Window(31, 98, 5, 72), P.Window(100, 103, 157, 160)]
    masks = [rs.rand(w.side, w.side) < 0.5 for w in wins]
    masks[3][:] = True
    masks[2][5] = False  # an empty window row
    plan = ops.PrepPlan((H, W), wins, masks, S, "cuda")
    N = plan.n_points
    assert N == sum(int(m.sum()) for m in masks)

    cbuf, crops = _guarded((len(wins), 3, S, S), torch.float32, float("nan"))
    ops.prep_crop_resize(torch.from_numpy(img).cuda(), plan, out=crops)
    pbuf, pix = _guarded((N,), torch.int32, -7)
    xbuf, cloud = _guarded((N, 3), torch.float64, float("nan"))
    dbuf, dist = _guarded((N,), torch.float64, float("nan"))
    ops.prep_lift(torch.from_numpy(depth).cuda(), K, plan, out=(pix, cloud, dist))
    picked = [0, 2, 3]
    index = np.stack([rs.randint(0, int(plan.n[d]), size=n) + int(plan.pt_off[d]) for d in picked])
    tbuf, pts = _guarded((len(picked), n, 3), torch.float32, float("nan"))
    ibuf, choose = _guarded((len(picked), n), torch.int64, -7)
    ops.prep_gather(plan, picked, index, pix, cloud, out=(pts, choose))
    torch.cuda.synchronize()

    for buf, fill in ((cbuf, None), (xbuf, None), (dbuf, None), (tbuf, None), (pbuf, -7), (ibuf, -7)):
        guard = buf[-64:]
        assert bool(torch.isnan(guard).all()) if fill is None else bool((guard == fill).all())
    # every element written, with the host provider's values
    want_pix = np.concatenate([np.flatnonzero(m) for m in masks])
    want_cloud = np.concatenate([P.lift_depth(depth, K, w).reshape(-1, 3)[np.flatnonzero(m)] for w, m in zip(wins, masks)])
    assert np.array_equal(pix.cpu().numpy(), want_pix)
    assert np.array_equal(cloud.cpu().numpy(), want_cloud)
    got_dist, at = dist.cpu().numpy(), 0
    for m in masks:
        c = want_cloud[at:at + int(m.sum())]
        want = np.linalg.norm(c - np.mean(c, axis=0)[None, :], axis=1)
        # the centroid is a sum of up to n = 1.3e4 coordinates below 2.3 m in another order: each sum differs by less than n * 2^-53 * 2.3 m
        # = 3.3e-12 m, a distance by less than sqrt(3) times that plus roundings of a few 2^-53: 1e-11 m bounds it
        assert not np.isnan(got_dist[at:at + len(c)]).any() and np.abs(got_dist[at:at + len(c)] - want).max() < 1e-11
        at += len(c)
    for d, (w, m) in enumerate(zip(wins, masks)):
        assert torch.equal(crops[d].cpu(), P._normalised_crop(img, w, S, m, False))
    for p, d in enumerate(picked):
        assert np.array_equal(pts[p].cpu().numpy(), torch.FloatTensor(want_cloud[index[p]]).numpy())
        local = want_pix[index[p]]
        assert np.array_equal(choose[p].cpu().numpy(), wins[d].to_resized(local, S))


def test_cpu_tensors_and_bad_plans_raise(tmp_path):
    from unopose_amd import ops

    win, mask = P.Window(0, 10, 0, 10), np.ones((10, 10), bool)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        ops.PrepPlan((20, 20), [win], [mask], 8, "cpu")
    with pytest.raises(RuntimeError, match="CPU not supported"):
        ops.prep_norm_table("cpu")
    plan = ops.PrepPlan((20, 20), [win], [mask], 8, "cuda")
    img, depth = torch.zeros(20, 20, 3, dtype=torch.uint8), torch.ones(20, 20, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        ops.prep_crop_resize(img, plan)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        ops.prep_lift(depth, np.eye(3), plan)
    pix, cloud, _ = ops.prep_lift(depth.cuda(), np.eye(3), plan)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        ops.prep_gather(plan, [0], np.zeros((1, 4), np.int64), pix.cpu(), cloud)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        ops.prep_crop_resize(img.cuda(), plan, out=torch.empty(1, 3, 8, 8))
    # descriptors are checked on the host before anything reaches a kernel
    with pytest.raises(ValueError):
        ops.PrepPlan((20, 20), [P.Window(15, 25, 0, 10)], [mask], 8, "cuda")
    with pytest.raises(ValueError):
        ops.PrepPlan((20, 20), [win], [np.ones((9, 10), bool)], 8, "cuda")
    with pytest.raises(ValueError):
        ops.prep_gather(plan, [0], np.full((1, 4), 100, np.int64), pix, cloud)
    cfg, det_path = bop_synth.build(str(tmp_path / "bop"))
    with pytest.raises(RuntimeError, match="CPU not supported"):
        P.BOPTestsetOneRef(cfg, "ycbv", det_path, device="cpu")


def test_image_without_candidates_launches_nothing(synth, monkeypatch):
    from unopose_amd.ops import prep

    host, dev = synth
    calls = []
    monkeypatch.setattr(prep, "call", lambda *a: calls.append(a[0]))
    monkeypatch.setattr(prep, "PrepPlan", lambda *a: calls.append("plan"))
    for ds in synth:
        ds.minimum_n_point = 10 ** 6  # no detection has that many valid pixels: each is dropped before its reference lookup
    np.random.seed(4)
    before = np.random.get_state()
    for ds in synth:
        with pytest.raises(ValueError, match="no qulified instance in 000048_000001"):
            ds[0]
        assert states_equal(np.random.get_state(), before)
    assert calls == [] and dev._device_image is None
