"""GPU: the provider's device path with the detections' run-length masks decoded on the device as well (`BOPTestsetOneRef(...,
device=..., device_masks=True)`, `cli --device-prep --device-masks`) against the device path that decodes them on the host -- itself
pinned to the host provider and to the reference by tests/test_device_prep_gpu.py -- and `python -m unopose_amd.coco_gt` on the device
against its `--host` route.  Masks, counts and extents are integers and everything after them is the same code on the same values, so
the items are held to `torch.equal` per key and the ``np.random`` state to equality."""
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
    assert list(got.keys()) == list(want.keys())
    for k, w in want.items():
        g = got[k]
        if not torch.is_tensor(w):
            assert g == w, k
            continue
        assert g.device == w.device and g.is_cuda == (k in DEVICE_KEYS) and g.dtype == w.dtype, k
        assert torch.equal(g, w), k


def states_equal(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def item_or_error(ds, i):
    try:
        return ds[i]
    except ValueError as e:
        return str(e)


@pytest.fixture()
def synth(tmp_path):
    cfg, det_path = bop_synth.build(str(tmp_path / "bop"))
    return P.BOPTestsetOneRef(cfg, "ycbv", det_path, device="cuda"), P.BOPTestsetOneRef(cfg, "ycbv", det_path, device="cuda", device_masks=True)


def _both(pair, index, seed):
    plain, masked = pair
    np.random.seed(seed)
    want = item_or_error(plain, index)
    state = np.random.get_state()
    np.random.seed(seed)
    got = item_or_error(masked, index)
    assert states_equal(np.random.get_state(), state)
    if isinstance(want, str):
        assert got == want
    else:
        assert_items_equal(got, want)
    return want


def test_items_equal_the_device_path_and_the_reference_golden(synth):
    for index, seed in ((0, 5), (1, 6), (0, 7)):
        _both(synth, index, seed)
    z = np.load(os.path.join(GOLD, "provider_dataset.npz"))
    masked = synth[1]
    np.random.seed(2024)
    items = [masked[i] for i in range(len(masked))]
    assert len(items) == int(z["n_items"]) == 2
    for i, it in enumerate(items):
        keys = {k.split("__", 1)[1] for k in z.files if k.startswith(f"item{i}__")}
        assert keys == set(it.keys()) - {"ref_keys"}
        for k in keys:
            got, want = it[k].cpu().numpy(), z[f"item{i}__{k}"]
            assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), (i, k)


def test_realistic_scenes_equal_the_device_path(tmp_path):
    cfg, det_path = bop_scenes.build(str(tmp_path / "bop"), n_images=6, seed=0)
    pair = P.BOPTestsetOneRef(cfg, "lm", det_path, device="cuda"), P.BOPTestsetOneRef(cfg, "lm", det_path, device="cuda", device_masks=True)
    np.random.seed(31)
    want = [item_or_error(pair[0], i) for i in range(len(pair[0]))]
    state = np.random.get_state()
    np.random.seed(31)
    for i, w in enumerate(want):
        g = item_or_error(pair[1], i)
        if isinstance(w, str):
            assert g == w
        else:
            assert_items_equal(g, w)
    assert states_equal(np.random.get_state(), state)
    assert len(want) == 6 and sum(int(w["pts"].shape[0]) for w in want if not isinstance(w, str)) > 20
    kinds = {type(d["segmentation"]["counts"]) for dets in pair[1].dets.values() for d in dets}
    assert kinds == {list, str}  # lists and strings mixed in one decode


def test_best_detection_kept_when_all_scores_low(synth):
    for ds in synth:
        ds.dets[ds.det_keys[1]][0]["score"] = 0.05
    want = _both(synth, 1, 0)
    assert want["pts"].shape[0] == 1 and want["inst_ids"].tolist() == [0]


def test_detection_without_reference_target(synth):
    for ds in synth:
        del ds.test_ref_target["48_1_5"]
    assert _both(synth, 0, 1)["inst_ids"].tolist() == [0]


def test_detection_with_too_few_valid_pixels(synth):
    tiny = np.zeros((bop_synth.H, bop_synth.W), bool)
    tiny[40:42, 40:43] = True  # 6 pixels: not more than minimum_n_point = 8
    for ds in synth:
        ds.dets[ds.det_keys[0]][0]["segmentation"] = P.rle_encode(tiny)
    assert _both(synth, 0, 2)["inst_ids"].tolist() == [1]
    for ds in synth:  # and the image's only detection: nothing qualifies, on either path
        ds.dets[ds.det_keys[1]][0]["segmentation"] = P.rle_encode(tiny)
    assert "no qulified instance" in _both(synth, 1, 3)


def test_image_without_candidates_stops_after_the_decode(synth, monkeypatch):
    from unopose_amd.ops import prep, rle

    masked = synth[1]
    calls = []
    real = rle.call
    monkeypatch.setattr(rle, "call", lambda *a: (calls.append(a[0]), real(*a))[1])
    monkeypatch.setattr(prep, "call", lambda *a: calls.append(a[0]))
    masked.minimum_n_point = 10 ** 6
    np.random.seed(4)
    before = np.random.get_state()
    with pytest.raises(ValueError, match="no qulified instance in 000048_000001"):
        masked[0]
    assert states_equal(np.random.get_state(), before)
    assert calls == ["unopose_rle_parse", "unopose_rle_fill"] * 2  # the score pass and the best-detection pass: decode and stats only
    assert masked._device_image[1] is None  # the colour image was not uploaded


@torch.no_grad()
def test_cli_device_masks_writes_the_same_lines(tmp_path):
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

    want = run("--device-prep")
    got = run("--device-prep", "--device-masks")
    assert len(want) >= 3 and got == want


def test_coco_gt_on_the_device_equals_the_host_route(tmp_path):
    import gt_info_case
    from unopose_amd import coco_gt, gt_info

    root = str(tmp_path / "bop")
    bop_scenes.build(root, n_images=1, dets_per_image=(1, 1))
    _, sid = gt_info_case.extend_bop_scenes(root)
    gt_info.write_gt_info(root, "lm", "test", scene_ids=[sid], overwrite=True)  # bop_scenes wrote a mask_visib of its own
    path = coco_gt.coco_path(root, "lm", "test", sid)
    base = ["--data-dir", root, "--dataset", "lm", "--split", "test", "--scene-ids", str(sid)]
    assert coco_gt.main(base + ["--host"]) == 0
    with open(path) as f:
        host = json.load(f)
    assert len(host["images"]) == bop_scenes.N_OBJ and len(host["annotations"]) >= len(host["images"]) and len(host["categories"]) == bop_scenes.N_OBJ
    assert [a["id"] for a in host["annotations"]] == list(range(1, len(host["annotations"]) + 1))
    for flags in ([], ["--compute"]):
        assert coco_gt.main(base + ["--check", *flags]) == 0, flags  # the stored file equals what this route computes
    assert coco_gt.main(base + ["--bbox-type", "modal"]) == 0
    assert coco_gt.main(base + ["--bbox-type", "modal", "--check", "--host"]) == 0
    # a chunk budget of two masks: the same lists from many small launches
    masks = np.stack([P.read_image(os.path.join(root, "lm", "test", f"{sid:06d}", "mask_visib", f"{i:06d}_000000.png")) > 0 for i in range(1, 6)])
    hc, ha, hb = coco_gt.encode_host(masks)
    for c, a, b in (coco_gt.encode_masks(masks, "cuda"), coco_gt.encode_masks(masks, "cuda", chunk_bytes=2 * masks[0].size)):
        assert [x.tolist() for x in c] == [x.tolist() for x in hc] and a.tolist() == ha.tolist() and b == hb
