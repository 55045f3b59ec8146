"""CPU: the numpy statement of the proposal-matching rule (unopose_amd/match_dets.py) on hand-made cases, and the file it writes read back
by the provider.  The ViT is replaced by an injected token function, so nothing here needs a GPU."""
import io
import json
import os

import numpy as np
import pytest

import match_dets_case as C
from unopose_amd import match_dets as M
from unopose_amd.provider import BOPTestsetOneRef, rle_decode


@pytest.mark.parametrize("img_size", [56, 70])
@pytest.mark.parametrize("s", [2, 14, 15, 56])
def test_patch_validity_equals_the_pixel_loop(s, img_size):
    for mask in C.validity_masks(s, img_size):
        got = M.patch_valid_host(mask, img_size)
        assert got.dtype == np.uint8 and got.shape == ((img_size // 14) ** 2,)
        assert np.array_equal(got, C.brute_patch_valid(mask, img_size))
    assert not M.patch_valid_host(np.zeros((s, s), bool), img_size).any()
    assert M.patch_valid_host(np.ones((s, s), bool), img_size).all()


def test_patch_validity_boundary_is_half_of_the_patch():
    masks = C.validity_masks(56, 56)
    v = M.patch_valid_host(masks[-1], 56).reshape(4, 4)
    assert v[0, 0] == 1 and v[1, 1] == 0 and v.sum() == 1  # 98 of 196 pixels is valid, 97 is not


def _score(q_rows, q_valid, r_rows, r_valid):
    s_sem, s_appe = M.scores_host(C.one_hot_tokens(q_rows)[None], np.array([q_valid]), C.one_hot_tokens(r_rows)[None], np.array([r_valid]))
    return float(s_sem[0, 0]), float(s_appe[0, 0])


def test_scores_on_hand_made_tokens():
    pre = [0, 30, 30, 30, 30]  # class token e0, registers
    assert _score(pre + [1, 2, 3], [1, 1, 1], pre + [3, 1, 2], [1, 1, 1]) == (1.0, 1.0)  # identical sets, any order
    assert _score(pre + [1, 2, 3], [1, 1, 1], [9, 30, 30, 30, 30] + [4, 5, 6], [1, 1, 1]) == (0.0, 0.0)  # mutually orthogonal
    assert _score(pre + [1, 2, 3], [0, 1, 0], pre + [2, 7, 8], [1, 1, 1]) == (1.0, 1.0)  # one valid patch, and it has a partner
    assert _score(pre + [1, 2, 3], [0, 1, 0], pre + [2, 7, 8], [0, 1, 1]) == (1.0, 0.0)  # ... whose partner is masked
    assert _score(pre + [1, 2, 3], [1, 1, 0], pre + [1, 7, 8], [1, 1, 1]) == (1.0, 0.5)  # mean over the valid rows of the row maxima
    assert _score(pre + [1, 2, 3], [0, 0, 0], pre + [1, 2, 3], [1, 1, 1])[1] == 0.0  # no valid patch on the query
    assert _score(pre + [1, 2, 3], [1, 1, 1], pre + [1, 2, 3], [0, 0, 0])[1] == 0.0  # ... on the reference
    assert _score([-1, 30, 30, 30, 30] + [1, -1, 3], [1, 1, 1], pre + [1, 2, 3], [1, 1, 1]) == (0.0, 2.0 / 3.0)  # zero-norm rows give zeros
    u = M.unit_rows_host(np.array([[3.0, 4.0], [0.0, 0.0], [1e4, 0.0]], dtype=np.float32))
    assert np.array_equal(u[1], [0.0, 0.0]) and np.array_equal(u[2], [1.0, 0.0])
    assert np.allclose(u[0], [0.6, 0.8], rtol=2.0 ** -8, atol=0) and np.array_equal(M.round_bf16(u[0].astype(np.float32)), u[0].astype(np.float32))


def test_combined_score_is_a_clipped_weighted_mean():
    s = M.combine_scores(np.array([[-1.0, 0.5, 1.0]]), np.array([[0.0, 0.25, 1.0]]), (1, 1))
    assert np.array_equal(s, [[0.0, 0.375, 1.0]])
    assert np.array_equal(M.combine_scores([[0.5]], [[0.25]], (3, 1)), [[0.4375]])
    with pytest.raises(ValueError):
        M.check_rule_arguments(224, (0, 0), 0.5, 0, 8)


def test_label_ties_go_to_the_smaller_object_id():
    score = np.array([[0.5, 0.5, 0.1], [0.2, 0.7, 0.7], [0.9, 0.1, 0.9]])
    cat, best = M.label_host(score, [5, 2, 9])  # columns are objects 5, 2, 9
    assert cat.tolist() == [2, 2, 5] and best.tolist() == [0.5, 0.7, 0.9]


def _strip(*spans, n=12):
    m = np.zeros((len(spans), 1, n), bool)
    for i, (a, b) in enumerate(spans):
        m[i, 0, a:b] = True
    return m


def test_suppression_thresholds_order_and_cap():
    at, above, below = _strip((0, 3), (1, 4)), _strip((0, 4), (1, 5)), _strip((0, 2), (1, 3))  # inter / union = 2/4, 3/5, 1/3
    cat, score = np.zeros(2, int), np.array([0.9, 0.8])
    assert M.nms_host(at, cat, score, 0.5)[0].tolist() == [1, 1]  # exactly at the threshold is not above it
    keep, area, inter = M.nms_host(above, cat, score, 0.5)
    assert keep.tolist() == [1, 0] and area.tolist() == [4, 4] and inter.tolist() == [[4, 3], [3, 4]]
    assert M.nms_host(below, cat, score, 0.5)[0].tolist() == [1, 1]
    assert M.nms_host(above, cat, score[::-1], 0.5)[0].tolist() == [0, 1]  # the better one stays
    assert M.nms_host(above, cat, np.array([0.8, 0.8]), 0.5)[0].tolist() == [1, 0]  # equal scores: the smaller number first
    assert M.nms_host(above, np.array([1, 2]), score, 0.5)[0].tolist() == [1, 1]  # other categories do not suppress
    far = _strip((0, 2), (3, 5), (6, 8), (9, 11))
    keep = M.nms_host(far, np.array([1, 1, 2, 1]), np.array([0.5, 0.9, 0.1, 0.7]), 0.5, max_per_object=2)[0]
    assert keep.tolist() == [0, 1, 1, 1]  # the two best of category 1, the only one of category 2
    assert M.nms_host(np.zeros((2, 3, 3), bool), cat, score, 0.5)[0].tolist() == [1, 1]  # empty masks: 0 > 0 is false


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("match_dets"))
    cfg, path, props = C.build(root)
    log = io.StringIO()
    matcher = M.Matcher(root, "ycbv", cfg["ref_targets_name"], C.fake_tokens, img_size=cfg["img_size"], min_points=cfg["minimum_n_point"], out=log)
    entries, records = matcher.run(props)
    out = os.path.join(root, "matched.json")
    M.save_detections(out, entries)
    return dict(root=root, cfg=cfg, props=props, entries=entries, records=records, out=out, log=log.getvalue(), matcher=matcher)


def test_written_file_is_read_by_the_provider(written):
    entries = json.load(open(written["out"]))
    assert entries == json.loads(json.dumps(written["entries"])) and len(entries) >= 3
    assert not [f for f in os.listdir(written["root"]) if ".tmp" in f]
    keys = [(e["scene_id"], e["image_id"]) for e in entries]
    assert keys == sorted(keys) and set(keys) == {(48, 1), (48, 2), (48, C.SELF_IMAGE)}
    for e in entries:
        assert set(e) == {"scene_id", "image_id", "category_id", "score", "bbox", "time", "segmentation"}
        assert e["category_id"] in ((2, 5) if e["image_id"] == 1 else (2,)) and 0.0 <= e["score"] <= 1.0
        assert e["segmentation"] in [p["segmentation"] for p in written["props"]]
        prop = next(p for p in written["props"] if p["segmentation"] == e["segmentation"] and p["image_id"] == e["image_id"])
        ys, xs = np.nonzero(rle_decode(prop["segmentation"]))
        assert e["bbox"] == prop.get("bbox", [int(xs.min()), int(ys.min()), int(np.ptp(xs)) + 1, int(np.ptp(ys)) + 1])  # its own box, else the mask's
        assert e["time"] == prop.get("time", -1)
    rec = written["records"][(48, 1)]
    assert rec["slots"] == [0, 1, 2, 3, 4] and rec["obj_ids"] == [2, 5]  # the speck was dropped before scoring
    assert any(e["bbox"] in ([1, 2, 3, 4], [5, 6, 7, 8]) for e in entries)  # a proposal's own box went through unchanged
    mine = [e for e in entries if e["image_id"] == C.SELF_IMAGE]
    assert len(mine) == 1 and mine[0]["time"] == -1 and mine[0]["category_id"] == 2 and mine[0]["score"] > 0.999
    c = written["matcher"].counts
    assert c["proposals"] == 10 and c["dropped"] == 1 and c["skipped_images"] == 1 and c["references"] == 3
    assert "scene 48 image 9" in written["log"] and "no targeted object" in written["log"]
    np.random.seed(0)
    ds = BOPTestsetOneRef(dict(written["cfg"], seg_filter_score=-1.0), "ycbv", written["out"])
    item = ds[0]
    assert item["rgb"].shape[1:] == (3, 56, 56) and len(item["rgb"]) >= 1 and int(item["scene_id"]) == 48


def test_check_leaves_the_file_untouched_and_agrees_with_itself(written):
    before, stamp = open(written["out"], "rb").read(), os.stat(written["out"]).st_mtime_ns
    log = io.StringIO()
    cfg = written["cfg"]
    matcher = M.Matcher(written["root"], "ycbv", cfg["ref_targets_name"], C.fake_tokens, img_size=cfg["img_size"], min_points=cfg["minimum_n_point"], out=log)
    assert M.check_detections(matcher, json.load(open(written["out"])), out=log) == 0
    assert "labelled differently, largest score difference 0.000000" in log.getvalue()
    assert open(written["out"], "rb").read() == before and os.stat(written["out"]).st_mtime_ns == stamp


def test_argument_errors_come_before_any_gpu_work(written, monkeypatch):
    import torch

    def no_gpu(*a, **k):
        raise AssertionError("the GPU was asked for before the arguments were checked")

    monkeypatch.setattr(torch.cuda, "is_available", no_gpu)
    base = ["--data-dir", written["root"], "--dataset", "ycbv", "--ref-targets", written["cfg"]["ref_targets_name"]]
    ckpt = os.path.join(written["root"], "vit.pth")
    open(ckpt, "wb").close()
    io_args = ["--proposals", os.path.join(written["root"], "proposals.json"), "--out", os.path.join(written["root"], "new.json")]
    for bad in (base + io_args,  # neither checkpoint
                base + io_args + ["--vit-ckpt", ckpt, "--checkpoint", ckpt],
                base + ["--vit-ckpt", ckpt],  # nothing to do
                base + io_args + ["--vit-ckpt", ckpt, "--img-size", "60"],
                base + io_args + ["--vit-ckpt", ckpt, "--weights", "0", "0"],
                base + io_args + ["--vit-ckpt", ckpt, "--nms-iou", "1.5"],
                base + io_args + ["--vit-ckpt", ckpt, "--max-per-object", "-1"]):
        with pytest.raises(SystemExit):
            M.main(bad)
    with pytest.raises(FileNotFoundError):
        M.main(base + io_args + ["--vit-ckpt", ckpt + ".missing"])
    with pytest.raises(FileExistsError):
        M.main(base + ["--proposals", io_args[1], "--out", written["out"], "--vit-ckpt", ckpt])
    with pytest.raises(RuntimeError, match="CPU"):
        M.Matcher(written["root"], "ycbv", written["cfg"]["ref_targets_name"], C.fake_tokens, img_size=56, device="cpu")
    assert not os.path.exists(io_args[3])
