"""CPU: `python -m unopose_amd.coco_gt --host` against tests/golden/coco_gt.json (the toolkit's calc_gt_coco.py loop body and
pycoco_utils on the ground truths of tests/gt_info_case.py), its --check / --force / argument rules, and the host packer of the
run-length decoder.  Everything is integers and strings: held to equality, apart from the three fields that hold the time of writing."""
import io
import json
import os.path as osp

import numpy as np
import pytest

import coco_gt_case
from unopose_amd import coco_gt
from unopose_amd import provider as P


def _args(root, name, split, *more):
    return ["--data-dir", root, "--dataset", name, "--split", split, "--host", *more]


@pytest.fixture()
def folder(tmp_path):
    fx, name, split = coco_gt_case.build(str(tmp_path))
    return str(tmp_path), fx, name, split


@pytest.mark.parametrize("bbox_type", ["amodal", "modal"])
def test_host_output_equals_the_toolkits(folder, bbox_type, capsys):
    root, fx, name, split = folder
    assert coco_gt.main(_args(root, name, split, "--bbox-type", bbox_type)) == 0
    for sid, want in fx["coco"][bbox_type].items():
        path = coco_gt.coco_path(root, name, split, int(sid), bbox_type)
        assert osp.basename(path) == ("scene_gt_coco.json" if bbox_type == "amodal" else "scene_gt_coco_modal.json")
        with open(path) as f:
            got = json.load(f)
        assert set(got) == set(want) and set(got["info"]) == set(want["info"])
        assert [set(im) for im in got["images"]] == [set(im) for im in want["images"]]
        assert [set(a) for a in got["annotations"]] == [set(a) for a in want["annotations"]]
        assert coco_gt.without_clock(got) == coco_gt.without_clock(want)
        assert coco_gt.differences(want, got) == []
    # the fixture's situations, as the generator asserted them
    anns = [a for sid in fx["coco"]["amodal"] for a in fx["coco"]["amodal"][sid]["annotations"]]
    assert any(a["ignore"] for a in anns) and any(a["segmentation"]["counts"][0] == 0 for a in anns)
    assert len(fx["coco"]["amodal"]["1"]["annotations"]) < sum(len(v) for v in fx["scene_gt"]["1"].values())


def test_check_passes_on_its_own_output_and_fails_on_an_altered_count(folder, capsys):
    root, fx, name, split = folder
    assert coco_gt.main(_args(root, name, split)) == 0
    before = {sid: open(coco_gt.coco_path(root, name, split, int(sid))).read() for sid in fx["scene_gt"]}
    assert coco_gt.main(_args(root, name, split, "--check")) == 0
    assert "equal" in capsys.readouterr().out
    path = coco_gt.coco_path(root, name, split, 1)
    coco = json.loads(before["1"])
    counts = coco["annotations"][2]["segmentation"]["counts"]
    counts[1], counts[2] = counts[1] + 1, counts[2] - 1  # one pixel moved from one run to the next
    with open(path, "w") as f:
        json.dump(coco, f)
    altered = open(path).read()
    assert coco_gt.main(_args(root, name, split, "--check")) == 1
    out = capsys.readouterr().out
    assert "DIFFERENT" in out and "annotation 3 (image 1): segmentation differ" in out
    assert open(path).read() == altered  # --check writes nothing
    assert open(coco_gt.coco_path(root, name, split, 2)).read() == before["2"]
    lines = coco_gt.write_coco_gt(root, name, split, device=None, check=True, out=io.StringIO())
    assert lines[2] == [] and len(lines[1]) == 1


def test_force_and_argument_errors(folder):
    root, fx, name, split = folder
    with pytest.raises(FileNotFoundError, match="nothing to check"):
        coco_gt.main(_args(root, name, split, "--check"))
    assert coco_gt.main(_args(root, name, split, "--scene-ids", "2")) == 0
    assert osp.exists(coco_gt.coco_path(root, name, split, 2)) and not osp.exists(coco_gt.coco_path(root, name, split, 1))
    with pytest.raises(FileExistsError, match="--force"):
        coco_gt.main(_args(root, name, split))
    assert not osp.exists(coco_gt.coco_path(root, name, split, 1))  # refused before anything was written
    path = coco_gt.coco_path(root, name, split, 2)
    with open(path, "w") as f:
        f.write("{}")
    assert coco_gt.main(_args(root, name, split, "--force")) == 0
    with open(path) as f:
        assert coco_gt.without_clock(json.load(f)) == coco_gt.without_clock(fx["coco"]["amodal"]["2"])
    assert coco_gt.main(_args(root, name, split, "--bbox-type", "modal")) == 0  # the modal file is another file
    with pytest.raises(SystemExit):
        coco_gt.main(_args(root, name, split, "--bbox-type", "polygon"))
    with pytest.raises(SystemExit):
        coco_gt.main(["--dataset", name, "--split", split])
    with pytest.raises(ValueError, match="not a valid bounding box type"):
        coco_gt.write_coco_gt(root, name, split, bbox_type="tight", device=None)
    with pytest.raises(FileNotFoundError):
        coco_gt.main(_args(root, name, "train"))


def test_host_encoder_matches_the_toolkits_recorded_lists():
    fx = coco_gt_case.fixture()
    assert len(fx["decoded"]) == 7
    masks = np.stack([np.array([[c == "1" for c in row] for row in e["rows"]]) for e in fx["decoded"]])
    counts, area, bbox = coco_gt.encode_host(masks)
    anns = [a for sid in fx["coco"]["modal"] for a in fx["coco"]["modal"][sid]["annotations"]]
    for e, c, n, b, a, m in zip(fx["decoded"], counts, area, bbox, anns, masks):
        assert c.tolist() == e["counts"] and int(n) == a["area"] and b == a["bbox"]
        assert np.array_equal(P.rle_decode(dict(size=e["size"], counts=e["counts"])), m)  # the toolkit's rle_to_binary_mask
    assert coco_gt.encode_host(np.zeros((1, 3, 4), bool))[2] == [None]


def test_packer_rejects_bad_bytes_and_mixed_sizes():
    from unopose_amd.ops.rle import pack_segs

    rs = np.random.RandomState(0)
    mask = rs.rand(7, 5) < 0.4
    lst = P.rle_encode(mask)
    text = dict(size=lst["size"], counts=P.rle_counts_to_string(lst["counts"]))
    H, W, desc, buf, ints, n_starts = pack_segs([lst, text, dict(size=[7, 5], counts=text["counts"].encode())])
    n = len(lst["counts"])
    assert (H, W) == (7, 5) and desc.dtype == np.int32 and buf.dtype == np.uint8 and ints.dtype == np.int32
    assert desc[:, 0].tolist() == [0, 1, 1] and desc[:, 3].tolist() == [n, n, n] and desc[:, 4].tolist() == [0, n + 1, 2 * n + 2]
    assert n_starts == 3 * (n + 1) and ints.tolist() == lst["counts"] and bytes(buf) == 2 * text["counts"].encode()
    assert desc[:, 1].tolist() == [0, 0, len(text["counts"])] and desc[:, 2].tolist() == [n, len(text["counts"]), len(text["counts"])]
    for bad in ("/", "p", "\x7f", " ", "é"):
        with pytest.raises(ValueError, match="mask 1"):
            pack_segs([lst, dict(size=[7, 5], counts=text["counts"][:3] + bad + text["counts"][3:])])
    with pytest.raises(ValueError, match="mask 2.*ends inside a number"):
        pack_segs([lst, text, dict(size=[7, 5], counts=text["counts"] + "P")])  # 'P' - 48 = 0x20: a continuation without end
    with pytest.raises(ValueError, match="different sizes"):
        pack_segs([lst, dict(size=[5, 7], counts=lst["counts"])])
    with pytest.raises(ValueError):
        pack_segs([])
    with pytest.raises(ValueError, match="mask size"):
        pack_segs([dict(size=[0, 5], counts=[])])
    # an empty string and an empty list are masks without runs
    assert pack_segs([dict(size=[2, 2], counts=""), dict(size=[2, 2], counts=[])])[2][:, 3].tolist() == [0, 0]
