"""CPU: the ground-truth visibility on the host -- `gt_info.gt_info_host` and the host route of `compute_gt_info` against the toolkit's own
functions on tests/gt_info_case.py (tests/golden/gt_info.json, gt_info_masks.npz), the scorer's validity rule against the toolkit's recalls,
the files `write_gt_info` writes, the plan the CLI prints and the error for a missing scene_gt_info.json."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import gt_info_case as C
from raster_np import NumpyRenderer
from unopose_amd import bop_eval, gt_info

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def case():
    want = json.load(open(os.path.join(GOLD, "gt_info.json")))
    W, H = want["size"]
    models = C.make_models()
    ren = NumpyRenderer(3 * W, 3 * H)
    for obj_id, m in models.items():
        ren.add_object(obj_id, m["verts"], m["faces"])
    scene_gt, cameras, depth_images, canvases = C.make_scenes(lambda *a: ren.render_object(*a)["depth"], W, H)
    return dict(want=want, masks=np.load(os.path.join(GOLD, "gt_info_masks.npz")), models=models, ren=ren, scene_gt=scene_gt, cameras=cameras,
                depth_images=depth_images, canvases=canvases)


def test_gt_info_host_equals_the_toolkit(case):
    assert len(case["canvases"]) == sum(len(v) for v in case["want"]["gt_info"].values()) == 10
    for (sid, iid, gid), canvas in case["canvases"].items():
        info, mask, visib = gt_info.gt_info_host(case["depth_images"][sid][iid], canvas, case["cameras"][sid][iid], C.DELTA)
        assert info == case["want"]["gt_info"][f"{sid}/{iid}"][gid], (sid, iid, gid)  # the integers and visib_fract exactly
        assert mask.dtype == bool and np.array_equal(mask, case["masks"][f"mask_{sid}_{iid}_{gid}"])
        assert visib.dtype == bool and np.array_equal(visib, case["masks"][f"visib_{sid}_{iid}_{gid}"])
    # the raw row: extrema of an empty set, image coordinates of the canvas
    row, _, _ = gt_info.gt_counts_host(case["depth_images"][1][0], case["canvases"][(1, 0, 3)], case["cameras"][1][0], C.DELTA)
    assert row == [0, 0, 0] + [gt_info.INT_MAX, gt_info.INT_MAX, gt_info.INT_MIN, gt_info.INT_MIN] * 2
    row, _, _ = gt_info.gt_counts_host(case["depth_images"][1][0], case["canvases"][(1, 0, 2)], case["cameras"][1][0], C.DELTA)
    assert row[0] > 0 and row[2] == 0 and row[5] < 0 and row[7:] == [gt_info.INT_MAX, gt_info.INT_MAX, gt_info.INT_MIN, gt_info.INT_MIN]
    with pytest.raises(ValueError, match="canvas"):
        gt_info.gt_info_host(case["depth_images"][1][0], case["canvases"][(1, 0, 0)][1:], case["cameras"][1][0], C.DELTA)


def test_compute_gt_info_on_the_host_equals_the_toolkit(case):
    out = gt_info.compute_gt_info(case["scene_gt"], case["cameras"], case["depth_images"], case["ren"], C.DELTA)
    assert {f"{sid}/{iid}": v for sid, ims in out.items() for iid, v in ims.items()} == case["want"]["gt_info"]
    out2, held = gt_info.compute_gt_info(case["scene_gt"], case["cameras"], case["depth_images"], case["ren"], C.DELTA, masks=True)
    assert out2 == out
    for (sid, iid, gid) in case["canvases"]:
        m, mv = held[sid][iid][gid]
        assert np.array_equal(m, case["masks"][f"mask_{sid}_{iid}_{gid}"]) and np.array_equal(mv, case["masks"][f"visib_{sid}_{iid}_{gid}"])
    with pytest.raises(RuntimeError):  # the device route is never entered on a CPU device, and never with another renderer
        gt_info.compute_gt_info(case["scene_gt"], case["cameras"], case["depth_images"], case["ren"], C.DELTA, device="cpu")
    small = NumpyRenderer(36, 24)
    small.models = case["ren"].models
    with pytest.raises(RuntimeError, match="renderer draws"):
        gt_info.compute_gt_info(case["scene_gt"], case["cameras"], case["depth_images"], small, C.DELTA)


def _gt_info_of(case):
    return {int(k.split("/")[0]): {int(kk.split("/")[1]): v for kk, v in case["want"]["gt_info"].items() if kk.split("/")[0] == k.split("/")[0]}
            for k in case["want"]["gt_info"]}


def test_average_recall_follows_the_toolkits_validity_rule(case):
    cases = C.recall_cases(case["scene_gt"], case["cameras"], _gt_info_of(case))
    assert sorted(cases) == sorted(case["want"]["recalls"])
    for name, c in cases.items():
        a = (c["results"], c["scene_gt"], case["models"], c["cameras"], 640.0)
        out = bop_eval.average_recall(*a, n_top=-1, targets=c["targets"], gt_info=c["gt_info"], visib_gt_min=c["visib_gt_min"])
        assert out["recalls_mssd"] == case["want"]["recalls"][name], name
        walk = bop_eval._walk(c["results"], c["scene_gt"], c["cameras"], -1, c["targets"], c["gt_info"], c["visib_gt_min"])
        assert {f"{sid}/{iid}": [g["valid"] for g in gts] for sid, iid, gts, _, _ in walk} == case["want"]["valid"][name], name
        # the further error types see the same flags
        more = bop_eval.average_recall(*a, n_top=-1, targets=c["targets"], gt_info=c["gt_info"], visib_gt_min=c["visib_gt_min"], error_types="mssd,te")
        assert more["errors"]["mssd"]["recalls"] == case["want"]["recalls"][name]
    c = cases["issue"]
    a = (c["results"], c["scene_gt"], case["models"], c["cameras"], 640.0)
    assert bop_eval.average_recall(*a, n_top=-1, targets=c["targets"], gt_info=c["gt_info"])["AR_MSSD"] == 0.0
    assert bop_eval.average_recall(*a, n_top=-1, targets=c["targets"])["AR_MSSD"] == 0.5  # without gt_info: today's rule, two targets
    # the tie: two equally visible instances, the first in ground-truth order counts
    assert case["want"]["valid"]["scenes_k1"]["2/0"] == [True, False, False]
    assert cases["scenes_k1"]["gt_info"][2][0][0]["visib_fract"] == cases["scenes_k1"]["gt_info"][2][0][2]["visib_fract"]
    # the rule differs from "every ground truth of a target counts" on these scenes
    c = cases["scenes_k1"]
    a = (c["results"], c["scene_gt"], case["models"], c["cameras"], 640.0)
    assert bop_eval.average_recall(*a, n_top=-1, targets=c["targets"])["recalls_mssd"] != case["want"]["recalls"]["scenes_k1"]
    with pytest.raises(ValueError, match="inst_count"):
        bop_eval.average_recall(*a, n_top=-1, gt_info=c["gt_info"])
    with pytest.raises(ValueError, match="gt_info of image"):
        bop_eval.average_recall(*a, n_top=-1, targets=c["targets"], gt_info={1: {0: []}})
    # an "valid" key of the caller's still switches a ground truth off
    off = {sid: {iid: [dict(g, valid=False) for g in gts] for iid, gts in ims.items()} for sid, ims in c["scene_gt"].items()}
    assert bop_eval.average_recall(c["results"], off, case["models"], c["cameras"], 640.0, n_top=-1, targets=c["targets"], gt_info=c["gt_info"])["AR_MSSD"] == 0.0


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    import bop_scenes

    root = str(tmp_path_factory.mktemp("bop"))
    bop_scenes.build(root, n_images=1, dets_per_image=(1, 1))
    csv, sid = C.extend_bop_scenes(root)
    ren = NumpyRenderer(3 * bop_scenes.W, 3 * bop_scenes.H)
    with pytest.raises(FileExistsError, match="mask_visib"):  # bop_scenes wrote masks of its own
        gt_info.write_gt_info(root, "lm", "test", scene_ids=[sid], device=None, renderer=ren)
    stale = os.path.join(root, "lm", "test", f"{sid:06d}", "mask_visib", "000001_000007.png")  # of a ground truth scene_gt.json does not list
    open(stale, "wb").write(b"left by another tool")
    out = gt_info.write_gt_info(root, "lm", "test", scene_ids=[sid], device=None, renderer=ren, overwrite=True)
    return root, csv, sid, out, ren


def test_write_gt_info_round_trips_through_load_dataset(written):
    from PIL import Image

    import bop_scenes

    root, csv, sid, out, ren = written
    folder = os.path.join(root, "lm", "test", f"{sid:06d}")
    gt = json.load(open(os.path.join(folder, "scene_gt.json")))
    stored = json.load(open(os.path.join(folder, "scene_gt_info.json")))
    assert sorted(stored) == sorted(gt) and all(len(stored[k]) == len(gt[k]) for k in gt)  # every image, string keys
    assert all(sorted(e) == sorted(gt_info.INFO_KEYS) for v in stored.values() for e in v)
    data = bop_eval.load_dataset(root, "lm", "test", gt_info=True)
    assert data["gt_info"] == {sid: {int(k): v for k, v in stored.items()}} == json.loads(json.dumps(out), object_hook=lambda d: {(int(k) if k.isdigit() else k): v for k, v in d.items()})
    assert "gt_info" not in bop_eval.load_dataset(root, "lm", "test")
    fracts = [e["visib_fract"] for v in stored.values() for e in v]
    assert max(fracts) <= 1.0 and min(fracts) < 0.999 and sum(len(v) for v in stored.values()) == bop_scenes.N_OBJ + (bop_scenes.N_OBJ + 1) // 2
    for iid, entries in stored.items():
        for gid, e in enumerate(entries):
            m = np.array(Image.open(os.path.join(folder, "mask", f"{int(iid):06d}_{gid:06d}.png")))
            mv = np.array(Image.open(os.path.join(folder, "mask_visib", f"{int(iid):06d}_{gid:06d}.png")))
            assert m.dtype == np.uint8 and m.shape == (bop_scenes.H, bop_scenes.W) and set(np.unique(m)) <= {0, 255} and set(np.unique(mv)) <= {0, 255}
            assert (mv > 0).sum() == e["px_count_visib"] and ((mv > 0) <= (m > 0)).all() and (m > 0).sum() <= e["px_count_all"]
    assert sorted(os.listdir(os.path.join(folder, "mask_visib"))) == sorted(os.listdir(os.path.join(folder, "mask"))) == \
        sorted(f"{int(iid):06d}_{gid:06d}.png" for iid, entries in stored.items() for gid in range(len(entries)))  # overwrite left no stale mask
    # a second run refuses, --no-masks writes the json alone
    with pytest.raises(FileExistsError, match="scene_gt_info.json"):
        gt_info.write_gt_info(root, "lm", "test", scene_ids=[sid], masks=False, device=None, renderer=ren)


def test_score_csv_reads_or_computes_the_visibility(written):
    root, csv, sid, out, ren = written
    import bop_scenes

    small = NumpyRenderer(bop_scenes.W, bop_scenes.H)
    off = bop_eval.score_csv(csv, root, "lm", "test", device_scoring=False, renderer=small, error_types="mssd,mspd")
    assert "gt_visibility" not in off and "visib_gt_min" not in off
    on = bop_eval.score_csv(csv, root, "lm", "test", device_scoring=False, renderer=small, error_types="mssd,mspd", gt_visibility="file")
    assert on["gt_visibility"] == "file" and on["visib_gt_min"] == -1 and sorted(set(on) - set(off)) == ["gt_visibility", "visib_gt_min"]
    assert json.load(open(os.path.join(os.path.dirname(csv), "scores_bop19.json")))["gt_visibility"] == "file"
    # the nearer instance is the more visible one and the only valid one; the better estimate sits on the farther instance
    assert on["AR_MSSD"] != off["AR_MSSD"]
    least = bop_eval.score_csv(csv, root, "lm", "test", device_scoring=False, renderer=small, error_types="mssd,mspd", gt_visibility="file", visib_gt_min=0.0)
    assert least["visib_gt_min"] == 0.0 and least["recalls_mssd"] == off["recalls_mssd"]  # every target visible to >= 0: today's rule
    with pytest.raises(ValueError, match="gt_visibility"):
        bop_eval.score_csv(csv, root, "lm", "test", device_scoring=False, renderer=small, gt_visibility="on")
    with pytest.raises(ValueError, match="visib_gt_min has no effect"):  # an option that would be ignored is refused
        bop_eval.score_csv(csv, root, "lm", "test", device_scoring=False, renderer=small, visib_gt_min=0.1)
    with pytest.raises(ValueError, match="gt_delta"):
        bop_eval.score_csv(csv, root, "lm", "test", device_scoring=False, renderer=small, gt_visibility="file", gt_delta=5.0)


def test_a_missing_gt_info_file_is_an_error_that_names_it(tmp_path):
    import bop_score_case
    from bop_eval_case import make_vsd_case

    root, case = str(tmp_path), make_vsd_case()
    csv, _ = bop_score_case.write_dataset(root, case)
    path = os.path.join(root, "synth", "test", "000003", "scene_gt_info.json")
    for call in (lambda: bop_eval.load_dataset(root, "synth", "test", gt_info=True),
                 lambda: bop_eval.score_csv(csv, root, "synth", "test", device_scoring=False, renderer=NumpyRenderer(*case[6]), gt_visibility="file")):
        with pytest.raises(FileNotFoundError) as e:
            call()
        assert path in str(e.value) and "compute" in str(e.value)
    assert not os.path.exists(os.path.join(os.path.dirname(csv), "scores_bop19.json"))  # no fallback to the rule without visibility


BASE = dict(model=dict(cfg=dict(coarse_npoint=196)),
            dataloader=dict(test=dict(dataset=dict(eval_dataset_name="tless", detetion_path="d.json", cfg=dict(img_size=224, data_dir="/data/bop")))),
            test=dict(amp=dict(enabled=False), instance_batch_size=16), misc=dict(output_dir="output/unopose", load_from="/x/ckpt_12.pth"),
            bop_eval=dict(split="test"))


def _plan(tmp_path, capsys, *extra):
    """`cli.main(--print-plan)` in this process: it touches no GPU and imports no torch."""
    from unopose_amd import cli

    cfgf = tmp_path / "c.json"
    cfgf.write_text(json.dumps(BASE))
    assert cli.main(["--config-file", str(cfgf), "--print-plan", *extra]) == 0
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def test_print_plan_names_the_visibility_options_only_when_set(tmp_path, capsys):
    plain = _plan(tmp_path, capsys, "--eval")
    assert "eval_gt_visibility" not in plain and "eval_visib_gt_min" not in plain
    both = _plan(tmp_path, capsys, "--eval", "bop_eval.gt_visibility=compute", "bop_eval.visib_gt_min=0.1")
    assert both["eval_gt_visibility"] == "compute" and both["eval_visib_gt_min"] == 0.1
    assert {k: v for k, v in both.items() if k not in ("eval_gt_visibility", "eval_visib_gt_min")} == plain
    one = _plan(tmp_path, capsys, "--eval", "bop_eval.gt_visibility=file")
    assert one["eval_gt_visibility"] == "file" and "eval_visib_gt_min" not in one
    with pytest.raises(ValueError, match="gt_visibility"):
        _plan(tmp_path, capsys, "--eval", "bop_eval.gt_visibility=yes")
    assert "eval_gt_visibility" not in _plan(tmp_path, capsys, "bop_eval.gt_visibility=file")  # without --eval nothing is scored
    tol = _plan(tmp_path, capsys, "--eval", "bop_eval.gt_visibility=compute", "bop_eval.gt_delta=5")
    assert tol["eval_gt_delta"] == 5.0 and "eval_gt_delta" not in both
    for bad in (["bop_eval.visib_gt_min=0.1"], ["bop_eval.visib_gt_min=0.1", "bop_eval.gt_visibility=off"], ["bop_eval.gt_delta=5", "bop_eval.gt_visibility=file"]):
        with pytest.raises(ValueError, match="needs bop_eval.gt_visibility|gt_delta is"):  # a key that would have no effect
            _plan(tmp_path, capsys, "--eval", *bad)


def test_the_module_has_a_command_line():
    r = subprocess.run([sys.executable, "-m", "unopose_amd.gt_info", "--help"], capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT), cwd=ROOT)
    assert r.returncode == 0 and all(flag in r.stdout for flag in ("--data-dir", "--dataset", "--split", "--scenes", "--no-masks", "--host", "--overwrite"))
