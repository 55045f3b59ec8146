"""CPU: what `cli --eval` needs around the scorer -- the PLY reader, `bop_eval.load_dataset` on a synthetic BOP folder (models,
symmetries as the toolkit lists them, targets), the targets' effect on what is scored, the plan the CLI prints -- and the host route
of `average_recall`, which must return what it returned before the device route existed (golden values of bop_toolkit_lib)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bop_score_case as C
from bop_eval_case import make_case, make_vsd_case
from unopose_amd import bop_eval

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def test_ply_reader_round_trips_ascii_and_binary(tmp_path):
    m = C._models()[3]
    for binary, vertex_type in ((False, "float"), (True, "float"), (True, "double")):
        p = str(tmp_path / f"m_{binary}_{vertex_type}.ply")
        C.write_ply(p, m["verts"], m["faces"], binary=binary, vertex_type=vertex_type)
        got = bop_eval.read_ply(p)
        assert got["pts"].dtype == np.float64 and got["pts"].shape == m["verts"].shape and got["faces"].dtype == np.int32
        assert np.array_equal(got["faces"], m["faces"])
        if binary and vertex_type == "float":
            assert np.array_equal(got["pts"], m["verts"].astype(np.float32).astype(np.float64))
        else:  # repr() text and float64 records keep every bit
            assert np.array_equal(got["pts"], m["verts"])
    # what the reader does not read is an error, not a guess
    quad = str(tmp_path / "quad.ply")
    open(quad, "w").write("ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\nelement face 1\n"
                          "property list uchar int vertex_indices\nend_header\n0 0 0\n1 0 0\n1 1 0\n0 1 0\n4 0 1 2 3\n")
    with pytest.raises(ValueError):
        bop_eval.read_ply(quad)
    big = str(tmp_path / "big.ply")
    open(big, "w").write("ply\nformat binary_big_endian 1.0\nelement vertex 0\nproperty float x\nproperty float y\nproperty float z\nend_header\n")
    with pytest.raises(ValueError):
        bop_eval.read_ply(big)
    odd = str(tmp_path / "odd.ply")  # a property type the reader does not know
    open(odd, "w").write("ply\nformat ascii 1.0\nelement vertex 1\nproperty half x\nproperty float y\nproperty float z\nend_header\n0 0 0\n")
    with pytest.raises(ValueError):
        bop_eval.read_ply(odd)
    # a byte outside ASCII in a header comment is no obstacle
    p = str(tmp_path / "latin.ply")
    C.write_ply(p, m["verts"], m["faces"], binary=True)
    raw = open(p, "rb").read()
    open(p, "wb").write(raw.replace(b"comment written by", b"comment \xe9crit par", 1))
    assert np.array_equal(bop_eval.read_ply(p)["faces"], m["faces"])


def test_symmetry_transformations_follow_the_toolkit():
    # discrete: identity first, then the listed 4 x 4 matrices
    models = C._models()
    disc = [np.block([[s["R"], s["t"].reshape(3, 1)], [np.zeros((1, 3)), np.ones((1, 1))]]).reshape(-1).tolist() for s in models[3]["symmetries"][1:]]
    syms = bop_eval.symmetry_transformations(dict(diameter=100.0, symmetries_discrete=disc))
    assert len(syms) == 5 and np.array_equal(syms[0]["R"], np.eye(3)) and np.array_equal(syms[0]["t"], np.zeros(3))
    for got, want in zip(syms[1:], models[3]["symmetries"][1:]):
        assert np.allclose(got["R"], want["R"], atol=1e-15) and np.allclose(got["t"], want["t"], atol=1e-12) and got["t"].shape == (3,)
    # continuous: ceil(pi / 0.01) = 315 steps whatever the diameter (misc.py:69-70), the first one the identity; an offset axis translates
    cont = dict(diameter=172.0, symmetries_continuous=[dict(axis=[0, 0, 1], offset=[10.0, 0.0, 0.0])])
    syms = bop_eval.symmetry_transformations(cont)
    assert len(syms) == int(np.ceil(np.pi / 0.01)) == 315
    assert np.allclose(syms[0]["R"], np.eye(3)) and np.allclose(syms[0]["t"], 0)
    step = 2 * np.pi / 315
    assert np.allclose(syms[1]["R"], [[np.cos(step), -np.sin(step), 0], [np.sin(step), np.cos(step), 0], [0, 0, 1]])
    assert np.allclose(syms[1]["t"], np.array([10.0, 0, 0]) - syms[1]["R"] @ np.array([10.0, 0, 0])) and np.abs(syms[1]["t"]).max() > 0.1
    # both: every discrete one combined with every step, discrete-major
    both = bop_eval.symmetry_transformations(dict(cont, symmetries_discrete=disc[:1]))
    assert len(both) == 2 * 315 and np.allclose(both[0]["R"], np.eye(3)) and np.allclose(both[315]["R"], models[3]["symmetries"][1]["R"])


@pytest.fixture(scope="module")
def small_dataset(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("bop"))
    case = make_vsd_case()
    csv, targets = C.write_dataset(root, case, skip_image=(3, 5), skip_object=(4, 0, 5), continuous_object=1)
    return root, case, csv, targets


def test_load_dataset_returns_the_dictionaries_of_the_folder(small_dataset):
    root, (models, scene_gt, cameras, results, _, depth_images, (W, H)), csv, targets = small_dataset
    data = bop_eval.load_dataset(root, "synth", "test")
    assert data["targets"] == targets and (3, 5) not in data["targets"] and 5 not in data["targets"][(4, 0)] and data["im_size"] == (W, H)
    assert sorted(data["models"]) == sorted(models)
    for oid, m in models.items():
        got = data["models"][oid]
        assert got["diameter"] == m["diameter"] and np.array_equal(got["faces"], m["faces"])
        want = m["verts"] if oid == 1 else m["verts"].astype(np.float32).astype(np.float64)  # object 1 is the ASCII file
        assert np.array_equal(got["pts"], want) and got["verts"] is got["pts"]
    assert len(data["models"][1]["symmetries"]) == 315 and len(data["models"][2]["symmetries"]) == 2 and len(data["models"][5]["symmetries"]) == 1
    for oid in models:
        assert np.array_equal(data["models"][oid]["symmetries"][0]["R"], np.eye(3))
    assert np.allclose(data["models"][2]["symmetries"][1]["R"], models[2]["symmetries"][1]["R"])
    for (sid, iid) in targets:
        assert np.array_equal(data["cameras"][sid][iid], cameras[sid][iid]) and data["depth_scales"][sid][iid] == 0.1
        for got, want in zip(data["scene_gt"][sid][iid], scene_gt[sid][iid]):
            assert got["obj_id"] == want["obj_id"] and np.array_equal(got["R"], want["R"]) and np.array_equal(got["t"], want["t"])
        d = data["depth_images"][sid][iid]
        assert d.dtype == np.float32 and d.shape == (H, W) and np.abs(d - depth_images[sid][iid]).max() <= 0.05 + 1e-3  # mm, 0.1 mm steps
        assert ((d == 0) == (depth_images[sid][iid] < 0.05)).all()
    assert 3 in data["scene_gt"] and 5 not in data["scene_gt"][3]  # an image outside the targets is not loaded
    # the LRU is bounded
    images = bop_eval.DepthImages(os.path.join(root, "synth", "test"), data["depth_scales"], max_images=2)
    for sid, iid in targets:
        images[sid][iid]
    assert len(images._store) == 2
    assert bop_eval.read_results(csv)[0]["R"].shape == (3, 3) and len(bop_eval.read_results(csv)) == len(results)


def test_only_targets_are_scored_and_inst_count_bounds_n_top():
    models, scene_gt, cameras, results, im_width = make_case()
    everything = {(sid, iid): {o: sum(g["obj_id"] == o for g in gts) for o in {g["obj_id"] for g in gts}} for sid, ims in scene_gt.items() for iid, gts in ims.items()}
    base = bop_eval.average_recall(results, scene_gt, models, cameras, im_width, n_top=1)
    assert bop_eval.average_recall(results, scene_gt, models, cameras, im_width, n_top=1, targets=everything) == base
    # without an image: the same as without its ground truths and estimates
    fewer = {k: v for k, v in everything.items() if k != (48, 7)}
    gt_wo = {sid: {iid: g for iid, g in ims.items() if (sid, iid) != (48, 7)} for sid, ims in scene_gt.items()}
    res_wo = [r for r in results if (r["scene_id"], r["im_id"]) != (48, 7)]
    want = bop_eval.average_recall(res_wo, gt_wo, models, cameras, im_width, n_top=1)
    assert bop_eval.average_recall(results, scene_gt, models, cameras, im_width, n_top=1, targets=fewer) == want != base
    # without an object of an image: its ground truth is no target (not valid) and its estimates are dropped
    no_obj = {k: {o: n for o, n in v.items() if (k, o) != ((49, 1), 2)} for k, v in everything.items()}
    gt_inv = {sid: {iid: [dict(g, valid=g["valid"] and (sid, iid, g["obj_id"]) != (49, 1, 2)) for g in gts] for iid, gts in ims.items()}
              for sid, ims in scene_gt.items()}
    res_no = [r for r in results if (r["scene_id"], r["im_id"], r["obj_id"]) != (49, 1, 2)]
    want = bop_eval.average_recall(res_no, gt_inv, models, cameras, im_width, n_top=1)
    assert bop_eval.average_recall(results, scene_gt, models, cameras, im_width, n_top=1, targets=no_obj) == want != base
    # the selection: inst_count (here 1 everywhere) bounds n_top and is what -1 means; 0 takes every estimate
    walk = lambda n_top, t: [len(rows) for *_, picked in bop_eval._walk(results, scene_gt, cameras, n_top, t) for _, rows in picked]  # noqa: E731
    assert max(walk(-1, None)) == 2 and max(walk(2, None)) == 2 and walk(0, everything) == walk(-1, None)
    assert set(walk(-1, everything)) == set(walk(2, everything)) == {1} and walk(1, everything) == walk(1, None)
    two = {k: {o: 2 for o in v} for k, v in everything.items()}
    assert walk(-1, two) == walk(2, two) == walk(5, two) == walk(2, None) and walk(1, two) == walk(1, None)


def test_host_route_returns_the_golden_values():
    """`average_recall` without `device` against the bop_toolkit_lib golden values, as tests/test_bop_eval_cpu.py holds it."""
    from raster_np import NumpyRenderer

    want = json.load(open(os.path.join(GOLD, "bop_eval.json")))
    models, scene_gt, cameras, results, im_width = make_case()
    out = bop_eval.average_recall(results, scene_gt, models, cameras, im_width, n_top=1)
    assert np.allclose(out["recalls_mssd"], want["recalls_mssd"]) and np.allclose(out["recalls_mspd"], want["recalls_mspd"])
    assert abs(out["AR_MSSD"] - want["AR_MSSD"]) < 1e-12 and abs(out["AR_MSPD"] - want["AR_MSPD"]) < 1e-12
    assert out["AR_VSD"] is None and out["AR"] is None and out["recalls_vsd"] is None
    want = want["vsd"]
    models, scene_gt, cameras, results, im_width, depth_images, (W, H) = make_vsd_case()
    ren = NumpyRenderer(W, H)
    for oid, m in models.items():
        ren.add_object(oid, m["verts"], m["faces"])
    out = bop_eval.average_recall(results, scene_gt, models, cameras, im_width, n_top=1, renderer=ren, depth_images=depth_images)
    assert np.allclose(out["recalls_vsd"], want["recalls_vsd"]) and np.allclose(out["recalls_mssd"], want["recalls_mssd"])
    assert np.allclose(out["recalls_mspd"], want["recalls_mspd"])
    for k in ("AR_VSD", "AR_MSSD", "AR_MSPD", "AR"):
        assert abs(out[k] - want[k]) < 1e-12, k
    assert sorted(out) == ["AR", "AR_MSPD", "AR_MSSD", "AR_MSSD_MSPD", "AR_VSD", "recalls_mspd", "recalls_mssd", "recalls_vsd"]
    # the device route is never entered silently, and never on a CPU device
    with pytest.raises(RuntimeError):
        bop_eval.average_recall(results, scene_gt, models, cameras, im_width, n_top=1, device="cpu")


def test_score_csv_on_the_host_writes_the_scores_file(small_dataset):
    """`score_csv` with the host scorer and the numpy rasteriser: the scores file beside the CSV, the targets' effect, the keys."""
    from raster_np import NumpyRenderer

    root, (models, scene_gt, cameras, results, im_width, depth_images, (W, H)), csv, targets = small_dataset
    out = bop_eval.score_csv(csv, root, "synth", "test", device_scoring=False, renderer=NumpyRenderer(W, H))
    path = os.path.join(os.path.dirname(csv), "scores_bop19.json")
    assert os.path.exists(path) and json.load(open(path)) == json.loads(json.dumps(out))
    assert sorted(out) == sorted(["AR", "AR_VSD", "AR_MSSD", "AR_MSPD", "AR_MSSD_MSPD", "recalls_vsd", "recalls_mssd", "recalls_mspd", "n_targets",
                                  "n_estimates", "n_scored_estimates", "dataset", "split", "n_top", "vsd_delta", "scorer"])
    assert out["n_targets"] == sum(len(v) for v in targets.values()) and out["n_estimates"] == len(results) and out["scorer"] == "host"
    assert out["n_scored_estimates"] < len(results) and out["vsd_delta"] == 15.0 and out["n_top"] == -1
    assert 0.0 < out["AR_VSD"] < 1.0 and 0.0 < out["AR_MSSD"] < 1.0 and 0.0 < out["AR_MSPD"] < 1.0 and abs(out["AR"] - np.mean([out["AR_VSD"], out["AR_MSSD"], out["AR_MSPD"]])) < 1e-12
    assert bop_eval.VSD_DELTAS["itodd"] == 5.0


BASE = dict(model=dict(cfg=dict(coarse_npoint=196)),
            dataloader=dict(test=dict(dataset=dict(eval_dataset_name="itodd", detetion_path="d.json", cfg=dict(img_size=224, data_dir="/data/bop")))),
            test=dict(amp=dict(enabled=False), instance_batch_size=16), misc=dict(output_dir="output/unopose", load_from="/x/ckpt_12.pth"),
            bop_eval=dict(split="test"))


def _plan(tmp_path, *extra):
    cfgf = tmp_path / "c.json"
    cfgf.write_text(json.dumps(BASE))
    r = subprocess.run([sys.executable, "-m", "unopose_amd.cli", "--config-file", str(cfgf), "--print-plan", *extra], capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=ROOT), cwd=ROOT)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_print_plan_reports_the_evaluation(tmp_path):
    plain, ev = _plan(tmp_path), _plan(tmp_path, "--eval")
    assert plain["eval"] is False and ev["eval"] is True
    new = {"eval", "eval_device", "eval_paths", "eval_scores", "eval_n_top", "eval_vsd_delta"}
    assert set(ev) - set(plain) == new - {"eval"} and {k: v for k, v in ev.items() if k not in new} == {k: v for k, v in plain.items() if k != "eval"}
    assert ev["eval_paths"] == dict(targets="/data/bop/itodd/test_targets_bop19.json", models_info="/data/bop/itodd/models_eval/models_info.json",
                                    models="/data/bop/itodd/models_eval", split="/data/bop/itodd/test")
    assert ev["eval_scores"] == "output/unopose/inference_ckpt_12/itodd/scores_bop19.json" and ev["eval_device"] is True
    assert ev["eval_n_top"] == -1 and ev["eval_vsd_delta"] == 5.0  # ITODD's visibility tolerance (bop_eval_utils.py:348-362)
    off = _plan(tmp_path, "--eval", "--eval-device-off", "bop_eval.targets_filename=test_targets_multiview_bop25.json", "bop_eval.n_top=1",
                "bop_eval.vsd_delta=15", "dataloader.test.dataset.eval_dataset_name=lmo", "bop_eval.split=test_primesense")
    assert off["eval_device"] is False and off["eval_n_top"] == 1 and off["eval_vsd_delta"] == 15.0
    assert off["eval_paths"]["targets"] == "/data/bop/lmo/test_targets_multiview_bop25.json" and off["eval_paths"]["split"] == "/data/bop/lmo/test_primesense"
    from unopose_amd import cli

    assert "--eval-device-off" in cli.__doc__
