"""GPU: the further pose errors on the device (csrc/posemetrics.hip through ops.pose_metrics / ops.adi and
`bop_eval.average_recall(..., device=..., error_types=...)`) against the host functions and the reference's values
(tests/golden/pose_metrics.json): a rounding bound for the errors, bit-equal repeats, equal recall tables end to end, `score_csv`, the CLI."""
import json
import os

import numpy as np
import pytest
import torch

import bop_score_case as C
import pose_metrics_case as M

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_metrics.json")))
NAMES = ("add", "adi", "proj", "re", "te", "projS", "reS", "teS")


@pytest.fixture(scope="module")
def cases():
    return M.kernel_cases()


@pytest.fixture(scope="module")
def host(cases):
    return {c["name"]: M.host_values(c) for c in cases}


def _device_values(c):
    from unopose_amd import ops

    poses = [np.stack([p[i] for p in c["poses"]]) for i in range(4)]
    got = ops.pose_metrics(c["pts"], c["symmetries"], *poses, c["K"], "cuda")
    got["adi"] = ops.adi(c["pts"], *poses, "cuda")
    for v in got.values():
        assert v.dtype == torch.float64 and v.is_cuda and tuple(v.shape) == (len(c["poses"]),)
    return got


@pytest.fixture(scope="module")
def device(cases):
    return {c["name"]: _device_values(c) for c in cases}


def test_the_cases_straddle_the_kernel_sizes(cases):
    from unopose_amd.ops import score

    assert score.adi_sizes() == (M.TILE, M.SLAB)
    assert {len(c["pts"]) for c in cases} >= {1, 2, 63, 64, 65, M.SLAB - 1, M.SLAB + 1, M.TILE - 1, M.TILE, M.TILE + 1, 2 * M.TILE + 3}


@pytest.mark.parametrize("against", ["host", "golden"])
def test_kernel_outputs(against, cases, host, device):
    """|delta| <= 1e-9 max(1, value), the bound tests/test_bop_score_gpu.py derives for float64 sums of this kind: a mean over n <= 2051
    terms of size <= ~1.5e3 rounds within ~n 1e-16 relative in any order, and the rotation error is formed from the host's bits."""
    worst, over, facts = {k: 0.0 for k in NAMES}, [], {}
    for c in cases:  # one pass: every figure is collected before anything is asserted
        want = host[c["name"]] if against == "host" else GOLD["kernel"][c["name"]]
        got = {k: v.cpu().numpy() for k, v in device[c["name"]].items()}
        for k in NAMES:
            for kind, a, b in zip(M.POSE_KINDS, got[k], want[k]):
                rel = abs(a - b) / max(1.0, abs(b))
                worst[k] = max(worst[k], rel)
                if not rel <= 1e-9:  # a NaN is over the bound too
                    over.append((c["name"], k, kind, float(a), float(b)))
        facts[c["name"]] = M.kernel_case_facts(c, {k: v.tolist() for k, v in got.items()})
    print("device against the", against, "worst |delta| / max(1, value):", {k: "%.1e" % v for k, v in worst.items()})
    assert not over, (against, over[:8])
    assert all(all(f.values()) for f in facts.values()), {n: f for n, f in facts.items() if not all(f.values())}


def test_calling_twice_gives_the_same_bits(cases, device):
    for c in cases:
        if len(c["pts"]) in (65, M.SLAB + 1, 2 * M.TILE + 3):
            again = _device_values(c)
            for k in NAMES:
                assert torch.equal(again[k], device[c["name"]][k]), (c["name"], k)


def test_a_pair_does_not_depend_on_its_launch(cases, device):
    """One pair alone, and the same pair among others in another order: the same bits (the reduction tree is fixed by the launch shape)."""
    from unopose_amd import ops

    c = [c for c in cases if len(c["pts"]) == M.TILE + 1][0]
    Re, te, Rg, tg = c["poses"][3]
    one = ops.pose_metrics(c["pts"], c["symmetries"], [Re], [te], [Rg], [tg], c["K"], "cuda")
    assert all(float(one[k][0]) == float(device[c["name"]][k][3]) for k in one)
    assert float(ops.adi(c["pts"], [Re], [te], [Rg], [tg], "cuda")[0]) == float(device[c["name"]]["adi"][3])
    back = [np.stack([p[i] for p in c["poses"][::-1]]) for i in range(4)]
    assert torch.equal(ops.adi(c["pts"], *back, "cuda").flip(0), device[c["name"]]["adi"])


def test_without_the_symmetric_projection_pass(cases, device):
    """proj_sym=False leaves the points x symmetries pass out: no "projS", every other output with the same bits.  With the identity as the
    only symmetry the kernel leaves the pass out by itself and projS carries proj's bits."""
    from unopose_amd import ops

    for c in cases:
        if len(c["symmetries"]) in (5, 315) or len(c["pts"]) == 65:
            poses = [np.stack([p[i] for p in c["poses"]]) for i in range(4)]
            lean = ops.pose_metrics(c["pts"], c["symmetries"], *poses, c["K"], "cuda", proj_sym=False)
            assert sorted(lean) == sorted(set(NAMES) - {"adi", "projS"})
            assert all(torch.equal(v, device[c["name"]][k]) for k, v in lean.items()), c["name"]
        if len(c["symmetries"]) == 1:
            assert torch.equal(device[c["name"]]["projS"], device[c["name"]]["proj"]), c["name"]
    # a single symmetry that is NOT the identity still takes the pass
    from unopose_amd import bop_eval

    c = [c for c in cases if c["name"] == "two_fold"][0]
    poses = [np.stack([p[i] for p in c["poses"]]) for i in range(4)]
    got = ops.pose_metrics(c["pts"], c["symmetries"][1:], *poses, c["K"], "cuda")["projS"].cpu().numpy()
    for a, (Re, te, Rg, tg) in zip(got, c["poses"]):
        b = bop_eval.proj_sym(Re, te, Rg, tg, c["K"], c["pts"], c["symmetries"][1:])
        assert abs(a - b) <= 1e-9 * max(1.0, abs(b)), (a, b)


def test_non_finite_poses_and_argument_checks(cases):
    from unopose_amd import ops

    c = [c for c in cases if c["name"] == "two_fold"][0]
    poses = [np.stack([p[i] for p in c["poses"]]) for i in range(4)]
    bad = [a.copy() for a in poses]
    bad[0][1, 0, 0], bad[3][4, 2] = np.nan, np.inf
    got, ref = ops.pose_metrics(c["pts"], c["symmetries"], *bad, c["K"], "cuda"), ops.pose_metrics(c["pts"], c["symmetries"], *poses, c["K"], "cuda")
    a, a_ref = ops.adi(c["pts"], *bad, "cuda"), ops.adi(c["pts"], *poses, "cuda")
    keep = torch.tensor([True, False, True, True, False, True], device="cuda")
    for v, w in list(zip(got.values(), ref.values())) + [(a, a_ref)]:
        assert torch.isnan(v[~keep]).all() and torch.equal(v[keep], w[keep])
    for fn, args in ((ops.adi, ()), (ops.pose_metrics, (c["K"],))):
        head = (c["pts"],) if fn is ops.adi else (c["pts"], c["symmetries"])
        with pytest.raises(ValueError):
            fn(*head, poses[0][:0], poses[1][:0], poses[2][:0], poses[3][:0], *args, "cuda")  # no pairs
        with pytest.raises(ValueError):
            fn(*head, poses[0], poses[1], poses[2][:3], poses[3][:3], *args, "cuda")  # mismatched
        with pytest.raises(ValueError):
            fn(*head, poses[0], poses[1][:2], poses[2], poses[3], *args, "cuda")
        with pytest.raises(ValueError):
            fn(np.zeros((0, 3)), *head[1:], *poses, *args, "cuda")  # no points
        with pytest.raises(ValueError):
            fn(c["pts"] * np.nan, *head[1:], *poses, *args, "cuda")
        with pytest.raises(RuntimeError, match="CPU not supported"):
            fn(*head, *poses, *args, "cpu")
    with pytest.raises(ValueError):
        ops.pose_metrics(c["pts"], [], *poses, c["K"], "cuda")
    with pytest.raises(ValueError):
        ops.pose_metrics(c["pts"], c["symmetries"], *poses, np.stack([c["K"]] * 4), "cuda")


@pytest.fixture(scope="module")
def scoring():
    return M.make_scoring_case()


def _assert_same_errors(dev, host):
    assert list(dev["errors"]) == list(host["errors"]) and dev["symmetric_obj_ids"] == host["symmetric_obj_ids"]
    for T, h in host["errors"].items():
        d = dev["errors"][T]
        assert d["recalls"] == h["recalls"] and d["obj_recalls"] == h["obj_recalls"] and d["thresholds"] == h["thresholds"], T
        assert abs(d["mean_recall"] - h["mean_recall"]) <= 1e-12 and abs(d["mean_obj_recall"] - h["mean_obj_recall"]) <= 1e-12, T


def test_average_recall_on_the_device_equals_the_host_route(scoring):
    from unopose_amd import bop_eval

    models, scene_gt, cameras, results, im_width = scoring[:5]
    host = bop_eval.average_recall(results, scene_gt, models, cameras, im_width, n_top=-1, error_types=M.NEW_TYPES)
    dev = bop_eval.average_recall(results, scene_gt, models, cameras, im_width, n_top=-1, error_types=M.NEW_TYPES, device="cuda")
    _assert_same_errors(dev, host)
    assert dev["recalls_mssd"] == host["recalls_mssd"] and dev["AR_VSD"] is None and sorted(dev) == sorted(host)
    pairs = bop_eval.metric_pairs(list(bop_eval._walk(results, scene_gt, cameras, -1, None)), models, M.NEW_TYPES, {2, 3})
    facts = M.scoring_case_facts(dev["errors"], pairs)
    assert all(facts.values()), facts
    for T in M.NEW_TYPES:  # the reference's pose_matching + score.calc_localization_scores
        want = GOLD["scoring"]["errors"][T]
        assert dev["errors"][T]["recalls"] == want["recalls"] and {str(o): v for o, v in dev["errors"][T]["obj_recalls"].items()} == want["obj_recalls"], T
    # the reference's default table, with its own symmetric ids and n_top = 1
    kw = dict(n_top=1, error_types="ad,rete,proj", symmetric_obj_ids=[1, 3])
    _assert_same_errors(bop_eval.average_recall(results, scene_gt, models, cameras, im_width, device="cuda", **kw),
                        bop_eval.average_recall(results, scene_gt, models, cameras, im_width, **kw))


def test_the_large_case_reproduces_the_reference_recalls():
    from unopose_amd import bop_eval

    models, scene_gt, cameras, results, im_width = C.make_large_case()[:5]
    dev = bop_eval.average_recall(results, scene_gt, models, cameras, im_width, n_top=-1, error_types=M.NEW_TYPES, device="cuda")
    for T in M.NEW_TYPES:
        want = GOLD["large"]["errors"][T]
        assert dev["errors"][T]["recalls"] == want["recalls"] and {str(o): v for o, v in dev["errors"][T]["obj_recalls"].items()} == want["obj_recalls"], T
        assert abs(dev["errors"][T]["mean_recall"] - want["mean_recall"]) <= 1e-12


def test_score_csv_device_and_host_agree(scoring, tmp_path):
    from unopose_amd import bop_eval

    csv, targets = C.write_dataset(str(tmp_path), scoring)
    types = "vsd,mssd,mspd,ad,AUCad,rete,reteS,proj,projS"
    host = bop_eval.score_csv(csv, str(tmp_path), "synth", "test", device="cuda", device_scoring=False, error_types=types)
    dev = bop_eval.score_csv(csv, str(tmp_path), "synth", "test", device="cuda", error_types=types)
    written = json.load(open(os.path.join(os.path.dirname(csv), "scores_bop19.json")))
    assert written == json.loads(json.dumps(dev)) and written["scorer"] == "device" and written["error_types"] == types.split(",")
    assert set(dev["errors"]) == set(types.split(",")) and dev["symmetric_obj_ids"] == [2, 3]
    _assert_same_errors(dev, host)
    for k in ("recalls_vsd", "recalls_mssd", "recalls_mspd", "n_targets", "n_scored_estimates"):
        assert dev[k] == host[k], k
    assert dev["errors"]["vsd"]["recalls"] == dev["recalls_vsd"] and dev["errors"]["mssd"]["recalls"] == dev["recalls_mssd"]
    assert 0.0 < dev["errors"]["ad"]["mean_recall"] < 1.0 and 0.0 < dev["errors"]["rete"]["mean_recall"] < 1.0
    # the file's ADD(-S) does not come from a renderer: the same numbers without one
    lean = bop_eval.score_csv(csv, str(tmp_path), "synth", "test", device="cuda", error_types="ad,AUCad,rete,reteS,proj,projS")
    assert lean["AR_VSD"] is None and all(lean["errors"][T] == dev["errors"][T] for T in lean["errors"])


@torch.no_grad()
def test_cli_eval_prints_the_table_and_writes_the_file(tmp_path, capsys):
    """`python -m unopose_amd.cli ... --eval bop_eval.error_types=ad,AUCad,rete,proj` on the synthetic provider dataset, as
    tests/test_bop_score_gpu.py runs the BOP'19 evaluation: the AR line, one line per type, the per-object table, the scores file."""
    import bop_synth
    from unopose_amd import bop_eval, cli
    from unopose_amd.model import UNOPose, default_model_cfg
    from unopose_amd.synthetic import trained_like_

    root = str(tmp_path / "bop")
    dcfg, det_path = bop_synth.build(root)
    sv, sf = C.icosphere()
    info = {}
    for obj_id, axes in ((2, (30.0, 40.0, 25.0)), (5, (45.0, 25.0, 30.0))):
        C.write_ply(os.path.join(root, "ycbv", "models_eval", f"obj_{obj_id:06d}.ply"), sv * np.asarray(axes), sf, binary=obj_id == 2)
        info[str(obj_id)] = dict(diameter=2.0 * max(axes))
    info["5"]["symmetries_discrete"] = [np.diag([-1.0, -1.0, 1.0, 1.0]).reshape(-1).tolist()]
    json.dump(info, open(os.path.join(root, "ycbv", "models_eval", "models_info.json"), "w"))
    json.dump([dict(scene_id=48, im_id=1, obj_id=2, inst_count=1), dict(scene_id=48, im_id=1, obj_id=5, inst_count=1),
               dict(scene_id=48, im_id=2, obj_id=2, inst_count=1)], open(os.path.join(root, "ycbv", "test_targets_bop19.json"), "w"))
    mcfg = default_model_cfg(fine_npoint=256, feature_extraction=dict(img_size=dcfg["img_size"]))
    torch.manual_seed(3)
    model = trained_like_(UNOPose(mcfg))
    ckpt = str(tmp_path / "model_final.pth")
    torch.save({"model": model.state_dict(), "iteration": 7}, ckpt)
    cfg = dict(model=dict(cfg=dict(mcfg)), dataloader=dict(test=dict(dataset=dict(cfg=dcfg, eval_dataset_name="ycbv", detetion_path=det_path))),
               test=dict(amp=dict(enabled=False), instance_batch_size=2), misc=dict(output_dir=str(tmp_path / "out"), load_from=""), bop_eval=dict(split="test"))
    cfgf = tmp_path / "cfg.json"
    cfgf.write_text(json.dumps(cfg))
    with pytest.raises(ValueError, match="unknown error type"):  # before the checkpoint is even looked for
        cli.main(["--config-file", str(cfgf), "--eval", "misc.load_from=/nowhere.pth", "bop_eval.error_types=ad,cus"])
    np.random.seed(11)
    torch.manual_seed(5)
    assert cli.main(["--config-file", str(cfgf), "--eval", f"misc.load_from={ckpt}", "bop_eval.error_types=ad,AUCad,rete,proj"]) == 0
    lines = capsys.readouterr().out.splitlines()
    ar = [l for l in lines if l.startswith("BOP19 ycbv-test")]
    assert len(ar) == 1 and "AR_VSD    n/a" in ar[0] and ("AR_MSSD 0." in ar[0] or "AR_MSSD 1." in ar[0])
    for T in ("ad", "AUCad", "rete", "proj"):
        assert len([l for l in lines if l.startswith(T + " ") and "average recall" in l]) == 1, T
    head = [i for i, l in enumerate(lines) if l.startswith("objects")]
    assert len(head) == 1
    table = [l.split() for l in lines[head[0]:head[0] + 4]]
    assert table[0] == ["objects", "ad_0.02", "ad_0.05", "ad_0.1", "AUCad_1:10", "rete_2", "rete_5", "rete_10", "proj_2", "proj_5", "proj_10"]
    assert [r[0] for r in table[1:]] == ["2", "5", "Avg(2)"] and all(len(r) == len(table[0]) for r in table)
    out_dir = tmp_path / "out" / "inference_model_final" / "ycbv"
    dev = json.load(open(out_dir / "scores_bop19.json"))
    assert dev["scorer"] == "device" and dev["error_types"] == ["ad", "AUCad", "rete", "proj"] and dev["symmetric_obj_ids"] == [5] and dev["AR_VSD"] is None
    host = bop_eval.score_csv(str(out_dir / "result_ycbv-test.csv"), root, "ycbv", "test", device="cuda", device_scoring=False, error_types="ad,AUCad,rete,proj")
    _assert_same_errors(dev, json.loads(json.dumps(host)))
