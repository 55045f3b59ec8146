"""CPU: the further error types of `unopose_amd.bop_eval` (add, adi, ad, ABS*, AUC*, re, te, rete, proj and the symmetry-aware forms): the
host functions against the reference's own lib/pysixd values (tests/golden/pose_metrics.json, made by
tests/golden/make_pose_metrics_golden.py), the error table, the two-element matching, the settings and the CLI plan."""
import json
import os

import numpy as np
import pytest

import bop_score_case as C
import pose_metrics_case as M
from bop_eval_case import make_case
from unopose_amd import bop_eval

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "pose_metrics.json")))
NAMES = ("add", "adi", "proj", "re", "te", "projS", "reS", "teS")


@pytest.fixture(scope="module")
def cases():
    return M.kernel_cases()


@pytest.fixture(scope="module")
def large():
    return C.make_large_case()


@pytest.fixture(scope="module")
def host(cases):
    return {c["name"]: M.host_values(c) for c in cases}


def test_host_functions_equal_the_reference(cases, host):
    """|delta| <= 1e-9 max(1, value) against lib/pysixd/pose_error.py on every kernel case, and the cases are graded as described."""
    assert sorted(GOLD["kernel"]) == sorted(c["name"] for c in cases)
    worst = {k: 0.0 for k in NAMES}
    for c in cases:
        want = GOLD["kernel"][c["name"]]
        assert all(M.kernel_case_facts(c, want).values()), (c["name"], M.kernel_case_facts(c, want))
        for k in NAMES:
            for kind, a, b in zip(M.POSE_KINDS, host[c["name"]][k], want[k]):
                worst[k] = max(worst[k], abs(a - b) / max(1.0, abs(b)))
                assert abs(a - b) <= 1e-9 * max(1.0, abs(b)), (c["name"], k, kind, a, b)
    print("host functions against the reference, worst |delta| / max(1, value):", {k: "%.1e" % v for k, v in worst.items()})
    assert {len(c["pts"]) for c in cases} >= {1, 2, 63, 64, 65, M.SLAB - 1, M.SLAB + 1, M.TILE - 1, M.TILE, M.TILE + 1, 2 * M.TILE + 3}
    assert sorted({len(c["symmetries"]) for c in cases}) == [1, 2, 5, 315]
    assert any(np.abs(s["t"]).max() > 1.0 for c in cases if len(c["symmetries"]) == 5 for s in c["symmetries"])


def test_host_adi_equals_a_kd_tree(cases, host):
    """The chunked brute force against scipy's cKDTree, what the toolkit's `adi` uses; a small chunk makes it take several passes."""
    from scipy import spatial

    for c in cases:
        for i, (Re, te, Rg, tg) in enumerate(c["poses"]):
            est, gt = c["pts"] @ Re.T + te, c["pts"] @ Rg.T + tg
            want = float(spatial.cKDTree(est).query(gt, k=1)[0].mean())
            assert abs(host[c["name"]]["adi"][i] - want) <= 1e-9 * max(1.0, want), (c["name"], i)
            if len(c["pts"]) in (65, M.SLAB + 1):
                assert bop_eval.adi(Re, te, Rg, tg, c["pts"], chunk=1000) == pytest.approx(want, rel=1e-12, abs=1e-12)


def test_the_error_table():
    T = bop_eval.ERROR_TYPES
    assert set(T) == set(M.NEW_TYPES) and bop_eval.KNOWN_ERROR_TYPES[:3] == ("vsd", "mssd", "mspd") and "cus" not in bop_eval.KNOWN_ERROR_TYPES
    for k in ("add", "adi", "ad"):
        assert T[k]["thresholds"] == [[0.02], [0.05], [0.1]] and T[k]["by_diameter"] and T[k]["sphere_rule"] and not T[k]["cm"]
        assert T["ABS" + k]["thresholds"] == [[2.0]] and T["ABS" + k]["cm"] and not T["ABS" + k]["by_diameter"] and not T["ABS" + k]["sphere_rule"]
        assert np.allclose(np.ravel(T["AUC" + k]["thresholds"]), np.arange(1, 11)) and T["AUC" + k]["auc"] and T["AUC" + k]["cm"]
    for k in ("re", "te", "proj", "reS", "teS", "projS"):
        assert T[k]["thresholds"] == [[2.0], [5.0], [10.0]] and not T[k]["by_diameter"] and not T[k]["sphere_rule"]
    assert T["rete"]["thresholds"] == T["reteS"]["thresholds"] == [[2.0, 2.0], [5.0, 5.0], [10.0, 10.0]]
    assert T["rete"]["elements"] == ("re", "te") and T["reteS"]["elements"] == ("reS", "teS")
    v = dict(add=30.0, adi=12.0, re=3.0, te=40.0, reS=1.0, teS=25.0, proj=4.0, projS=2.0)
    e = lambda k, sym=False, apart=False: bop_eval.pair_error(k, v, 200.0, sym, apart)  # noqa: E731
    assert e("add") == [0.15] and e("adi") == [0.06] and e("ad") == [0.15] and e("ad", sym=True) == [0.06]
    assert e("add", apart=True) == e("ad", True, True) == e("adi", apart=True) == [float("inf")]
    assert e("ABSadd", apart=True) == [3.0] and e("AUCad", sym=True, apart=True) == [1.2] and e("AUCadi") == [1.2]  # cm, no sphere rule
    assert e("rete") == [3.0, 4.0] and e("reteS") == [1.0, 2.5] and e("te") == [4.0] and e("teS") == [2.5] and e("re") == [3.0]
    assert e("proj") == [4.0] and e("projS", apart=True) == [2.0]


def test_the_sphere_rule_spares_the_adi(large):
    """A pair whose centres are a diameter or more apart is decided on the host: no ADI is computed for it unless an ABS / AUC type asks."""
    models, scene_gt, cameras, results = large[:4]
    walk = list(bop_eval._walk(results, scene_gt, cameras, -1, None))
    sym = set(bop_eval.default_symmetric_obj_ids(models))
    assert sym == {2, 3}
    pairs = bop_eval.metric_pairs(walk, models, ("ad", "rete"), sym)
    assert len(pairs) == GOLD["large"]["n_pairs"] == 259 and sum(p["apart"] for p in pairs) == GOLD["large"]["n_apart"] == 53
    for p in pairs:
        want = {"re", "te"} | ({"add"} if p["obj_id"] == 1 else set() if p["apart"] else {"adi"})
        assert p["bases"] == want, (p["key"], p["bases"])
    pairs = bop_eval.metric_pairs(walk, models, ("ad", "AUCad"), sym)
    assert all(("adi" in p["bases"]) == (p["obj_id"] != 1) for p in pairs)
    pairs = bop_eval.metric_pairs(walk, models, ("ad",), set())
    assert all(p["bases"] == {"add"} for p in pairs)


def test_matching_over_two_error_elements():
    """pose_matching.match_poses: an estimate matches when EVERY element is below its threshold, and a later ground truth replaces the
    best so far only when every element is lower."""
    gts = [dict(obj_id=1, valid=True), dict(obj_id=1, valid=True), dict(obj_id=2, valid=True), dict(obj_id=2, valid=False)]
    ests = [dict(score=0.9, errors={0: [1.0, 4.0], 1: [3.0, 1.0]}),   # takes 0; 1 is not lower in both elements
            dict(score=0.8, errors={0: [0.1, 0.1], 1: [4.0, 6.0]}),   # 0 is taken, 1 misses the second threshold
            dict(score=0.7, errors={2: [float("nan"), 0.0], 3: [0.0, 0.0]})]  # NaN never matches, 3 is not valid
    recall, objs = bop_eval.localization_scores([(gts, ests)], [5.0, 5.0], [1, 2, 3], -1)
    assert recall == 1 / 3 and objs == {1: 0.5, 2: 0.0, 3: 0.0}
    assert bop_eval.localization_scores([(gts, ests)], [5.0, 7.0], [1, 2], -1)[0] == 2 / 3
    # n_top = 1 (the walk hands over one estimate per image and object): an image holds one target of an object, however many instances
    assert bop_eval.localization_scores([(gts, ests[:1])], [5.0, 7.0], [1, 2], 1)[1] == {1: 1.0, 2: 0.0}


@pytest.mark.parametrize("which", ["large", "scoring"])
def test_host_route_reproduces_the_reference_recalls(which, large):
    case = large if which == "large" else M.make_scoring_case(case=large)
    models, scene_gt, cameras, results, im_width = case[:5]
    out = bop_eval.average_recall(results, scene_gt, models, cameras, im_width, n_top=-1, error_types=",".join(M.NEW_TYPES))
    assert out["symmetric_obj_ids"] == [2, 3] and list(out["errors"]) == list(M.NEW_TYPES) and out["AR_VSD"] is None
    for T in M.NEW_TYPES:
        got, want = out["errors"][T], GOLD[which]["errors"][T]
        assert got["recalls"] == want["recalls"] and {str(o): v for o, v in got["obj_recalls"].items()} == want["obj_recalls"], T
        assert abs(got["mean_recall"] - want["mean_recall"]) <= 1e-12 and got["thresholds"] == bop_eval.ERROR_TYPES[T]["thresholds"]
        assert abs(got["mean_obj_recall"] - np.mean([np.mean(v) for v in want["obj_recalls"].values()])) <= 1e-12
    pairs = bop_eval.metric_pairs(list(bop_eval._walk(results, scene_gt, cameras, -1, None)), models, M.NEW_TYPES, {2, 3})
    facts = M.scoring_case_facts(out["errors"], pairs)
    if which == "scoring":
        assert all(facts.values()), facts
    else:  # the figures the large case was chosen by; without the added estimates `rete` is `re`
        r = lambda T: [round(v, 2) for v in out["errors"][T]["recalls"]]  # noqa: E731
        assert r("ad") == [0.55, 0.71, 0.83] and r("add") == [0.35, 0.45, 0.57] and r("proj") == [0.36, 0.47, 0.56] and r("rete") == r("re") == [0.41, 0.52, 0.67]
        assert r("AUCad")[0] == 0.75 and r("AUCad")[-1] == 0.92 and not facts["rete_is_neither"]
    table = bop_eval.format_error_table(out["errors"]).splitlines()
    assert table[0].split()[:4] == ["objects", "add_0.02", "add_0.05", "add_0.1"] and "AUCad_1:10" in table[0] and "rete_2" in table[0]
    assert [l.split()[0] for l in table[1:]] == ["1", "2", "3", "Avg(3)"] and len({len(l.split()) for l in table}) == 1


def test_the_default_dictionaries_are_unchanged(tmp_path):
    from raster_np import NumpyRenderer
    from bop_eval_case import make_vsd_case

    models, scene_gt, cameras, results, im_width = make_case()
    base = bop_eval.average_recall(results, scene_gt, models, cameras, im_width, n_top=1)
    keys = ["AR", "AR_MSPD", "AR_MSSD", "AR_MSSD_MSPD", "AR_VSD", "recalls_mspd", "recalls_mssd", "recalls_vsd"]
    assert sorted(base) == keys
    for spec in (("vsd", "mssd", "mspd"), "vsd,mssd,mspd", None):
        assert bop_eval.average_recall(results, scene_gt, models, cameras, im_width, n_top=1, error_types=spec) == base
    more = bop_eval.average_recall(results, scene_gt, models, cameras, im_width, n_top=1, error_types="mssd,mspd,te")
    assert sorted(more) == sorted(keys + ["errors", "symmetric_obj_ids"]) and {k: more[k] for k in keys} == base
    assert more["errors"]["mssd"]["recalls"] == base["recalls_mssd"] and more["errors"]["mspd"]["recalls"] == base["recalls_mspd"]
    assert set(more["errors"]) == {"mssd", "mspd", "te"} and set(more["errors"]["mssd"]["obj_recalls"]) == set(models)
    # with a renderer: VSD is rendered only when it is asked for, and then tabulated per object too, weighted by the instance counts
    case = make_vsd_case()
    models, scene_gt, cameras, results, im_width, depth_images, (W, H) = case
    ren = NumpyRenderer(W, H)
    for oid, m in models.items():
        ren.add_object(oid, m["verts"], m["faces"])
    full = bop_eval.average_recall(results, scene_gt, models, cameras, im_width, n_top=1, renderer=ren, depth_images=depth_images)
    assert sorted(full) == keys

    class NoRender:
        def render_object(self, *a, **k):
            raise AssertionError("rendered although vsd was not asked for")

    skip = bop_eval.average_recall(results, scene_gt, models, cameras, im_width, n_top=1, renderer=NoRender(), depth_images=depth_images,
                                   error_types="ad,rete,proj")
    assert skip["AR_VSD"] is None and skip["AR"] is None and skip["recalls_mssd"] == full["recalls_mssd"] and set(skip["errors"]) == {"ad", "rete", "proj"}
    both = bop_eval.average_recall(results, scene_gt, models, cameras, im_width, n_top=1, renderer=ren, depth_images=depth_images,
                                   error_types="vsd,mssd,ad")
    assert {k: both[k] for k in keys} == full and both["errors"]["vsd"]["recalls"] == full["recalls_vsd"]
    assert abs(both["errors"]["vsd"]["mean_recall"] - full["AR_VSD"]) <= 1e-12
    blk = both["errors"]["mssd"]
    counts = {o: sum(g["valid"] and g["obj_id"] == o for ims in scene_gt.values() for gts in ims.values() for g in gts) for o in models}
    want = sum(counts[o] * np.mean(blk["obj_recalls"][o]) for o in models) / sum(counts.values())
    assert abs(blk["mean_obj_recall"] - want) <= 1e-12


def test_score_csv_default_and_further_types(tmp_path):
    from raster_np import NumpyRenderer
    from bop_eval_case import make_vsd_case

    case = make_vsd_case()
    csv, _ = C.write_dataset(str(tmp_path), case, skip_image=(-1, -1), skip_object=(-1, -1, -1))
    W, H = case[6]
    base = bop_eval.score_csv(csv, str(tmp_path), "synth", "test", device_scoring=False, renderer=NumpyRenderer(W, H))
    assert "errors" not in base and "error_types" not in base and "symmetric_obj_ids" not in base
    out = bop_eval.score_csv(csv, str(tmp_path), "synth", "test", device_scoring=False, error_types="ad,AUCad,rete", symmetric_obj_ids=[1])  # no renderer
    path = os.path.join(os.path.dirname(csv), "scores_bop19.json")
    assert json.load(open(path)) == json.loads(json.dumps(out))
    assert set(out) - set(base) == {"errors", "error_types", "symmetric_obj_ids"} and set(base) <= set(out)
    assert out["error_types"] == ["ad", "AUCad", "rete"] and out["symmetric_obj_ids"] == [1] and out["AR_VSD"] is None
    assert out["recalls_mssd"] == base["recalls_mssd"]


def test_error_types_parsing():
    p = bop_eval.parse_error_types
    assert p(None) == ("vsd", "mssd", "mspd") and p("ad, rete,proj,ad") == ("ad", "rete", "proj") and p(["AUCad", "te"]) == ("AUCad", "te")
    for bad in ("ad,cus", "ADD", "", ["add", "nope"]):
        with pytest.raises(ValueError, match="known: vsd, mssd, mspd, add, adi, ad, ABSadd"):
            p(bad)
    models, scene_gt, cameras, results, im_width = make_case()
    with pytest.raises(ValueError, match="cus"):
        bop_eval.average_recall(results, scene_gt, models, cameras, im_width, error_types="ad,cus")


def test_symmetric_obj_ids_default_and_override(large):
    models, scene_gt, cameras, results, im_width = large[:5]
    a = bop_eval.average_recall(results, scene_gt, models, cameras, im_width, n_top=-1, error_types="ad,add,adi")
    assert a["symmetric_obj_ids"] == [2, 3] and a["errors"]["ad"]["obj_recalls"][1] == a["errors"]["add"]["obj_recalls"][1]
    assert a["errors"]["ad"]["obj_recalls"][2] == a["errors"]["adi"]["obj_recalls"][2] != a["errors"]["add"]["obj_recalls"][2]
    b = bop_eval.average_recall(results, scene_gt, models, cameras, im_width, n_top=-1, error_types="ad,add,adi", symmetric_obj_ids=[1])
    assert b["symmetric_obj_ids"] == [1] and b["errors"]["ad"]["obj_recalls"][2] == a["errors"]["add"]["obj_recalls"][2]
    assert b["errors"]["ad"]["obj_recalls"][1] == a["errors"]["adi"]["obj_recalls"][1] and b["errors"]["add"] == a["errors"]["add"]
    none = bop_eval.average_recall(results, scene_gt, models, cameras, im_width, n_top=-1, error_types="ad,add", symmetric_obj_ids=[])
    assert none["symmetric_obj_ids"] == [] and none["errors"]["ad"]["recalls"] == none["errors"]["add"]["recalls"]


BASE = dict(model=dict(cfg=dict(coarse_npoint=196)),
            dataloader=dict(test=dict(dataset=dict(eval_dataset_name="ycbv", detetion_path="d.json", cfg=dict(img_size=224, data_dir="/data/bop")))),
            test=dict(amp=dict(enabled=False), instance_batch_size=16), misc=dict(output_dir="output/unopose", load_from="/x/ckpt_12.pth"),
            bop_eval=dict(split="test"))


def _plan(tmp_path, capsys, *extra, cfg=BASE):
    """`--print-plan` touches no GPU and starts nothing: run in this process."""
    from unopose_amd import cli

    cfgf = tmp_path / "c.json"
    cfgf.write_text(json.dumps(cfg))
    assert cli.main(["--config-file", str(cfgf), "--print-plan", *extra]) == 0
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def test_print_plan_with_and_without_the_keys(tmp_path, capsys):
    from unopose_amd import cli

    plain = _plan(tmp_path, capsys, "--eval")
    assert "eval_error_types" not in plain and "eval_symmetric_obj_ids" not in plain
    ev = _plan(tmp_path, capsys, "--eval", "bop_eval.error_types=ad,AUCad,rete,proj", "bop_eval.symmetric_obj_ids=13,16,19")
    assert ev["eval_error_types"] == ["ad", "AUCad", "rete", "proj"] and ev["eval_symmetric_obj_ids"] == [13, 16, 19]
    assert {k: v for k, v in ev.items() if k not in ("eval_error_types", "eval_symmetric_obj_ids")} == plain
    listed = _plan(tmp_path, capsys, "--eval", cfg=dict(BASE, bop_eval=dict(split="test", error_types=["te", "reS"], symmetric_obj_ids=[4])))
    assert listed["eval_error_types"] == ["te", "reS"] and listed["eval_symmetric_obj_ids"] == [4]
    assert "eval_error_types" not in _plan(tmp_path, capsys, "bop_eval.error_types=ad")  # without --eval nothing is evaluated
    with pytest.raises(ValueError, match="unknown error type.*AUCad"):
        _plan(tmp_path, capsys, "--eval", "bop_eval.error_types=ad,cus")
    assert "bop_eval.error_types" in cli.__doc__ and "cus" in cli.__doc__


def test_the_ops_refuse_a_cpu_device():
    from unopose_amd import ops

    c = M.kernel_cases()[2]
    Re, te, Rg, tg = c["poses"][2]
    with pytest.raises(RuntimeError, match="CPU not supported"):
        ops.adi(c["pts"], [Re], [te], [Rg], [tg], "cpu")
    with pytest.raises(RuntimeError, match="CPU not supported"):
        ops.pose_metrics(c["pts"], c["symmetries"], [Re], [te], [Rg], [tg], c["K"], "cpu")
    models, scene_gt, cameras, results, im_width = make_case()
    with pytest.raises(RuntimeError):
        bop_eval.average_recall(results, scene_gt, models, cameras, im_width, n_top=1, device="cpu", error_types="ad")
