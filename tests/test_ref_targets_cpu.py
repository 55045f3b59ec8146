"""CPU: the one-reference target rule of `unopose_amd.ref_targets` -- the hash's known answers, `select_host` against a restatement with numpy's
own products and Python loops (on inputs whose traces all lie away from the threshold, so the order of arithmetic cannot decide), the edge
cases and the exact boundary -- and its command line on the synthetic dataset of tests/bop_synth.py."""
import json
import os.path as osp

import numpy as np
import pytest

import bop_synth
import ref_targets_case as K
from unopose_amd import bop_eval, ref_targets
from unopose_amd.provider import BOPTestsetOneRef, ref_split_folder, rle_decode


def test_known_answers_of_the_hash():
    assert int(ref_targets.mix64(K.G)) == 0xE220A8397B1DCDAF
    assert int(ref_targets.mix64((2 * K.G) & K.M64)) == 0x6E789E6AA1B965F4
    assert int(ref_targets.mix64((3 * K.G) & K.M64)) == 0x06C45D188009454F
    assert int(ref_targets.priority(7, 3 << 32 | 5, 1 << 32 | 1000)) == 0x34A6928B644B7A82
    assert K.priority_int(7, 3 << 32 | 5, 1 << 32 | 1000) == 0x34A6928B644B7A82
    keys = np.array([[3 << 32 | 5], [K.M64]], np.uint64)  # broadcasting and wrap-around
    got = ref_targets.priority(K.M64, keys, np.array([1 << 32 | 1000, 0], np.uint64))
    assert got.shape == (2, 2) and all(int(got[i, j]) == K.priority_int(K.M64, int(keys[i, 0]), [1 << 32 | 1000, 0][j]) for i in range(2) for j in range(2))


def test_trace_min_is_the_trace_of_the_bound():
    assert ref_targets.trace_min_of(0) == 3.0 and abs(ref_targets.trace_min_of(180) + 1.0) < 1e-15
    assert abs(ref_targets.trace_min_of(50) - (1 + 2 * np.cos(np.deg2rad(50)))) < 1e-15


@pytest.mark.parametrize("S", [1, 315])
def test_host_rule_equals_a_plain_restatement(S):
    case = K.make_case(0, 40, 300, S)
    plain = K.plain_best(case)
    mine = ref_targets.best_traces(case["Rq"], case["Rc"], case["syms"])
    assert np.abs(mine - plain).max() < 1e-12
    seen_none = seen_all = False
    for max_rot in (20.0, 50.0):
        trace_min = ref_targets.trace_min_of(max_rot)
        assert np.abs(plain - trace_min).min() > 1e-9 and np.abs(mine - trace_min).min() > 1e-9  # no pair the order of arithmetic could decide
        for seed, cross in ((0, True), (12345, True), (0, False)) if S == 1 else ((7, True),):  # the 315-symmetry traces cost the host seconds per call
            pick, count, nearest, nearest_trace = K.host(case, max_rot, seed, cross)
            p_pick, p_count, p_nearest = K.plain_select(case, plain, trace_min, seed, cross)
            assert pick.tolist() == p_pick and count.tolist() == p_count
            assert all(a == b or abs(plain[q, a] - plain[q, b]) < 1e-12 for q, (a, b) in enumerate(zip(nearest.tolist(), p_nearest)))
            assert (nearest_trace == mine[np.arange(40), nearest]).all()
            seen_none |= bool((pick < 0).any())
            seen_all |= bool((pick >= 0).all())
            assert ((pick >= 0) == (count > 0)).all()
    assert seen_all and (seen_none or S > 1)  # both branches: at 20 degrees an asymmetric object leaves queries without a view
    if S == 1:  # the picks move with the seed and do not follow the nearest view
        a, b = K.host(case, 50.0, 0)[0], K.host(case, 50.0, 1)[0]
        assert (a != b).any() and (a != K.host(case, 50.0, 0)[2]).any()


def test_picks_do_not_depend_on_candidate_order_or_on_a_split():
    case = K.make_case(3, 17, 90, 2)
    pick = K.host(case, 50.0, 5)[0]
    order = np.random.RandomState(1).permutation(90)
    moved = dict(case, Rc=case["Rc"][order], c_scene=case["c_scene"][order], c_key=case["c_key"][order])
    again = K.host(moved, 50.0, 5)[0]
    assert [int(order[c]) if c >= 0 else -1 for c in again] == pick.tolist()
    small = ref_targets.select_host(case["Rq"], case["q_scene"], case["q_key"], case["Rc"], case["c_scene"], case["c_key"], case["syms"],
                                    ref_targets.trace_min_of(50.0), 5, True, block=1)  # one candidate at a time
    assert all(np.array_equal(x, y) for x, y in zip(small, K.host(case, 50.0, 5)))


def test_edge_cases():
    case = K.make_case(4, 6, 20, 1)
    same = dict(case, c_scene=np.full(20, 7, np.int64), q_scene=np.full(6, 7, np.int64))
    pick, count, nearest, nearest_trace = K.host(same, 180.0)
    assert (pick == -1).all() and (nearest == -1).all() and (count == 0).all() and np.isneginf(nearest_trace).all()
    # every candidate is the same view: equal priorities and equal traces go to the lower index
    dup = dict(case, Rc=np.repeat(case["Rc"][:1], 20, axis=0), c_key=np.repeat(case["c_key"][:1], 20), c_scene=np.full(20, 99, np.int64))
    pick, count, nearest, _ = K.host(dup, 180.0)
    assert (pick == 0).all() and (nearest == 0).all() and (count == 20).all()
    # same-scene: only the view itself is excluded
    own = dict(case, Rc=np.concatenate([case["Rq"][:1], case["Rc"]]), c_scene=np.concatenate([case["q_scene"][:1], np.full(20, case["q_scene"][0])]),
               c_key=np.concatenate([case["q_key"][:1], case["c_key"]]))
    pick, count, nearest, nearest_trace = K.host(own, 180.0, cross_scene=False)
    assert count[0] == 20 and (count[1:] == 21).all() and pick[0] != 0 and nearest[0] != 0 and nearest[1:].min() >= 0
    cross = K.host(own, 180.0, cross_scene=True)
    assert cross[1][0] == 0 and cross[0][0] == -1
    # nothing to choose from, nothing to choose for
    empty = dict(case, Rc=np.zeros((0, 3, 3)), c_scene=np.zeros(0, np.int64), c_key=np.zeros(0, np.uint64))
    pick, count, nearest, nearest_trace = K.host(empty, 50.0)
    assert pick.tolist() == [-1] * 6 and count.tolist() == [0] * 6 and nearest.tolist() == [-1] * 6 and np.isneginf(nearest_trace).all()
    none = dict(case, Rq=np.zeros((0, 3, 3)), q_scene=np.zeros(0, np.int64), q_key=np.zeros(0, np.uint64))
    assert [len(x) for x in K.host(none, 50.0)] == [0, 0, 0, 0]
    with pytest.raises(ValueError):
        K.host(dict(case, syms=np.zeros((0, 3, 3))), 50.0)
    with pytest.raises(ValueError):
        K.host(dict(case, Rc=np.where(np.arange(180).reshape(20, 3, 3) == 5, np.nan, case["Rc"])), 50.0)


def test_the_boundary_is_a_comparison_of_traces():
    case = K.make_case(5, 3, 4, 315)
    best = ref_targets.best_traces(case["Rq"], case["Rc"], case["syms"])
    one = dict(case, Rq=case["Rq"][1:2], q_scene=np.array([0]), q_key=case["q_key"][1:2], Rc=case["Rc"][2:3], c_scene=np.array([1]), c_key=case["c_key"][2:3])
    args = (one["Rq"], one["q_scene"], one["q_key"], one["Rc"], one["c_scene"], one["c_key"], one["syms"])
    at = ref_targets.select_host(*args, float(best[1, 2]))
    above = ref_targets.select_host(*args, float(np.nextafter(best[1, 2], np.inf)))
    assert at[0].tolist() == [0] and at[1].tolist() == [1] and above[0].tolist() == [-1] and above[1].tolist() == [0]
    assert above[2].tolist() == [0] and K.bits(above[3])[0] == K.bits(best[1, 2])[0]


def test_provider_and_tool_share_one_folder_rule(tmp_path):
    cfg, dets = bop_synth.build(str(tmp_path))
    ds = BOPTestsetOneRef(cfg, "ycbv", dets)
    for sid in (0, 10, 47, 48, 59, 60, 91):
        assert ds._ref_split_folder(sid) == ref_split_folder(cfg["data_dir"], "ycbv", sid) == ref_split_folder(cfg["data_dir"], "ycbv", sid, ds.data_folder)
    assert ref_split_folder("d", "tudl", 1) == osp.join("d", "tudl", "train_real") and ref_split_folder("d", "lmo", 2) == osp.join("d", "lmo", "test")


@pytest.fixture()
def synth(tmp_path):
    cfg, dets = bop_synth.build(str(tmp_path))
    return cfg, ["--host", "--data-dir", str(tmp_path), "--dataset", "ycbv", "--all-images"]


def test_missing_gt_info_names_the_tool(synth):
    with pytest.raises(FileNotFoundError, match="unopose_amd.gt_info"):
        ref_targets.main(synth[1] + ["--out", "new.json"])


def test_command_line_on_the_synthetic_dataset(synth, capsys):
    cfg, argv = synth
    root = cfg["data_dir"]
    K.write_gt_info(root)
    with pytest.raises(FileExistsError, match="--overwrite"):  # bop_synth wrote a list under the default name
        ref_targets.main(argv)
    assert ref_targets.main(argv + ["--overwrite"]) == 0
    path = osp.join(root, "ycbv", "test_ref_targets_crossscene_rot50.json")
    assert path == osp.join(root, "ycbv", cfg["ref_targets_name"])  # the defaults give the reference's own name
    entries = json.load(open(path))
    queries = [(48, 1, 2), (48, 1, 5), (48, 2, 2), (49, 7, 5), (49, 7, 2)]  # scene, image, scene_gt order
    assert [tuple(e) for e in entries] == [ref_targets.ENTRY_KEYS] * 5
    assert [(e["scene_id"], e["im_id"], e["obj_id"]) for e in entries] == queries
    assert all(e["ref_scene_id"] != e["scene_id"] for e in entries)
    assert {(e["ref_scene_id"], e["ref_im_id"]) for e in entries if e["obj_id"] == 5} == {(49, 7), (48, 1)}
    loaded = BOPTestsetOneRef.load_ref(path)
    assert loaded == {f"{e['scene_id']}_{e['im_id']}_{e['obj_id']}": f"{e['ref_scene_id']}_{e['ref_im_id']}" for e in entries} and len(loaded) == 5
    text = capsys.readouterr().out
    assert "total: 5 targets, 0 without an eligible view" in text and "obj      2: 3 targets, 4 candidate views" in text
    # the audit: every entry passes; the angles are the synthetic poses' (0.3 obj + 0.1 im about z)
    assert ref_targets.main(argv + ["--check", path]) == 0
    text = capsys.readouterr().out
    assert "total: 5 entries, 0 break the rule" in text and "BROKEN" not in text
    first = next(e for e in entries if (e["scene_id"], e["im_id"], e["obj_id"]) == (48, 1, 5))
    assert f"scene 48 image 1 object 5 -> scene {first['ref_scene_id']} image {first['ref_im_id']}: {np.rad2deg(0.6):.3f} deg, another scene" in text
    # hand-broken entries: a reference from the target's own scene, one beyond a tighter bound, one that does not exist
    for broken, extra, word in ((dict(entries[0], ref_scene_id=48, ref_im_id=2), [], "scene"), (entries[1], ["--max-rot", "30"], "rotation"),
                                (dict(entries[0], ref_im_id=77), [], "does not exist"), (entries[1], ["--min-visib", "1.5"], "visibility")):
        bad = osp.join(root, "broken.json")
        json.dump([entries[2], broken], open(bad, "w"))
        assert ref_targets.main(argv + extra + ["--check", bad]) == 1
        assert word in capsys.readouterr().out
    assert ref_targets.main(argv + ["--same-scene", "--check", osp.join(root, "broken.json")]) == 0  # entries[2] and entries[1] obey the same-scene rule
    assert json.load(open(path)) == entries  # --check wrote nothing


def test_skip_same_scene_and_ground_truth_detections(synth, capsys):
    cfg, argv = synth
    root = cfg["data_dir"]
    K.write_gt_info(root)
    # 20 degrees: object 5's only other view is 34 degrees away, and object 2 in (48, 1) at 0.7 rad has its other scenes' views at 1.1 and 1.3 rad
    assert ref_targets.main(argv + ["--max-rot", "20", "--fallback", "skip", "--out", "skip.json"]) == 0
    kept = json.load(open(osp.join(root, "ycbv", "skip.json")))
    assert "3 without an eligible view (left out)" in capsys.readouterr().out and [(e["scene_id"], e["im_id"], e["obj_id"]) for e in kept] == [(48, 2, 2), (49, 7, 2)]
    assert ref_targets.main(argv + ["--max-rot", "20", "--out", "near.json"]) == 0
    near = json.load(open(osp.join(root, "ycbv", "near.json")))
    assert len(near) == 5 and ref_targets.main(argv + ["--max-rot", "20", "--check", "near.json"]) == 1
    capsys.readouterr()
    assert ref_targets.main(argv + ["--same-scene", "--out", "same.json"]) == 0
    same = json.load(open(osp.join(root, "ycbv", "same.json")))
    assert len(same) == 5 and all((e["ref_scene_id"], e["ref_im_id"]) != (e["scene_id"], e["im_id"]) for e in same)
    # ground-truth detections: with the list written beside them the provider yields the first image
    dets = osp.join(root, "gt_dets.json")
    assert ref_targets.main(argv + ["--overwrite", "--gt-dets", dets]) == 0
    rows = json.load(open(dets))
    assert len(rows) == 5 and set(rows[0]) == {"scene_id", "image_id", "category_id", "bbox", "score", "time", "segmentation"}
    mask = rle_decode(rows[0]["segmentation"])
    x, y, w, h = rows[0]["bbox"]
    assert mask.shape == (bop_synth.H, bop_synth.W) and mask[y:y + h, x:x + w].sum() == mask.sum() > 0 and mask[y].any() and mask[:, x].any()
    np.random.seed(0)
    item = BOPTestsetOneRef(cfg, "ycbv", dets)[0]
    assert item["scene_id"].tolist() == [48] and item["img_id"].tolist() == [1] and item["obj_id"].reshape(-1).tolist() == [2, 5]
    with pytest.raises(FileExistsError):
        ref_targets.main(argv + ["--gt-dets", dets, "--out", "other.json"])


def test_a_pick_depends_on_its_target_alone(synth, capsys):
    """The same seed gives a target the same reference whatever else is listed, in whatever order, and whatever unrelated scenes exist: the
    keys behind the priorities are functions of (split folder, scene id, image) alone."""
    cfg, argv = synth
    root = cfg["data_dir"]
    K.write_gt_info(root)
    argv = [a for a in argv if a != "--all-images"] + ["--max-rot", "180", "--overwrite"]  # every allowed view is eligible: the hash alone decides
    rows = [dict(scene_id=s, im_id=i, obj_id=o, inst_count=1) for s, i, o in ((48, 1, 2), (48, 1, 5), (48, 2, 2), (49, 7, 5), (49, 7, 2))]
    lists = dict(all=rows, reversed=rows[::-1], object2=[r for r in rows if r["obj_id"] == 2][::-1], one=[rows[2]])
    for name, part in lists.items():
        json.dump(part, open(osp.join(root, "ycbv", f"targets_{name}.json"), "w"))

    def picks(name, seed):
        assert ref_targets.main(argv + ["--targets", f"targets_{name}.json", "--seed", str(seed), "--out", "out.json"]) == 0
        got = json.load(open(osp.join(root, "ycbv", "out.json")))
        assert [(e["scene_id"], e["im_id"], e["obj_id"]) for e in got] == [(r["scene_id"], r["im_id"], r["obj_id"]) for r in lists[name]]
        return {(e["scene_id"], e["im_id"], e["obj_id"]): (e["ref_scene_id"], e["ref_im_id"]) for e in got}

    seeds = range(12)
    base = {seed: picks("all", seed) for seed in seeds}
    assert len({tuple(sorted(b.items())) for b in base.values()}) > 1  # the seed does move the picks: the comparisons below can fail
    for name in ("reversed", "object2", "one"):
        for seed in seeds:
            assert all(base[seed][k] == v for k, v in picks(name, seed).items()), (name, seed)
    # scenes that hold none of the targets' objects, one per folder, sorting before and after the others
    rs = np.random.RandomState(9)
    bop_synth._scene(root, "train_real", 3, {4: [(9, (50, 60, 30, 24), 3600)]}, rs)
    bop_synth._scene(root, "test", 59, {1: [(9, (50, 60, 30, 24), 3600)]}, rs)
    K.write_gt_info(root)
    for seed in seeds:
        assert picks("all", seed) == base[seed], seed
    # the identity itself: the scene id in the split's folder, 2^24 + scene id under train_real
    ds = ref_targets._Dataset(root, "ycbv", "test")
    assert ds.identity(ds.test_folder, 48) == 48 and ds.identity(osp.join(root, "ycbv", "train_real"), 10) == (1 << 24) + 10
    with pytest.raises(ValueError):
        ds.identity(ds.test_folder, 1 << 24)
    capsys.readouterr()
