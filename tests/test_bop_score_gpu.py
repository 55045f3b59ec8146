"""GPU: the device route of the BOP'19 scorer (csrc/bopscore.hip through ops.vsd_counts / ops.pose_errors and
`bop_eval.average_recall(..., device=...)`) against the host route on the same rendered maps: integer equality for the VSD counts,
a rounding bound for MSSD / MSPD, equal recall tables end to end, the bop_toolkit golden values, chunking, `score_csv` and the CLI."""
import json
import os

import numpy as np
import pytest
import torch

import bop_score_case as C
from bop_eval_case import make_case, make_vsd_case

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def large():
    return C.make_large_case()


def _renderer(case):
    from unopose_amd.render import HipDepthRenderer

    models, (W, H) = case[0], case[6]
    ren = HipDepthRenderer(W, H)
    for oid, m in models.items():
        ren.add_object(oid, m["verts"], m["faces"])
    return ren


def _host_counts(d_est, d_gt, d_test, K, delta, taus, diameter):
    """The counts inside `bop_eval.vsd`, restated: inter.sum(), union.sum(), np.sum(dists >= tau)."""
    from unopose_amd.bop_eval import _visib_mask, depth_to_dist

    dist_test, dist_gt, dist_est = depth_to_dist(d_test, K), depth_to_dist(d_gt, K), depth_to_dist(d_est, K)
    visib_gt = _visib_mask(dist_test, dist_gt, delta)
    visib_est = np.logical_or(_visib_mask(dist_test, dist_est, delta), np.logical_and(visib_gt, dist_est > 0))
    inter, union = np.logical_and(visib_gt, visib_est), np.logical_or(visib_gt, visib_est)
    dists = np.abs(dist_gt[inter] - dist_est[inter])
    dists /= diameter
    return [int(union.sum()), int(inter.sum())] + [int(np.sum(dists >= tau)) for tau in taus]


def _pairs(case, n_top=-1):
    """Every scored pair of a case, in walk order: (estimate, ground truth, scene, image, K, object)."""
    from unopose_amd import bop_eval

    models, scene_gt, cameras, results = case[:4]
    out = []
    for sid, iid, K, obj_id, rows, mine in bop_eval.scored_pairs(bop_eval._walk(results, scene_gt, cameras, n_top, None)):
        out += [(r, g, sid, iid, K, obj_id) for r in rows for _, g in mine]
    return out


@pytest.mark.parametrize("which", ["vsd_case", "large"])
def test_vsd_counts_equal_the_host_counts(which, large):
    from unopose_amd import bop_eval, ops

    case = make_vsd_case() if which == "vsd_case" else large
    models, depth_images = case[0], case[5]
    ren = _renderer(case)
    pairs = _pairs(case)
    assert len(pairs) >= (200 if which == "large" else 15)
    images = list(dict.fromkeys((p[2], p[3]) for p in pairs))
    test = torch.from_numpy(np.stack([depth_images[s][i] for s, i in images])).cuda()
    deltas = [15.0] * len(pairs)
    if which == "large":
        deltas[C.ITODD_DELTA_PAIR] = 5  # the ITODD value, as the Python int the reference's table holds
    seen = {"empty_est": 0, "empty_union": 0, "zero_test": 0, "tau_counts": set()}
    for obj_id in models:
        sel = [k for k, p in enumerate(pairs) if p[5] == obj_id]
        K4 = np.asarray([[p[4][0, 0], p[4][1, 1], p[4][0, 2], p[4][1, 2]] for p in (pairs[k] for k in sel)])
        d_est = ren.render_batch(obj_id, np.stack([pairs[k][0]["R"] for k in sel]), np.stack([pairs[k][0]["t"] for k in sel]), K4)
        d_gt = ren.render_batch(obj_id, np.stack([pairs[k][1]["R"] for k in sel]), np.stack([pairs[k][1]["t"] for k in sel]), K4)
        got = ops.vsd_counts(test, d_gt, d_est, K4, [deltas[k] for k in sel], models[obj_id]["diameter"], bop_eval.VSD_TAUS,
                             image_index=[images.index((pairs[k][2], pairs[k][3])) for k in sel])
        assert got.dtype == torch.int64 and tuple(got.shape) == (len(sel), 2 + len(bop_eval.VSD_TAUS)) and got.is_cuda
        got, est_h, gt_h = got.cpu().numpy(), d_est.cpu().numpy(), d_gt.cpu().numpy()
        for j, k in enumerate(sel):
            r, g, sid, iid, K, _ = pairs[k]
            want = _host_counts(est_h[j], gt_h[j], depth_images[sid][iid], K, deltas[k], bop_eval.VSD_TAUS, models[obj_id]["diameter"])
            assert got[j].tolist() == want, (which, obj_id, k, got[j].tolist(), want)
            seen["empty_est"] += not (est_h[j] > 0).any()
            seen["empty_union"] += want[0] == 0
            seen["tau_counts"].add(tuple(want[2:]))
        seen["zero_test"] += int((test == 0).sum())
    assert seen["zero_test"] > 0 and len(seen["tau_counts"]) > len(pairs) // 4  # dropped test pixels; the counts differ between pairs
    if which == "large":
        assert seen["empty_est"] >= 2 and seen["empty_union"] >= 1  # behind the camera and outside the image; both outside: n_union = 0
        # the ITODD pair: its counts with delta = 5 differ from those with 15 (the tolerance is in the result)
        r, g, sid, iid, K, obj_id = pairs[C.ITODD_DELTA_PAIR]
        k4 = [K[0, 0], K[1, 1], K[0, 2], K[1, 2]]
        e, t = ren.render_batch(obj_id, r["R"][None], r["t"][None], k4), ren.render_batch(obj_id, g["R"][None], g["t"][None], k4)
        img = torch.from_numpy(depth_images[sid][iid][None]).cuda()
        c5, c15 = (ops.vsd_counts(img, t, e, k4, d, models[obj_id]["diameter"], bop_eval.VSD_TAUS).cpu().numpy()[0].tolist() for d in (5, 15.0))
        assert c5 != c15 and c5 == _host_counts(e[0].cpu().numpy(), t[0].cpu().numpy(), depth_images[sid][iid], K, 5, bop_eval.VSD_TAUS, models[obj_id]["diameter"])


def test_vsd_counts_without_vector_loads_and_argument_checks():
    """An image whose pixel count is not a multiple of 4 takes the scalar loop; wrong inputs are refused before the launch."""
    from unopose_amd import bop_eval, ops

    rs = np.random.RandomState(0)
    H, W = 37, 51
    K = np.array([[60.0, 0, 25.2], [0, 61.0, 18.1], [0, 0, 1.0]])
    k4 = [K[0, 0], K[1, 1], K[0, 2], K[1, 2]]
    maps = (rs.uniform(300, 420, size=(3, 2, H, W)) * (rs.rand(3, 2, H, W) < 0.7)).astype(np.float32)
    t, g, e = (torch.from_numpy(m).cuda() for m in maps)
    got = ops.vsd_counts(t, g, e, k4, 15.0, 100.0, bop_eval.VSD_TAUS[:3], image_index=[1, 0], gt_index=[0, 0], est_index=[1, 0]).cpu().numpy()
    assert got.shape == (2, 5)
    assert got[0].tolist() == _host_counts(maps[2][1], maps[1][0], maps[0][1], K, 15.0, bop_eval.VSD_TAUS[:3], 100.0)
    assert got[1].tolist() == _host_counts(maps[2][0], maps[1][0], maps[0][0], K, 15.0, bop_eval.VSD_TAUS[:3], 100.0) and got[:, 2].min() > 0
    with pytest.raises(ValueError):
        ops.vsd_counts(t, g, e, k4, 15.0, 100.0, bop_eval.VSD_TAUS, image_index=[0, 2])  # outside the stack of test images
    with pytest.raises(ValueError):
        ops.vsd_counts(t, g, e, k4, 15.0, 100.0, np.arange(17) * 0.01)
    with pytest.raises(RuntimeError):
        ops.vsd_counts(t.cpu(), g, e, k4, 15.0, 100.0, bop_eval.VSD_TAUS)
    with pytest.raises(RuntimeError):
        ops.vsd_counts(t, g[:, :-1].contiguous(), e, k4, 15.0, 100.0, bop_eval.VSD_TAUS)


def test_vsd_counts_on_maps_off_a_16_byte_boundary():
    """Contiguous views that start 4 bytes into an allocation: the entry point must not take the 16-byte loads."""
    from unopose_amd import bop_eval, ops

    rs = np.random.RandomState(1)
    H, W = 36, 52  # a multiple of 4 pixels: only the base pointers rule the wide loads out
    K = np.array([[60.0, 0, 25.2], [0, 61.0, 18.1], [0, 0, 1.0]])
    k4 = [K[0, 0], K[1, 1], K[0, 2], K[1, 2]]
    maps = (rs.uniform(300, 420, size=(3, 2, H, W)) * (rs.rand(3, 2, H, W) < 0.7)).astype(np.float32)
    shifted = []
    for m in maps:
        buf = torch.zeros(1 + m.size, dtype=torch.float32, device="cuda")
        buf[1:] = torch.from_numpy(m.reshape(-1)).cuda()
        shifted.append(buf[1:].view(2, H, W))
        assert shifted[-1].is_contiguous() and shifted[-1].data_ptr() % 16 == 4
    aligned = [torch.from_numpy(m).cuda() for m in maps]
    got = ops.vsd_counts(*shifted, k4, 15.0, 100.0, bop_eval.VSD_TAUS).cpu().numpy()
    assert np.array_equal(got, ops.vsd_counts(*aligned, k4, 15.0, 100.0, bop_eval.VSD_TAUS).cpu().numpy())
    for p in range(2):
        assert got[p].tolist() == _host_counts(maps[2][p], maps[1][p], maps[0][p], K, 15.0, bop_eval.VSD_TAUS, 100.0)


@pytest.mark.parametrize("which", ["case", "vsd_case", "large"])
def test_pose_errors_agree_with_the_host(which, large):
    """|delta| <= 1e-9 max(1, value): both sides are about a dozen float64 roundings on coordinates <= ~1.5e3 (absolute error near 1e-12)
    in different summation orders (the host goes through BLAS); 1e-9 leaves three orders of margin and sits seven orders below the
    smallest threshold step (0.05 of a diameter, 5 px)."""
    from unopose_amd import bop_eval, ops

    case = {"case": make_case, "vsd_case": make_vsd_case}[which]() if which != "large" else large
    models = case[0]
    pairs = _pairs(case)
    worst = 0.0
    for obj_id, m in models.items():
        sel = [p for p in pairs if p[5] == obj_id]
        e_s, e_p = ops.pose_errors(m["pts"], m["symmetries"], [p[0]["R"] for p in sel], [p[0]["t"] for p in sel], [p[1]["R"] for p in sel],
                                   [p[1]["t"] for p in sel], [p[4] for p in sel], "cuda")
        assert e_s.dtype == e_p.dtype == torch.float64 and tuple(e_s.shape) == tuple(e_p.shape) == (len(sel),) and e_s.is_cuda
        for (r, g, _, _, K, _), a, b in zip(sel, e_s.cpu().numpy(), e_p.cpu().numpy()):
            want_s = bop_eval.mssd(r["R"], r["t"], g["R"], g["t"], m["pts"], m["symmetries"])
            want_p = bop_eval.mspd(r["R"], r["t"], g["R"], g["t"], K, m["pts"], m["symmetries"])
            worst = max(worst, abs(a - want_s) / max(1.0, want_s), abs(b - want_p) / max(1.0, want_p))
            assert abs(a - want_s) <= 1e-9 * max(1.0, want_s) and abs(b - want_p) <= 1e-9 * max(1.0, want_p), (which, obj_id, a, want_s, b, want_p)
    print(f"pose_errors {which}: {len(pairs)} pairs, worst |delta| / max(1, value) = {worst:.3e}")


def test_pose_errors_over_more_symmetries_than_one_tile():
    """315 discretised steps of a continuous symmetry x 2 discrete ones = 630 symmetries: three LDS tiles, a short last block."""
    from unopose_amd import bop_eval, ops

    m = C._models()[2]
    syms = bop_eval.symmetry_transformations(dict(symmetries_continuous=[dict(axis=[0, 0, 1], offset=[3.0, -2.0, 0.0])],
                                                  symmetries_discrete=[np.diag([1.0, -1.0, -1.0, 1.0]).reshape(-1).tolist()]))
    assert len(syms) == 630
    rs = np.random.RandomState(2)
    K = np.array([[572.4, 0.3, 325.3], [0, 573.6, 242.0], [0, 0, 1.0]])  # with a skew term: the whole matrix is used
    Re, Rg = [C.rot(rs.randn(3), a) for a in (0.4, 2.0, 3.0)], [C.rot(rs.randn(3), a) for a in (0.5, 1.0, 2.5)]
    te, tg = rs.randn(3, 3) * 30 + [0, 0, 800], rs.randn(3, 3) * 30 + [0, 0, 800]
    for S in (630, 257, 3):
        e_s, e_p = ops.pose_errors(m["pts"], syms[:S], Re, te, Rg, tg, K, "cuda")
        for i in range(3):
            want_s, want_p = bop_eval.mssd(Re[i], te[i], Rg[i], tg[i], m["pts"], syms[:S]), bop_eval.mspd(Re[i], te[i], Rg[i], tg[i], K, m["pts"], syms[:S])
            assert abs(float(e_s[i]) - want_s) <= 1e-9 * max(1.0, want_s) and abs(float(e_p[i]) - want_p) <= 1e-9 * max(1.0, want_p)


def _assert_same(dev, host, vsd=True):
    assert sorted(dev) == sorted(host)
    for k in ("recalls_mssd", "recalls_mspd") + (("recalls_vsd",) if vsd else ()):
        assert dev[k] == host[k], k  # lists of floats, exactly
    for k in ("AR_MSSD", "AR_MSPD", "AR_MSSD_MSPD") + (("AR_VSD", "AR") if vsd else ()):
        assert abs(dev[k] - host[k]) <= 1e-12, k
    if not vsd:
        assert dev["AR_VSD"] is None and dev["AR"] is None and dev["recalls_vsd"] is None


@pytest.mark.parametrize("which,n_top", [("case", 1), ("vsd_case", 1), ("large", 1), ("large", 2), ("large", -1)])
def test_average_recall_on_the_device_equals_the_host_route(which, n_top, large):
    from unopose_amd import bop_eval

    if which == "case":  # no meshes: MSSD and MSPD only, AR_VSD and AR stay None on both routes
        models, scene_gt, cameras, results, im_width = make_case()
        host = bop_eval.average_recall(results, scene_gt, models, cameras, im_width, n_top=n_top)
        dev = bop_eval.average_recall(results, scene_gt, models, cameras, im_width, n_top=n_top, device="cuda")
        _assert_same(dev, host, vsd=False)
        return
    case = make_vsd_case() if which == "vsd_case" else large
    models, scene_gt, cameras, results, im_width, depth_images, _ = case
    ren = _renderer(case)
    host = bop_eval.average_recall(results, scene_gt, models, cameras, im_width, n_top=n_top, renderer=ren, depth_images=depth_images)
    dev = bop_eval.average_recall(results, scene_gt, models, cameras, im_width, n_top=n_top, renderer=ren, depth_images=depth_images, device="cuda")
    _assert_same(dev, host)
    if which == "large":
        assert all(C.large_case_facts(host).values()), C.large_case_facts(host)  # a graded problem: the equalities mean something
    # without depth images there is no VSD on either route
    dev = bop_eval.average_recall(results, scene_gt, models, cameras, im_width, n_top=n_top, renderer=ren, device="cuda")
    assert dev["AR_VSD"] is None and dev["AR"] is None and dev["recalls_mssd"] == host["recalls_mssd"]


def test_device_route_equals_bop_toolkit():
    """The device route under the assertions of test_bop_average_recall_with_the_hip_renderer_equals_bop_toolkit."""
    from unopose_amd import bop_eval

    want = json.load(open(os.path.join(GOLD, "bop_eval.json")))["vsd"]
    case = make_vsd_case()
    models, scene_gt, cameras, results, im_width, depth_images, _ = case
    out = bop_eval.average_recall(results, scene_gt, models, cameras, im_width, n_top=1, renderer=_renderer(case), depth_images=depth_images, device="cuda")
    assert np.allclose(out["recalls_vsd"], want["recalls_vsd"])
    for k in ("AR_VSD", "AR_MSSD", "AR_MSPD", "AR"):
        assert abs(out[k] - want[k]) < 1e-12, k


def test_device_route_refuses_another_renderer():
    from raster_np import NumpyRenderer
    from unopose_amd import bop_eval
    from unopose_amd.render import HipDepthRenderer

    case = make_vsd_case()
    models, scene_gt, cameras, results, im_width, depth_images, (W, H) = case
    ren = NumpyRenderer(W, H)
    for oid, m in models.items():
        ren.add_object(oid, m["verts"], m["faces"])
    with pytest.raises(RuntimeError, match="HipDepthRenderer"):
        bop_eval.average_recall(results, scene_gt, models, cameras, im_width, n_top=1, renderer=ren, depth_images=depth_images, device="cuda")
    small = HipDepthRenderer(W // 2, H // 2)
    for oid, m in models.items():
        small.add_object(oid, m["verts"], m["faces"])
    with pytest.raises(RuntimeError, match="depth image"):
        bop_eval.average_recall(results, scene_gt, models, cameras, im_width, n_top=1, renderer=small, depth_images=depth_images, device="cuda")


def test_chunked_scoring_gives_identical_counts(large):
    from unopose_amd import bop_eval

    models, scene_gt, cameras, results, im_width, depth_images, (W, H) = large
    ren = _renderer(large)
    units = bop_eval.scored_pairs(bop_eval._walk(results, scene_gt, cameras, -1, None))
    whole, n_whole = bop_eval.device_vsd_counts(units, models, ren, depth_images, 15.0, "cuda", chunk_bytes=1 << 40)
    parts, n_parts = bop_eval.device_vsd_counts(units, models, ren, depth_images, 15.0, "cuda", chunk_bytes=40 * 4 * H * W)
    tiny, n_tiny = bop_eval.device_vsd_counts(units, models, ren, depth_images, 15.0, "cuda", chunk_bytes=4 * 4 * H * W)  # splits units too
    assert n_whole == 1 and n_parts >= 4 and n_tiny > n_parts and len(whole) >= 200
    assert sorted(whole) == sorted(parts) == sorted(tiny)
    for k, v in whole.items():
        assert v.dtype == np.int64 and np.array_equal(v, parts[k]) and np.array_equal(v, tiny[k]), k
    a = bop_eval.average_recall(results, scene_gt, models, cameras, im_width, n_top=-1, renderer=ren, depth_images=depth_images, device="cuda",
                                chunk_bytes=40 * 4 * H * W)
    b = bop_eval.average_recall(results, scene_gt, models, cameras, im_width, n_top=-1, renderer=ren, depth_images=depth_images, device="cuda")
    assert a == b


def test_score_csv_device_and_host_agree(large, tmp_path):
    from unopose_amd import bop_eval

    csv, targets = C.write_dataset(str(tmp_path), large)
    host = bop_eval.score_csv(csv, str(tmp_path), "synth", "test", device="cuda", device_scoring=False)
    path = os.path.join(os.path.dirname(csv), "scores_bop19.json")
    assert json.load(open(path))["scorer"] == "host"
    dev = bop_eval.score_csv(csv, str(tmp_path), "synth", "test", device="cuda")
    written = json.load(open(path))
    assert written == json.loads(json.dumps(dev)) and written["scorer"] == "device"
    for k in ("recalls_vsd", "recalls_mssd", "recalls_mspd", "n_targets", "n_estimates", "n_scored_estimates", "n_top", "vsd_delta", "dataset", "split"):
        assert dev[k] == host[k], k
    for k in ("AR_VSD", "AR_MSSD", "AR_MSPD", "AR"):
        assert abs(dev[k] - host[k]) <= 1e-12, k
    assert dev["n_targets"] == sum(len(v) for v in targets.values()) and (6, 1) not in targets and 0.0 < dev["AR"] < 1.0
    assert all(C.large_case_facts(host).values())
    # the targets file decides what is scored: fewer estimates than the file holds, the instance counts bound the selection
    assert dev["n_scored_estimates"] < dev["n_estimates"] and dev["n_top"] == -1


@torch.no_grad()
def test_cli_eval_scores_the_csv_it_wrote(tmp_path, capsys):
    """`python -m unopose_amd.cli ... --eval` on the synthetic provider dataset with models and a targets file added: the CSV, then
    scores_bop19.json beside it and the AR line; the host scorer on the same CSV agrees."""
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
    np.random.seed(11)
    torch.manual_seed(5)
    assert cli.main(["--config-file", str(cfgf), f"misc.load_from={ckpt}", "--eval"]) == 0
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("BOP19 ycbv-test")]
    assert len(line) == 1 and all(k in line[0] for k in ("AR_VSD", "AR_MSSD", "AR_MSPD", " AR "))
    out_dir = tmp_path / "out" / "inference_model_final" / "ycbv"
    csv = out_dir / "result_ycbv-test.csv"
    assert csv.exists() and (out_dir / "scores_bop19.json").exists()
    dev = json.load(open(out_dir / "scores_bop19.json"))
    assert dev["scorer"] == "device" and dev["n_targets"] == 3 and dev["n_estimates"] >= 3 and dev["dataset"] == "ycbv" and dev["vsd_delta"] == 15.0
    host = bop_eval.score_csv(str(csv), root, "ycbv", "test", device="cuda", device_scoring=False)
    for k in ("recalls_vsd", "recalls_mssd", "recalls_mspd"):
        assert dev[k] == host[k], k
    for k in ("AR_VSD", "AR_MSSD", "AR_MSPD", "AR"):
        assert abs(dev[k] - host[k]) <= 1e-12, k
