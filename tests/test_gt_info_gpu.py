"""GPU: the ground-truth visibility on the device -- csrc/gtinfo.hip through `ops.score.gt_visibility` against `gt_info.gt_counts_host` on
the same HIP renders (all 11 integers and both masks equal), over the image sizes at which the kernel takes another path, and end to
end: `compute_gt_info` on the device against the host route, `score_csv` computing the visibility against reading the written files, and
the provider reading a written `mask_visib`."""
import json
import os

import numpy as np
import pytest
import torch

import gt_info_case as C

pytestmark = pytest.mark.gpu

# H x W: 16-byte loads; 4-byte loads with the crop's edges inside a would-be vector; 16-byte loads over rows that start on any 8-byte
# boundary (W % 4 == 2: vectors straddle row ends and both edges of the crop); the degenerate ones
SIZES = [(24, 36), (23, 35), (24, 34), (1, 4), (5, 1)]


def _renderer(W, H):
    from unopose_amd.render import HipDepthRenderer

    ren = HipDepthRenderer(3 * W, 3 * H)
    for obj_id, m in C.make_models().items():
        ren.add_object(obj_id, m["verts"], m["faces"])
    return ren


def _host(test, canvas, K4, delta):
    """`gt_counts_host` per ground truth -> (rows (G, 11) int64, masks (G, H, W) uint8, visible masks)."""
    from unopose_amd.gt_info import gt_counts_host

    rows, ms, mvs = [], [], []
    for t, c, k, d in zip(test, canvas, K4, delta):
        row, m, mv = gt_counts_host(t, c, np.array([[k[0], 0, k[2]], [0, k[1], k[3]], [0, 0, 1.0]]), d)
        rows.append(row), ms.append(m.astype(np.uint8) * 255), mvs.append(mv.astype(np.uint8) * 255)
    return torch.tensor(rows, dtype=torch.int64), torch.from_numpy(np.stack(ms)), torch.from_numpy(np.stack(mvs))


def _assert_equal(got, want, what):
    for g, w, name in zip(got, want, ("integers", "mask", "mask_visib")):
        assert g.dtype == w.dtype and torch.equal(g.cpu(), w), (what, name, g.cpu()[:4], w[:4])


def _scene_launch(W, H, images=None):
    """The fixture scenes at W x H on HIP renders -> test stack, canvas stack, per ground truth: test index, K4."""
    ren = _renderer(W, H)
    scene_gt, cameras, depth_images, canvases = C.make_scenes(lambda *a: ren.render_object(*a)["depth"], W, H, images=images)
    order = [(sid, iid) for sid, ims in scene_gt.items() for iid in ims]
    test = np.stack([depth_images[sid][iid] for sid, iid in order])
    keys = list(canvases)
    canvas = np.stack([canvases[k] for k in keys])
    image_index = np.array([order.index(k[:2]) for k in keys])
    K4 = np.array([[cameras[k[0]][k[1]][0, 0], cameras[k[0]][k[1]][1, 1], cameras[k[0]][k[1]][0, 2], cameras[k[0]][k[1]][1, 2]] for k in keys])
    return test, canvas, image_index, K4


@pytest.mark.parametrize("H,W", SIZES)
def test_fixture_scenes_equal_the_host(H, W):
    from unopose_amd import ops

    test, canvas, image_index, K4 = _scene_launch(W, H)
    G = len(canvas)
    assert G == 10 and len(test) == 3
    want = _host(test[image_index], canvas, K4, [C.DELTA] * G)
    if (H, W) == (24, 36):
        assert (want[0][:, 0] > 0).sum() == 9 and (want[0][:, 2] == 0).sum() == 3 and (want[0][:, 3] < 0).any()  # the scenes are the fixture's
    t_dev, c_dev = torch.from_numpy(test).cuda(), torch.from_numpy(canvas).cuda()
    # every ground truth in one launch that spans the three test images, in shuffled order
    perm = np.random.RandomState(0).permutation(G)
    got = ops.gt_visibility(t_dev, c_dev, K4[perm], C.DELTA, image_index=image_index[perm], canvas_index=perm, masks=True)
    _assert_equal(got, [w[perm] for w in want], "shuffled")
    rows = ops.gt_visibility(t_dev, c_dev, K4[perm], np.full(G, C.DELTA), image_index=image_index[perm], canvas_index=perm)
    assert torch.equal(rows.cpu(), want[0][perm])  # without masks, delta per ground truth
    # one ground truth per launch, default indices
    for g in range(G):
        got = ops.gt_visibility(t_dev[image_index[g]][None], c_dev[g][None], K4[g], C.DELTA, masks=True)
        _assert_equal(got, [w[g:g + 1] for w in want], g)


@pytest.mark.parametrize("H,W", SIZES)
def test_random_maps_equal_the_host(H, W):
    """Maps no renderer would draw: a silhouette pixel anywhere on the canvas, the crop's border rows and columns included, test depth on
    both sides of the tolerance, holes, a canvas stack that does not start on a 16-byte boundary."""
    from unopose_amd import ops

    rs = np.random.RandomState(H * 100 + W)
    G, n_test = 5, 2
    canvas = np.where(rs.rand(G, 3 * H, 3 * W) < 0.45, rs.uniform(600, 900, (G, 3 * H, 3 * W)), 0.0).astype(np.float32)
    canvas[0], canvas[1] = 0.0, 750.0  # an empty canvas, a full one
    test = np.where(rs.rand(n_test, H, W) < 0.2, 0.0, rs.uniform(600, 900, (n_test, H, W))).astype(np.float32)
    K4 = np.stack([[30.0 + g, 31.0, W / 2.0 - 0.3 * g, H / 2.0 + 0.1] for g in range(G)])
    image_index, delta = rs.randint(0, n_test, G), [15.0, 5.0, np.float64(15.0), 0.0, 40.0]
    want = _host(test[image_index], canvas, K4, delta)
    assert want[0][0, 0] == 0 and want[0][1, 0] == 9 * H * W and (want[0][2:, 2] < want[0][2:, 0]).all()
    t_dev = torch.from_numpy(test).cuda()
    got = ops.gt_visibility(t_dev, torch.from_numpy(canvas).cuda(), K4, delta, image_index=image_index, masks=True)
    _assert_equal(got, want, "aligned")
    shifted = torch.empty(canvas.size + 1, dtype=torch.float32, device="cuda")[1:].view(canvas.shape)
    shifted.copy_(torch.from_numpy(canvas))
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    got = ops.gt_visibility(t_dev, shifted, K4, delta, image_index=image_index, masks=True)
    _assert_equal(got, want, "shifted")


def test_real_size_launch_equals_the_host():
    from unopose_amd import ops

    test, canvas, image_index, K4 = _scene_launch(640, 480, images=[(1, 1)])
    assert canvas.shape == (3, 1440, 1920)
    want = _host(test[image_index], canvas, K4, [C.DELTA] * 3)
    assert (want[0][:, 0] > 10000).all() and 0 < want[0][1, 2] < 0.1 * want[0][1, 0] and want[0][2, 2] == 0
    got = ops.gt_visibility(torch.from_numpy(test).cuda(), torch.from_numpy(canvas).cuda(), K4, C.DELTA, image_index=image_index, masks=True)
    _assert_equal(got, want, "480 x 640")


def test_bad_arguments_raise():
    from unopose_amd import ops

    test, canvas = torch.zeros(1, 4, 8, device="cuda"), torch.zeros(2, 12, 24, device="cuda")
    K4 = [10.0, 10.0, 4.0, 2.0]
    assert ops.gt_visibility(test, canvas, K4, 15.0, image_index=[0, 0]).shape == (2, 11)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        ops.gt_visibility(test.cpu(), canvas, K4, 15.0, image_index=[0, 0])
    with pytest.raises(RuntimeError, match="expected"):
        ops.gt_visibility(test, torch.zeros(2, 12, 23, device="cuda"), K4, 15.0, image_index=[0, 0])
    with pytest.raises(ValueError, match="image_index"):
        ops.gt_visibility(test, canvas, K4, 15.0)  # two ground truths, one test image
    with pytest.raises(ValueError, match="canvas_index"):
        ops.gt_visibility(test, canvas, K4, 15.0, image_index=[0], canvas_index=[2])
    with pytest.raises(RuntimeError, match="float32"):
        ops.gt_visibility(test, canvas.double(), K4, 15.0, image_index=[0, 0])


# ---- end to end, on a tests/bop_scenes.py dataset -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    import bop_scenes

    root = str(tmp_path_factory.mktemp("bop"))
    cfg, det_path = bop_scenes.build(root, n_images=1, dets_per_image=(1, 1))
    csv, sid = C.extend_bop_scenes(root)
    return root, cfg, det_path, csv, sid


def test_device_route_equals_the_host_route(dataset):
    import bop_scenes
    from unopose_amd import bop_eval, gt_info
    from unopose_amd.render import HipDepthRenderer

    root, _, _, _, sid = dataset
    data = bop_eval.load_dataset(root, "lm", "test")
    ren = HipDepthRenderer(3 * bop_scenes.W, 3 * bop_scenes.H)
    for obj_id, m in data["models"].items():
        ren.add_object(obj_id, m["verts"], m["faces"])
    part = {sid: {iid: data["scene_gt"][sid][iid] for iid in sorted(data["scene_gt"][sid])[:5]}}  # 5 images, 8 ground truths of 5 objects
    a = (part, data["cameras"], data["depth_images"], ren, 15.0)
    host, host_masks = gt_info.compute_gt_info(*a, masks=True)
    dev, dev_masks = gt_info.compute_gt_info(*a, device="cuda", masks=True)
    assert dev == host and sum(len(v) for v in host[sid].values()) == 8
    for iid, pairs in host_masks[sid].items():
        for (m, mv), (dm, dmv) in zip(pairs, dev_masks[sid][iid]):
            assert np.array_equal(m, dm) and np.array_equal(mv, dmv) and dm.dtype == bool
    assert any(0 < e["visib_fract"] < 1 for v in host[sid].values() for e in v) and any(e["visib_fract"] == 1.0 for v in host[sid].values() for e in v)
    # a budget of 22 images = two ground truths (9 each) and their images: four chunks, the third image's depth shared by two of them
    rows, chunks = gt_info._device_rows(gt_info._flat(part, data["cameras"]), data["depth_images"], ren, 15.0, "cuda", False,
                                        chunk_bytes=22 * 4 * bop_scenes.H * bop_scenes.W)
    assert chunks == 4 and [gt_info.info_from_counts(r) for r, _ in rows] == [e for iid in part[sid] for e in host[sid][iid]]
    assert gt_info.compute_gt_info(*a, device="cuda") == host  # without masks
    with pytest.raises(RuntimeError, match="no fallback"):
        gt_info.compute_gt_info(part, data["cameras"], data["depth_images"], object(), 15.0, device="cuda")


def test_score_csv_computes_what_the_written_files_say_and_the_provider_reads_them(dataset):
    import bop_scenes
    from unopose_amd import bop_eval, gt_info
    from unopose_amd import provider as P
    from unopose_amd.render import HipDepthRenderer

    root, cfg, det_path, csv, sid = dataset
    written = gt_info.write_gt_info(root, "lm", "test", scene_ids=[sid], overwrite=True)  # bop_scenes wrote a mask_visib of its own
    scores = os.path.join(os.path.dirname(csv), "scores_bop19.json")
    from_file = bop_eval.score_csv(csv, root, "lm", "test", gt_visibility="file")
    assert json.load(open(scores))["gt_visibility"] == "file"
    computed = bop_eval.score_csv(csv, root, "lm", "test", gt_visibility="compute")
    assert json.load(open(scores))["gt_visibility"] == "compute" and computed["gt_delta"] == 15.0 and "gt_delta" not in from_file
    drop = lambda d: {k: v for k, v in d.items() if k not in ("gt_visibility", "gt_delta")}  # noqa: E731
    assert drop(computed) == drop(from_file) and computed["scorer"] == "device" and computed["AR_VSD"] is not None
    on_host = bop_eval.score_csv(csv, root, "lm", "test", gt_visibility="compute", device_scoring=False, error_types="mssd,mspd")
    assert on_host["recalls_mssd"] == computed["recalls_mssd"]
    off = bop_eval.score_csv(csv, root, "lm", "test")
    assert "gt_visibility" not in off and off["AR_MSSD"] != computed["AR_MSSD"]  # the farther, better-found instances are no targets under the rule
    # a reference view from the written mask: its pixels are the visible mask of the object's first ground truth inside the view's square
    # window (which drops a last row or column of an odd extent)
    data = bop_eval.load_dataset(root, "lm", "test")
    canvas = HipDepthRenderer(3 * bop_scenes.W, 3 * bop_scenes.H)
    for obj_id, m in data["models"].items():
        canvas.add_object(obj_id, m["verts"], m["faces"])
    ds = P.BOPTestsetOneRef(cfg, "lm", det_path)
    for obj_id in (1, 2, 7):
        view = ds.ref_views.get(os.path.join(root, "lm", "test"), sid, obj_id, obj_id)
        _, held = gt_info.compute_gt_info({sid: {obj_id: data["scene_gt"][sid][obj_id]}}, data["cameras"], data["depth_images"], canvas, 15.0, device="cuda", masks=True)
        visible = held[sid][obj_id][0][1]
        assert visible.sum() == written[sid][obj_id][0]["px_count_visib"] > 500
        assert view is not None and np.array_equal(view["pixels"], np.flatnonzero(view["window"].crop(visible))) and len(view["pixels"]) > 0.98 * visible.sum()
