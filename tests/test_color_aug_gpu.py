"""GPU: ops.color_augment (csrc/coloraug.hip) against ColorAugmentor.apply byte for byte, ops.finish_crops against the host loader's
batches, and a short `fit --device-crops` run on the synthetic MegaPose tree."""
import itertools
import json
import os

import numpy as np
import pytest
import torch

import megapose_synth
from color_aug_case import GPU_CROPS, chain_plan, draw_items, host_finish, image, params_for, twin_datasets
from unopose_amd import provider_train as P

pytestmark = pytest.mark.gpu

ALL_OPS = tuple(range(13))
ORDERS = (ALL_OPS, ALL_OPS[::-1], (3, 10, 1, 0, 12, 7, 2, 9, 5, 11, 4, 8, 6))


def _crops(seed=0):
    return [image(h, w, k % 2, seed=seed + k) for k, (h, w) in enumerate(GPU_CROPS)]


def _run(crops, plans, **kw):
    from unopose_amd import ops

    atlas, boxes = P.build_atlas(crops)
    done = ops.color_augment(torch.from_numpy(atlas).cuda(), boxes, plans, **kw).cpu().numpy()
    return [done[y0:y0 + h, :w] for y0, h, w in boxes], done, atlas


def _expect(crops, plans):
    aug = P.ColorAugmentor()
    return [aug.apply(c, p) if p is not None else c for c, p in zip(crops, plans)]


def _check(got, want, plans):
    for k, (g, w, p) in enumerate(zip(got, want, plans)):
        names = [] if p is None else [P.OP_NAMES[op] for op, _ in p.ops]
        assert np.array_equal(g, w), (k, g.shape, names, int(np.abs(g.astype(int) - w.astype(int)).max()))


@pytest.mark.parametrize("opcode", ALL_OPS)
def test_single_operator_equals_apply(opcode):
    """One atlas of crops with sides 2, 3, 5, 6, 65, 130 x 67, ... : padding right of the narrow ones; sides below 2 r + 2 take the blur's
    clamped indices on both ends at once.  Three parameter variants per operator (blend inside and outside [0, 1], blur radii 0 .. 2)."""
    crops = _crops(opcode)
    for variant in range(3):
        rng = np.random.default_rng([opcode, variant])
        plans = [P.AugPlan(c.shape[0], c.shape[1], [(opcode, params_for(opcode, c.shape[0], c.shape[1], rng, variant + k))]) for k, c in enumerate(crops)]
        got, done, atlas = _run(crops, plans)
        _check(got, _expect(crops, plans), plans)
        for (y0, h, w) in P.build_atlas(crops)[1]:
            assert not done[y0:y0 + h, w:].any()  # the padding of a fresh result is zero


def test_full_chains_in_three_orders_an_empty_chain_and_late_tables():
    crops = _crops(40)
    # crops 0 .. 2: all thirteen operators in three orders; 3: empty; 4: None; 5: noise and dropout blocks that are not the first of their
    # tables (crops 0 .. 2 own earlier ones) behind a second dropout of its own; 6, 7: short chains ending at different positions
    plans = [chain_plan(c.shape[0], c.shape[1], ORDERS[k], seed=k) for k, c in enumerate(crops[:3])]
    plans += [P.AugPlan(6, 6), None]
    h, w = crops[5].shape[:2]
    rng = np.random.default_rng(8)
    plans.append(P.AugPlan(h, w, [(P.OP_COARSE_DROPOUT, params_for(P.OP_COARSE_DROPOUT, h, w, rng)), (P.OP_GAUSSIAN_BLUR, np.float32(2.5)),
                                  (P.OP_COARSE_DROPOUT, params_for(P.OP_COARSE_DROPOUT, h, w, rng)), (P.OP_CONTRAST, np.float32(0.6)),
                                  (P.OP_GAUSSIAN_NOISE, params_for(P.OP_GAUSSIAN_NOISE, h, w, rng)), (P.OP_CONTRAST, np.float32(3.0))]))
    plans.append(chain_plan(3, 70, (1, 3), seed=5))
    plans.append(chain_plan(1, 4, (2, 1, 12), seed=6))
    want = _expect(crops, plans)
    got, _, atlas = _run(crops, plans)
    _check(got, want, plans)
    # into a caller's buffer, from packed tables: the same bytes, and the atlas is only read
    from unopose_amd import ops

    boxes = P.build_atlas(crops)[1]
    dev_atlas = torch.from_numpy(atlas).cuda()
    out = torch.full_like(dev_atlas, 7)
    assert ops.color_augment(dev_atlas, None, P.pack_plans(boxes, plans), out=out) is out
    res = out.cpu().numpy()
    _check([res[y0:y0 + h, :w] for y0, h, w in boxes], want, plans)
    assert torch.equal(dev_atlas.cpu(), torch.from_numpy(atlas))
    # every chain empty: one copy-through launch
    got, _, _ = _run(crops, [None] * len(crops))
    _check(got, crops, [None] * len(crops))


def test_tables_are_checked_before_anything_is_launched():
    from unopose_amd import ops

    crops = _crops(3)[:2]
    atlas, boxes = P.build_atlas(crops)
    dev = torch.from_numpy(atlas).cuda()
    plans = [chain_plan(c.shape[0], c.shape[1], (0, 10, 3), seed=1) for c in crops]
    desc, entries, grids, noise = P.pack_plans(boxes, plans)
    for change in ("rows", "width", "chain", "opcode", "grid", "noise", "slot", "overlap"):
        d, e = desc.copy(), entries.copy()
        if change == "rows":
            d[1, 1] += 1
        elif change == "width":
            d[1, 2] = atlas.shape[1] + 1
        elif change == "chain":
            d[1, 3] += 1
        elif change == "opcode":
            e[0, 0] = 13
        elif change == "grid":
            e[3, 3] += 1
        elif change == "noise":
            e[4, 1] += 1
        elif change == "slot":
            e[5, 2] = 5
        else:
            d[1, 0] -= 1
        with pytest.raises(ValueError):
            ops.color_augment(dev, None, (d, e, grids, noise))
    with pytest.raises(RuntimeError):
        ops.color_augment(torch.from_numpy(atlas), boxes, plans)  # no CPU path
    big = P.AugPlan(2, 1400, [(P.OP_GAUSSIAN_BLUR, np.float32(1.0))])
    with pytest.raises(ValueError):
        ops.color_augment(torch.zeros(2, 1400, 3, dtype=torch.uint8, device="cuda"), [(0, 2, 1400)], [big])


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return megapose_synth.build(str(tmp_path_factory.mktemp("megapose_aug_gpu")))


def test_finish_crops_equals_the_host_loaders_batch(tree):
    """Without grayscale the device batch is the host loader's batch; with it, the batch of `apply`-based host finishing."""
    from unopose_amd import ops
    from unopose_amd.fit import build_loader

    for grayscale in (False, True):
        host, dev = twin_datasets(tree, 5, grayscale=grayscale)
        batches = []
        for ds in (host, dev):
            np.random.seed(5)
            ds.reset()
            batches.append(next(iter(build_loader(ds, 2, workers=0, seed=5))))
        want, raw = batches
        got = ops.finish_crops(raw, "cuda")
        assert set(got) == set(want) and all(v.is_cuda for v in got.values())
        for k in want:
            if k not in ("rgb", "tem1_rgb"):
                assert torch.equal(got[k].cpu(), want[k]), k
        assert got["rgb"].shape == want["rgb"].shape == (2, 3, 56, 56) and got["rgb"].dtype == torch.float32
        if grayscale:  # the same items again, finished on the host through apply
            np.random.seed(5)
            dev2 = twin_datasets(tree, 5)[1]
            dev2.reset()
            order = list(itertools.islice(iter(build_loader(dev2, 2, workers=0, seed=5).sampler), 2))
            items = [dev2[i] for i in order]
            want = {key: torch.stack([host_finish(dev2, it[stem + "crop"], it[stem + "cropmask"], it[stem + "plan"]) for it in items])
                    for stem, key in (("rgb_", "rgb"), ("tem1_", "tem1_rgb"))}
        assert torch.equal(got["rgb"].cpu(), want["rgb"]) and torch.equal(got["tem1_rgb"].cpu(), want["tem1_rgb"])
        assert len(raw["crop_ops"]) > 1  # the batch did hold augmentation chains


def test_fit_runs_three_iterations_with_device_crops(tmp_path, tree):
    from oracle.unopose_ref import default_cfg, random_state_dict  # weights only
    from unopose_amd import fit as F
    from unopose_amd.model import default_model_cfg

    torch.save(random_state_dict(default_cfg(), seed=0, tame=0.1), tmp_path / "init.pth")
    data = dict(tree, img_size=224, n_sample_observed_point=512, n_sample_template_point=1200)
    cfg = {"train": {"max_iter": 3, "log_period": 1, "seed": 3, "checkpointer": {"period": 100}, "clip_grad": {"enabled": True, "params": {"max_norm": 35}}},
           "dataloader": {"train": {"batch_size": 2, "dataset": {"cfg": data, "num_img_per_epoch": 8}}},
           "model": {"cfg": dict(default_model_cfg(fine_npoint=512))}, "misc": {"load_from": str(tmp_path / "init.pth")}}
    (tmp_path / "cfg.json").write_text(json.dumps(cfg))
    out = tmp_path / "run"
    assert F.main(["--config", str(tmp_path / "cfg.json"), "--output-dir", str(out), "--device-crops", "--workers", "0", "--seed", "3"]) == 0
    lines = [json.loads(line) for line in open(out / "metrics.json")]
    assert [r["iteration"] for r in lines] == [0, 1, 2] and all(np.isfinite(r["total_loss"]) and np.isfinite(r["total_grad_norm"]) for r in lines)
    assert os.path.exists(out / "model_final.pth") and open(out / "last_checkpoint").read() == "model_final.pth"
