"""CPU: the colour augmentation split into draw and apply (provider_train.ColorAugmentor.plan / .apply): the numpy operators against
Pillow byte for byte, the generator state, whole chains against augment_image, the device_crops items and their collation."""
import json
import pickle

import numpy as np
import pytest
import torch

import megapose_synth
from color_aug_case import FACTORS, SIDES, SIGMAS, draw_items, host_finish, image, twin_datasets
from unopose_amd import fit as F
from unopose_amd import provider_train as P

ENHANCERS = (("Brightness", P.OP_BRIGHTNESS), ("Contrast", P.OP_CONTRAST), ("Color", P.OP_COLOR), ("Sharpness", P.OP_SHARPNESS))


def _images():
    for h in SIDES:
        for w in SIDES:
            for kind in (0, 1):
                yield (h, w, kind), image(h, w, kind)


def _assert_same(mine, ref, what):
    ref = np.asarray(ref)
    assert mine.dtype == np.uint8 and mine.shape == ref.shape, what
    assert np.array_equal(mine, ref), (what, int(np.abs(mine.astype(int) - ref.astype(int)).max()))


def test_l_conversion_and_smooth_equal_pillow():
    from PIL import Image, ImageFilter

    for tag, img in _images():
        im = Image.fromarray(img)
        _assert_same(P.image_to_l(img), im.convert("L"), ("L", tag))
        _assert_same(P.image_smooth(img), im.filter(ImageFilter.SMOOTH), ("SMOOTH", tag))


def test_blend_equals_pillow_inside_and_outside_the_unit_interval():
    from PIL import Image

    for tag, img in _images():
        other = image(tag[0], tag[1], 0, seed=7)
        for f in FACTORS + (-0.5,):
            ref = Image.blend(Image.fromarray(other), Image.fromarray(img), float(np.float32(f)))
            _assert_same(P.image_blend(other, img, np.float32(f)), ref, ("blend", tag, f))


@pytest.mark.parametrize("name,opcode", ENHANCERS)
def test_enhancement_equals_pillow(name, opcode):
    from PIL import Image, ImageEnhance

    for tag, img in _images():
        enhancer = getattr(ImageEnhance, name)(Image.fromarray(img))
        for f in FACTORS:
            _assert_same(P.ColorAugmentor.apply_op(img, opcode, np.float32(f)), enhancer.enhance(float(np.float32(f))), (name, tag, f))


def test_gaussian_blur_equals_pillow():
    """All sides of SIDES, 1 .. 4 included: nothing has to be left out of a plan for a degenerate size."""
    from PIL import Image, ImageFilter

    assert P.box_blur_weights(np.float32(2.99))[0] == 2 and P.box_blur_weights(np.float32(0.3))[0] == 0  # sides below 2 r + 2 are in SIDES
    for tag, img in _images():
        for sigma in SIGMAS:
            s = float(np.float32(sigma))
            ref = img if s < P.BLUR_MIN_SIGMA else Image.fromarray(img).filter(ImageFilter.GaussianBlur(s))
            _assert_same(P.ColorAugmentor.apply_op(img, P.OP_GAUSSIAN_BLUR, np.float32(sigma)), ref, ("blur", tag, sigma))


def _twins(seed, grayscale=True):
    a, b = P.ColorAugmentor(seed), P.ColorAugmentor(seed)
    if not grayscale:
        for aug in (a, b):
            aug.ops = [o for o in aug.ops if o[1].__name__ != "grayscale"]
    return a, b


def test_plan_leaves_the_generator_where_augment_image_does():
    a, b = _twins(3)
    sizes = np.random.default_rng(1).integers(1, 48, (200, 2))
    seen = set()
    for h, w in sizes:
        a.augment_image(image(int(h), int(w), 0, seed=2))
        plan = b.plan(h, w)
        assert a.rng.bit_generator.state == b.rng.bit_generator.state
        seen.update(op for op, _ in plan.ops)
        for op, params in plan.ops:
            want = {P.OP_COARSE_DROPOUT: np.uint8}.get(op, np.float32)
            assert np.asarray(params).dtype == want
            if op == P.OP_GAUSSIAN_NOISE:
                assert params.shape == (h, w, 3)
    assert seen == set(range(13))
    before = b.rng.bit_generator.state
    assert len(b.plan(0, 5)) == 0 and len(b.plan(4, 0)) == 0 and b.rng.bit_generator.state == before  # a zero-size image draws nothing


def test_apply_equals_augment_image_without_grayscale():
    a, b = _twins(11, grayscale=False)
    sizes = np.random.default_rng(2).integers(1, 72, (120, 2))
    lengths = []
    for k, (h, w) in enumerate(sizes):
        img = image(int(h), int(w), k % 2, seed=k)
        want = a.augment_image(img)
        plan = b.plan(h, w)
        lengths.append(len(plan))
        got = b.apply(img, plan)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (k, h, w, [P.OP_NAMES[op] for op, _ in plan.ops])
    assert max(lengths) >= 8 and min(lengths) <= 2


def test_grayscale_alone_is_within_one_level():
    """The two luma sums (BLAS product in augment_image, elementwise here) are fp32 evaluations of the same three terms: a few ulp apart, so
    the rounded bytes differ by at most one step."""
    a, b = _twins(5)
    worst = 0
    for k in range(40):
        img = image(33 + k, 47, k % 2, seed=k)
        for aug in (a, b):
            aug.rng = np.random.default_rng(k)
        want = a.grayscale(img)
        got = b.apply_op(img, P.OP_GRAYSCALE, b._plan_grayscale(*img.shape[:2]))
        worst = max(worst, int(np.abs(got.astype(int) - want.astype(int)).max()))
    assert worst <= 1


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return megapose_synth.build(str(tmp_path_factory.mktemp("megapose_aug")))


def test_device_items_carry_the_host_items_other_keys_bit_for_bit(tree):
    host, dev = twin_datasets(tree, 5, grayscale=False)
    a, b = draw_items(host, 5, 6), draw_items(dev, 5, 6)
    assert host.color_augmentor.rng.bit_generator.state == dev.color_augmentor.rng.bit_generator.state
    planned = 0
    for x, y in zip(a, b):
        shared = [k for k in x if k not in ("rgb", "tem1_rgb")]
        assert set(y) == set(shared) | {s + t for s in ("rgb_", "tem1_") for t in ("crop", "cropmask", "plan")}
        for k in shared:
            assert x[k].dtype == y[k].dtype and torch.equal(x[k], y[k]), k
        for stem, key in (("rgb_", "rgb"), ("tem1_", "tem1_rgb")):
            crop, mask, plan = y[stem + "crop"], y[stem + "cropmask"], y[stem + "plan"]
            assert crop.dtype == np.uint8 and mask.dtype == np.uint8 and crop.shape == mask.shape + (3,) and isinstance(plan, P.AugPlan)
            assert torch.equal(host_finish(dev, crop, mask, plan), x[key])  # the apply route gives the host item's image
            planned += len(plan) > 0
    assert planned >= 6


def test_global_stream_is_consumed_alike(tree):
    host, dev = twin_datasets(tree, 9)
    draw_items(host, 9, 4)
    state = np.random.get_state()
    draw_items(dev, 9, 4)
    other = np.random.get_state()
    assert state[2] == other[2] and np.array_equal(state[1], other[1])


def test_collation_builds_one_atlas_with_descriptors_and_tables(tree):
    _, dev = twin_datasets(tree, 5)
    items = draw_items(dev, 5, 3)
    batch = P.collate_pairs_device(items, img_size=dev.img_size, rgb_mask_flag=dev.rgb_mask_flag)
    assert set(P.CROP_KEYS) <= set(batch) and "rgb" not in batch and batch["pts"].shape[0] == 3
    desc = batch["crop_desc"].numpy()
    crops = [it["rgb_crop"] for it in items] + [it["tem1_crop"] for it in items]  # queries first, then references
    plans = [it["rgb_plan"] for it in items] + [it["tem1_plan"] for it in items]
    atlas = batch["crop_atlas"].numpy()
    assert atlas.shape == (sum(c.shape[0] for c in crops), max(c.shape[1] for c in crops), 3) and desc.shape == (6, P.AUG_DESC_INTS)
    y = at = 0
    for c, (crop, plan) in enumerate(zip(crops, plans)):
        y0, h, w, length, first = desc[c, :5]
        assert (y0, h, w, length, first) == (y, crop.shape[0], crop.shape[1], len(plan), at)
        assert np.array_equal(atlas[y0:y0 + h, :w], crop) and not atlas[y0:y0 + h, w:].any()
        assert batch["crop_ops"].numpy()[first:first + length, 0].tolist() == [op for op, _ in plan.ops]
        y, at = y + h, at + len(plan)
    assert batch["crop_masks"].numel() == sum(c.shape[0] * c.shape[1] for c in crops) and batch["crop_rows"].numel() == atlas.shape[0]
    assert int(batch["crop_rows"].sum()) == int(batch["crop_masks"].sum()) and batch["crop_cfg"].tolist() == [dev.img_size, 1]
    loader = F.build_loader(dev, 2, workers=0, seed=5)
    assert pickle.loads(pickle.dumps(loader.collate_fn)).keywords == dict(img_size=dev.img_size, rgb_mask_flag=True)  # spawned workers
    assert loader.collate_fn.func is P.collate_pairs_device and F.build_loader(twin_datasets(tree, 5)[0], 2, workers=0).collate_fn is P.collate_pairs


def test_pack_plans_refuses_what_does_not_fit():
    plan = P.AugPlan(4, 5, [(P.OP_GAUSSIAN_NOISE, np.zeros((4, 5, 3), np.float32))])
    with pytest.raises(ValueError):
        P.pack_plans([(0, 5, 4)], [plan])
    with pytest.raises(ValueError):
        P.pack_plans([(0, 4, 5)], [P.AugPlan(4, 5, [(99, np.float32(1))])])
    desc, ops, grids, noise = P.pack_plans([(0, 4, 5), (4, 2, 2)], [plan, None])
    assert desc[:, 3].tolist() == [1, 0] and ops.shape == (1, P.AUG_ENTRY_INTS) and noise.size == 60 and grids.size == 1


def test_fit_command_line_selects_the_route(tmp_path, capsys):
    cfg = {"train": {}, "dataloader": {"train": {"dataset": {"cfg": {}}}}, "misc": {"output_dir": "/somewhere"}, "model": {}}
    path = tmp_path / "cfg.json"
    path.write_text(json.dumps(cfg))

    def plan(*argv):
        assert F.main(["--config", str(path), "--print-plan", *argv]) == 0
        return json.loads(capsys.readouterr().out)

    assert plan()["device_crops"] is False and plan("--device-crops")["device_crops"] is True
    assert plan("dataloader.train.device_crops=true")["device_crops"] is True
