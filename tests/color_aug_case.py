"""Shared inputs of the colour-augmentation tests (tests/test_color_aug_cpu.py, tests/test_color_aug_gpu.py): test images, plans with
one entry per operator, full chains in a given order, twin datasets on the synthetic MegaPose tree and the host finishing of a device item
through `ColorAugmentor.apply`."""
import numpy as np
import torch

from unopose_amd import provider_train as P
from unopose_amd.provider import resize_bilinear_u8, to_tensor_normalize

SIDES = (1, 2, 3, 5, 6, 64, 89)
SIGMAS = (0.0005, 0.3, 1.0, 2.99)
FACTORS = (0.0, 0.37, 1.0, 1.7, 20.5, 49.0)  # blend at 0 <= f <= 1 (both ends included) and f > 1
GPU_CROPS = ((2, 2), (3, 3), (5, 5), (6, 6), (65, 65), (130, 67), (3, 70), (1, 4))  # (h, w): mixed widths, so the atlas has padding


def image(h, w, kind, seed=0):
    """kind 0: random bytes; 1: a gradient with different slopes per channel (wraps at 256)."""
    if kind == 0:
        return np.random.default_rng([seed, h, w]).integers(0, 256, (h, w, 3), dtype=np.uint8)
    return (np.add.outer(np.arange(h) * 3, np.arange(w) * 2)[:, :, None] * np.array([1, 2, 3]) % 256).astype(np.uint8)


def params_for(opcode, h, w, rng, variant=0):
    """Parameters of one plan entry inside the augmentor's ranges; `variant` walks the special values of the operator."""
    f32 = np.float32
    if opcode == P.OP_COARSE_DROPOUT:
        grid = (rng.random((max(3, int(round(h * 0.05))), max(3, int(round(w * 0.05))))) < 0.4).astype(np.uint8)
        grid[0, 0], grid[-1, -1] = 1, 0
        return grid
    if opcode == P.OP_GAUSSIAN_BLUR:
        return f32((0.3, 1.0, 2.99, 1.7)[variant % 4])
    if opcode in (P.OP_SHARPNESS, P.OP_CONTRAST, P.OP_BRIGHTNESS, P.OP_COLOR):
        return f32((0.37, 1.7, 0.0, 1.0, 20.5, 49.0)[variant % 6])
    if opcode == P.OP_ADD:
        return rng.integers(-25, 26, 3).astype(f32)
    if opcode == P.OP_INVERT:
        return np.array([(1, 0, 1), (0, 1, 0), (1, 1, 1), (0, 0, 0)][variant % 4], f32)
    if opcode in (P.OP_MULTIPLY_PC, P.OP_MULTIPLY):
        return rng.uniform(0.6, 1.4, 3).astype(f32)
    if opcode == P.OP_GAUSSIAN_NOISE:
        return rng.normal(0.0, 10.0, (h, w, 3)).astype(f32)
    if opcode == P.OP_LINEAR_CONTRAST:
        return rng.uniform(0.5, 2.2, 3).astype(f32)
    if opcode == P.OP_GRAYSCALE:
        return f32(rng.uniform(0.0, 1.0))
    raise ValueError(opcode)


def chain_plan(h, w, order, seed):
    rng = np.random.default_rng(seed)
    return P.AugPlan(h, w, [(op, params_for(op, h, w, rng, variant=seed + k)) for k, op in enumerate(order)])


def twin_datasets(tree, seed, grayscale=True, num=8):
    """(host dataset, device_crops dataset) with equal seeds; grayscale=False removes that operator from both augmentors."""
    out = []
    for device_crops in (False, True):
        ds = P.MegaPoseOneRefTrainSet(tree, num_img_per_epoch=num, color_augmentor="default", seed=seed, device_crops=device_crops)
        if not grayscale:
            ds.color_augmentor.ops = [o for o in ds.color_augmentor.ops if o[1].__name__ != "grayscale"]
        out.append(ds)
    return out


def draw_items(ds, seed, count):
    np.random.seed(seed)
    ds.reset()
    return [ds[i] for i in range(count)]


def host_finish(ds, crop, mask, plan):
    """`MegaPoseOneRefTrainSet._crop_tensor` behind the window crop, with `ColorAugmentor.apply` in place of `augment_image`."""
    rgb = P.ColorAugmentor().apply(crop, plan)
    if ds.rgb_mask_flag:
        rgb = rgb * (mask[:, :, None] > 0).astype(np.uint8)
    return torch.FloatTensor(to_tensor_normalize(resize_bilinear_u8(np.ascontiguousarray(rgb), ds.img_size)))
