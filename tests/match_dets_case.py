"""Shared inputs of the match_dets tests: a brute-force patch validity, hand-made token sets, the bop_synth dataset extended by one image
whose target lists its own view as the reference, a proposal file for it, and a token function that needs no GPU."""
import json
import os.path as osp

import numpy as np
import torch

import bop_synth
from unopose_amd.provider import rle_counts_to_string, rle_encode

TARGETS_NAME = "match_dets_ref_targets.json"
SELF_IMAGE = 3  # scene 48: the image that is its own reference
SELF_BLOB = (48, 60, 20, 26)


def brute_patch_valid(mask, img_size):
    """The rule of match_dets.patch_valid_host, pixel by pixel."""
    mask = np.asarray(mask)
    s, side = mask.shape[0], img_size // 14
    out = np.zeros(side * side, dtype=np.uint8)
    for r in range(side):
        for c in range(side):
            cnt = 0
            for dy in range(14):
                for dx in range(14):
                    Y, X = r * 14 + dy, c * 14 + dx
                    cnt += bool(mask[Y * s // img_size, X * s // img_size])
            out[r * side + c] = 2 * cnt >= 196
    return out


def validity_masks(s, img_size, seed=0):
    """Window masks of side s for `img_size`: empty, full, random, a half plane and, where the window is the crop itself, patches holding
    exactly 98 and 97 set pixels (2 cnt = 196 and 194)."""
    rs = np.random.RandomState(1000 * s + img_size + seed)
    masks = [np.zeros((s, s), bool), np.ones((s, s), bool), rs.rand(s, s) < 0.5, np.tril(np.ones((s, s), bool)), rs.rand(s, s) < 0.48,
             rs.rand(s, s) < 0.52]
    if s == img_size:
        m = np.zeros((s, s), bool)
        m[:7, :14] = True  # patch (0, 0): 98 pixels
        m[14:21, 14:28] = True
        m[20, 27] = False  # patch (1, 1): 97 pixels
        masks.append(m)
    return masks


def one_hot_tokens(rows, D=32):
    """(5 + T, D) float32 tokens whose row t is the unit vector rows[t] (-1: a zero row)."""
    t = np.zeros((len(rows), D), dtype=np.float32)
    for i, k in enumerate(rows):
        if k >= 0:
            t[i, k] = 1.0
    return t


def fake_tokens(crops, D=32):
    """crops (B, 3, S, S) -> (B, 5 + T, D) float32: per patch a fixed random projection of its mean colour and position, the class token
    from the crop's mean; a deterministic stand-in for the ViT on machines without a GPU."""
    crops = torch.as_tensor(crops, dtype=torch.float32).cpu()
    B, _, S, _ = crops.shape
    side = S // 14
    g = torch.Generator().manual_seed(7)
    proj = torch.randn(5, D, generator=g)
    pm = crops.reshape(B, 3, side, 14, side, 14).mean(dim=(3, 5)).permute(0, 2, 3, 1).reshape(B, side * side, 3)
    pos = torch.stack(torch.meshgrid(torch.linspace(-1, 1, side), torch.linspace(-1, 1, side), indexing="ij"), -1).reshape(1, side * side, 2).expand(B, -1, -1)
    patches = torch.cat([pm, 0.1 * pos], dim=2) @ proj
    cls = (torch.cat([crops.mean(dim=(2, 3)), torch.zeros(B, 2)], dim=1) @ proj)[:, None]
    return torch.cat([cls, torch.zeros(B, 4, D), patches], dim=1)


def _seg(mask, as_string):
    seg = rle_encode(mask)
    return {"size": seg["size"], "counts": rle_counts_to_string(seg["counts"])} if as_string else seg


def build(root):
    """bop_synth's dataset under `root` plus scene 48 image 3 (one object, depth without holes, its own reference) -> (cfg, proposals path,
    proposals).  At most 12 proposals: the dataset's detector blobs, shifted near-duplicates, a rectangle across both objects of image 1,
    a speck that the minimum-count rule drops, the self-reference mask, and one proposal of an image without a target."""
    cfg, _ = bop_synth.build(root)
    H, W = bop_synth.H, bop_synth.W
    folder = osp.join(root, "ycbv", "test", "000048")
    rs = np.random.RandomState(77)
    own = bop_synth._blob(*SELF_BLOB)
    yy, xx = np.mgrid[0:H, 0:W]
    depth = np.zeros((H, W), np.uint16)
    depth[own] = (5000 + 0.3 * (xx - 60) + 0.1 * (yy - 48))[own].astype(np.uint16)
    bop_synth._write_png(osp.join(folder, "rgb", f"{SELF_IMAGE:06d}.png"), rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8))
    bop_synth._write_png(osp.join(folder, "depth", f"{SELF_IMAGE:06d}.png"), depth)
    bop_synth._write_png(osp.join(folder, "mask_visib", f"{SELF_IMAGE:06d}_000000.png"), (own * 255).astype(np.uint8))
    cam = json.load(open(osp.join(folder, "scene_camera.json")))
    gt = json.load(open(osp.join(folder, "scene_gt.json")))
    cam[str(SELF_IMAGE)] = dict(cam["1"])
    gt[str(SELF_IMAGE)] = [{"cam_R_m2c": [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0], "cam_t_m2c": [0.0, 0.0, 5000.0], "obj_id": 2}]
    json.dump(cam, open(osp.join(folder, "scene_camera.json"), "w"))
    json.dump(gt, open(osp.join(folder, "scene_gt.json"), "w"))
    targets = json.load(open(osp.join(root, "ycbv", bop_synth.CFG["ref_targets_name"])))
    targets.append(dict(scene_id=48, im_id=SELF_IMAGE, obj_id=2, ref_scene_id=48, ref_im_id=SELF_IMAGE))
    json.dump(targets, open(osp.join(root, "ycbv", TARGETS_NAME), "w"))

    a, b, c = (40, 40, 22, 17), (55, 95, 14, 25), (10, 118, 16, 14)
    det = lambda cy, cx, ry, rx, dy=0, dx=0: bop_synth._blob(cy + 1 + dy, cx - 1 + dx, ry + 2, rx + 1)  # noqa: E731
    rect, speck = np.zeros((H, W), bool), np.zeros((H, W), bool)
    rect[22:72, 30:112] = True
    speck[40:42, 40:43] = True
    props = [
        dict(scene_id=48, image_id=1, segmentation=_seg(det(*a), False), bbox=[1, 2, 3, 4], time=0.25),
        dict(scene_id=48, image_id=1, segmentation=_seg(det(*b), True), time=0.25),
        dict(scene_id=48, image_id=1, segmentation=_seg(det(*a, 3, 2), True), bbox=[5, 6, 7, 8]),
        dict(scene_id=48, image_id=1, segmentation=_seg(det(*b, -2, 3), False), extra="ignored"),
        dict(scene_id=48, image_id=1, segmentation=_seg(rect, False)),
        dict(scene_id=48, image_id=1, segmentation=_seg(speck, False)),
        dict(scene_id=48, image_id=2, segmentation=_seg(det(*c), False), time=0.5),
        dict(scene_id=48, image_id=2, segmentation=_seg(det(*c, 2, -3), True), time=0.5),
        dict(scene_id=48, image_id=SELF_IMAGE, segmentation=_seg(own, True)),
        dict(scene_id=48, image_id=9, segmentation=_seg(rect, False)),
    ]
    path = osp.join(root, "proposals.json")
    json.dump(props, open(path, "w"))
    return dict(cfg, ref_targets_name=TARGETS_NAME), path, props
