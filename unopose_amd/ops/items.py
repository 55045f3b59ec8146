"""Training items from rendered views on the device (csrc/train_items.hip): the per-pixel and per-point work of
`provider_online.items_from_views_host` for all views of a chunk of (query, reference) pairs -- `item_views` (visible mask against an
occluder, scene depth and colour, dilation, counts and extents), `item_points` (window pixels, back-projection, centroid, keep rule, the
keyed draw, `pts` / `tem1_pts` and `rgb_choose` / `tem1_choose`, the reference's radius) and `item_crops` (the window crops in the atlas
layout `finish_crops` reads).  Results equal the host function's.  The kernels trust the descriptors they are given: every window is checked
against the canvas and the scratch buffers here, before anything is launched.  Inputs are CUDA tensors; there is no CPU path."""
import functools

import numpy as np
import torch

from .._lib import _D, call, lib, on_device, ptr, stream_ptr
from .prep import _require


@functools.lru_cache(maxsize=None)
def _ints():
    """(table, point descriptor, crop descriptor, pair constants, row record, minimum kept) of the library."""
    return tuple(int(lib().unopose_items_ints(k)) for k in range(6))


def min_kept_points():
    return _ints()[5]


def item_views(obj_depth, obj_rgb, occ_depth, occ_rgb, occ_slot, dilate):
    """obj_depth (V, H, W) float32, obj_rgb (V, H, W, 3) uint8; occ_depth (O, H, W) / occ_rgb (O, H, W, 3) or None; occ_slot: V host integers,
    the occluder canvas of each view or -1; dilate: V host 0 / 1 -> (mask (V, H, W) uint8, scene_depth (V, H, W) float32, scene_rgb
    (V, H, W, 3) uint8, table (V, 8) int32), all on the device.  table: object, visible and final-mask counts, then the final mask's half-open
    extents top, bottom, left, right."""
    _require(obj_depth, "item_views: obj_depth", torch.float32)
    if obj_depth.dim() != 3 or obj_depth.numel() == 0:
        raise RuntimeError(f"item_views: obj_depth {tuple(obj_depth.shape)} is not (V, H, W)")
    V, H, W = (int(v) for v in obj_depth.shape)
    _require(obj_rgb, "item_views: obj_rgb", torch.uint8, (V, H, W, 3))
    occ_slot = np.asarray(occ_slot, dtype=np.int64).reshape(-1)
    dilate = np.asarray(dilate, dtype=np.int64).reshape(-1)
    if len(occ_slot) != V or len(dilate) != V or V > 65535 or H * W >= 2 ** 31:
        raise ValueError(f"item_views: {V} views of {H} x {W}, {len(occ_slot)} occluder slots, {len(dilate)} dilation flags")
    n_occ = 0
    if occ_depth is not None:
        _require(occ_depth, "item_views: occ_depth", torch.float32)
        n_occ = int(occ_depth.shape[0])
        if tuple(occ_depth.shape[1:]) != (H, W):
            raise RuntimeError(f"item_views: occ_depth {tuple(occ_depth.shape)} for {H} x {W} canvases")
        _require(occ_rgb, "item_views: occ_rgb", torch.uint8, (n_occ, H, W, 3))
    if occ_slot.min() < -1 or occ_slot.max() >= n_occ:
        raise ValueError("item_views: occluder slot outside the occluder canvases")
    dev = obj_depth.device
    flags = torch.from_numpy(np.concatenate([occ_slot, dilate != 0]).astype(np.int32)).to(dev)
    mask = torch.empty((V, H, W), dtype=torch.uint8, device=dev)
    scene_depth = torch.empty((V, H, W), dtype=torch.float32, device=dev)
    scene_rgb = torch.empty((V, H, W, 3), dtype=torch.uint8, device=dev)
    rows = torch.empty((V, H, _ints()[4]), dtype=torch.int32, device=dev)
    table = torch.empty((V, _ints()[0]), dtype=torch.int32, device=dev)
    with on_device(dev):
        call("unopose_items_views", ptr(obj_depth), ptr(obj_rgb), ptr(occ_depth) if n_occ else None, ptr(occ_rgb) if n_occ else None,
             ptr(flags[:V]), ptr(flags[V:]), V, H, W, ptr(mask), ptr(scene_depth), ptr(scene_rgb), ptr(rows), ptr(table), stream_ptr(dev))
    return mask, scene_depth, scene_rgb, table


def sense_views(depth, rgb, desc):
    """The scene stage (csrc/scene.hip; `provider_online.sense_views_host` is the specification, equal in every depth bit and colour byte):
    depth (V, H, W) float32 and rgb (V, H, W, 3) uint8 on the device, desc: V host descriptor rows (`provider_online.scene_rows`; range-checked
    here) -> new (depth, rgb): per view the background plane where the canvas is empty, holes and edge drop-outs, axial noise and disparity
    quantisation.  One launch for all views, enqueued on the current stream; nothing comes back to the host."""
    from ..provider_online import SCENE_DESC, check_scene_rows

    _require(depth, "sense_views: depth", torch.float32)
    if depth.dim() != 3 or depth.numel() == 0:
        raise RuntimeError(f"sense_views: depth {tuple(depth.shape)} is not (V, H, W)")
    V, H, W = (int(v) for v in depth.shape)
    _require(rgb, "sense_views: rgb", torch.uint8, (V, H, W, 3))
    desc = check_scene_rows(desc, H, W)
    if len(desc) != V or V > 65535 or H * W >= 2 ** 31 or int(lib().unopose_scene_desc_words()) != SCENE_DESC:
        raise ValueError(f"sense_views: {len(desc)} descriptors of {SCENE_DESC} words for {V} views of {H} x {W}")
    dev = depth.device
    desc_dev = torch.from_numpy(desc.view(np.int64)).to(dev)
    out_depth, out_rgb = torch.empty_like(depth), torch.empty_like(rgb)
    with on_device(dev):
        call("unopose_scene_sense", ptr(depth), ptr(rgb), ptr(desc_dev), V, H, W, ptr(out_depth), ptr(out_rgb), stream_ptr(dev))
    return out_depth, out_rgb


def _windows(windows, H, W, max_side, what):
    """(y0, y1, x0, x1) or None per view -> (n, 5) integers y0, x0, h, w, valid, checked against the canvas and the scratch side."""
    out = np.zeros((len(windows), 5), dtype=np.int64)
    for d, win in enumerate(windows):
        if win is None:
            continue
        y0, y1, x0, x1 = (int(v) for v in (win.as_list() if hasattr(win, "as_list") else win))
        if not (0 <= y0 < y1 <= H and 0 <= x0 < x1 <= W) or y1 - y0 > max_side or x1 - x0 > max_side:
            raise ValueError(f"{what}: window {(y0, y1, x0, x1)} outside the {H} x {W} canvas or above {max_side} pixels a side")
        out[d] = (y0, x0, y1 - y0, x1 - x0, 1)
    return out


def item_points(mask, scene_depth, K, views, windows, pairs, n_pairs, keys, spin, shift, noise, n_want, img_size, is_ref, radius):
    """The points of D views of one kind.  mask / scene_depth: `item_views`' (V, H, W) outputs; K: 3 x 3 intrinsics (host); views: D source view
    numbers; windows: D windows ((y0, y1, x0, x1) or `provider.Window`; None = no item, nothing of the view is read); pairs: D pair numbers
    below n_pairs; keys (n_pairs, 2) uint64, spin (n_pairs, 3, 3) and shift (n_pairs, 3) float64 (host), noise (n_pairs, n_want, 3) float64 on
    the device (queries) or None; radius (n_pairs,) float64 on the device: written by the references, read by the queries (so the references'
    call comes first) -> (pts (D, n_want, 3) float32, choose (D, n_want) int64, counts (D, 2) int32 = set and kept window pixels, win_rows
    (D, max_side) int32 = set pixels per window row).  A view with fewer kept points than the rule asks has undefined pts / choose."""
    _require(mask, "item_points: mask", torch.uint8)
    if mask.dim() != 3:
        raise RuntimeError(f"item_points: mask {tuple(mask.shape)} is not (V, H, W)")
    V, H, W = (int(v) for v in mask.shape)
    _require(scene_depth, "item_points: scene_depth", torch.float32, (V, H, W))
    views, pairs = np.asarray(views, dtype=np.int64).reshape(-1), np.asarray(pairs, dtype=np.int64).reshape(-1)
    D, P, n_want, S = len(views), int(n_pairs), int(n_want), int(img_size)
    max_side = min(H, W)
    if D < 1 or D > 65535 or len(windows) != D or len(pairs) != D or P < 1 or n_want < 1 or not 1 <= S <= 4096:
        raise ValueError(f"item_points: {D} views, {len(windows)} windows, {len(pairs)} pair numbers, {P} pairs, {n_want} points, size {S}")
    if views.min() < 0 or views.max() >= V or pairs.min() < 0 or pairs.max() >= P:
        raise ValueError("item_points: view or pair number out of range")
    win = _windows(windows, H, W, max_side, "item_points")
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    consts = np.concatenate([np.asarray(spin, dtype=np.float64).reshape(-1, 9), np.asarray(shift, dtype=np.float64).reshape(-1, 3)], axis=1)
    if keys.shape != (P, 2) or consts.shape != (P, _ints()[3]):
        raise ValueError(f"item_points: keys {keys.shape}, spin and shift {consts.shape} for {P} pairs")
    dev = mask.device
    _require(radius, "item_points: radius", torch.float64, (P,))
    if not is_ref:
        _require(noise, "item_points: noise", torch.float64, (P, n_want, 3))
    nd = _ints()[1]
    desc = np.zeros((D, nd), dtype=np.int64)
    desc[:, 0], desc[:, 1:5], desc[:, 5], desc[:, 6] = views, win[:, :4], pairs, win[:, 4]
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    words = torch.from_numpy(np.concatenate([np.ascontiguousarray(consts).reshape(-1).view(np.int64), keys.reshape(-1).view(np.int64)])).to(dev)
    consts_dev, keys_dev = words[:consts.size], words[consts.size:]  # 8-byte words: float64 constants, then the uint64 keys
    desc_dev = torch.from_numpy(desc.astype(np.int32)).to(dev)
    ints = torch.empty(D * (2 * max_side + 2 * max_side * max_side), dtype=torch.int32, device=dev)
    win_rows, row_base = ints[:D * max_side].view(D, max_side), ints[D * max_side:2 * D * max_side]
    pix, kept = ints[2 * D * max_side:2 * D * max_side + D * max_side * max_side], ints[2 * D * max_side + D * max_side * max_side:]
    doubles = torch.empty(D * 3 * (max_side + n_want), dtype=torch.float64, device=dev)
    row_sums, drawn = doubles[:D * 3 * max_side], doubles[D * 3 * max_side:]
    counts = torch.empty((D, 2), dtype=torch.int32, device=dev)
    pts = torch.empty((D, n_want, 3), dtype=torch.float32, device=dev)
    choose = torch.empty((D, n_want), dtype=torch.int64, device=dev)
    with on_device(dev):
        call("unopose_items_points", ptr(mask), ptr(scene_depth), H, W, ptr(desc_dev), ptr(consts_dev), ptr(keys_dev), None if is_ref else ptr(noise),
             _D(K[0, 0]), _D(K[1, 1]), _D(K[0, 2]), _D(K[1, 2]), D, int(bool(is_ref)), n_want, S, max_side, ptr(win_rows), ptr(row_base), ptr(pix),
             ptr(kept), ptr(row_sums), ptr(drawn), ptr(radius), ptr(counts), ptr(pts), ptr(choose), stream_ptr(dev))
    return pts, choose, counts, win_rows


def item_crops(mask, scene_rgb, views, windows, atlas, packed, atlas_rows, mask_offsets):
    """The window crops of D views into `atlas` (rows, AW, 3) uint8 and `packed` uint8 (both on the device, written in place): crop d goes to
    atlas rows atlas_rows[d] .. + h - 1, columns 0 .. w - 1, and its h * w mask bytes to packed[mask_offsets[d]:] -- the layout of
    `provider_train.collate_pairs_device`."""
    _require(mask, "item_crops: mask", torch.uint8)
    V, H, W = (int(v) for v in mask.shape)
    _require(scene_rgb, "item_crops: scene_rgb", torch.uint8, (V, H, W, 3))
    _require(atlas, "item_crops: atlas", torch.uint8)
    _require(packed, "item_crops: packed", torch.uint8)
    views = np.asarray(views, dtype=np.int64).reshape(-1)
    D = len(views)
    atlas_rows, mask_offsets = np.asarray(atlas_rows, dtype=np.int64).reshape(-1), np.asarray(mask_offsets, dtype=np.int64).reshape(-1)
    if D < 1 or D > 65535 or len(windows) != D or len(atlas_rows) != D or len(mask_offsets) != D or atlas.dim() != 3 or atlas.shape[2] != 3 or packed.dim() != 1:
        raise ValueError(f"item_crops: {D} views, {len(windows)} windows, atlas {tuple(atlas.shape)}")
    if any(w is None for w in windows) or views.min() < 0 or views.max() >= V:
        raise ValueError("item_crops: a crop without a window or a view out of range")
    win = _windows(windows, H, W, min(H, W), "item_crops")
    h, w = win[:, 2], win[:, 3]
    AH, AW = int(atlas.shape[0]), int(atlas.shape[1])
    if (atlas_rows < 0).any() or (atlas_rows + h > AH).any() or (w > AW).any() or (mask_offsets < 0).any() or (mask_offsets + h * w > packed.numel()).any():
        raise ValueError("item_crops: a crop outside the atlas or the packed masks")
    desc = np.zeros((D, _ints()[2]), dtype=np.int64)
    desc[:, 0], desc[:, 1:5], desc[:, 5], desc[:, 6] = views, win[:, :4], atlas_rows, mask_offsets
    if desc.max() >= 2 ** 31:
        raise ValueError("item_crops: too many pixels for 32-bit offsets")
    dev = mask.device
    desc_dev = torch.from_numpy(desc.astype(np.int32)).to(dev)
    with on_device(dev):
        call("unopose_items_crops", ptr(mask), ptr(scene_rgb), H, W, ptr(desc_dev), D, int(h.max()), AW, ptr(atlas), ptr(packed), stream_ptr(dev))
