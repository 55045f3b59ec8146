"""The training provider's colour augmentation on the device (csrc/coloraug.hip) and the finishing of a batch's crops behind it.
`provider_train.ColorAugmentor.apply` is the specification: `color_augment` equals it byte for byte.  The loader draws (`ColorAugmentor.plan`)
and packs (`provider_train.pack_plans`, `collate_pairs_device`); here the tables are range-checked against the atlas BEFORE anything is
launched -- the kernels trust them -- and the launches are enqueued: one per chain position over all crops, alternating two atlases, plus
a luma reduction in front of a position that holds a contrast and two line launches behind one that holds a blur.  Inputs are CUDA tensors;
there is no CPU path."""
import functools

import numpy as np
import torch

from .._lib import call, lib, on_device, ptr, stream_ptr
from .prep import PrepPlan, _require, _result, prep_crop_resize

MAX_BLUR_RADIUS = 255


@functools.lru_cache(maxsize=None)
def _ints():
    from ..provider_train import AUG_DESC_INTS, AUG_ENTRY_INTS

    nd, ne, max_line, n_ops = (int(lib().unopose_coloraug_ints(k)) for k in range(4))
    if (nd, ne) != (AUG_DESC_INTS, AUG_ENTRY_INTS):
        raise RuntimeError(f"color_augment: the library's tables are {nd} / {ne} ints wide, provider_train packs {AUG_DESC_INTS} / {AUG_ENTRY_INTS}")
    return nd, ne, max_line, n_ops


def _host(x, dtype):
    return np.ascontiguousarray(x.numpy() if torch.is_tensor(x) else x, dtype=dtype)


class AugTables:
    """Packed plan tables (`provider_train.pack_plans`' four arrays, numpy or CPU tensors), checked against an H x W atlas: every crop
    inside it and on rows of its own, every entry's opcode, grid, noise field, blur radius and sum slot in range.  Holds what the launches
    need: per chain position, whether a contrast is there and the extents of the crops that blur."""

    def __init__(self, desc, ops, grids, noise, atlas_hw):
        from ..provider_train import OP_COARSE_DROPOUT, OP_CONTRAST, OP_GAUSSIAN_BLUR, OP_GAUSSIAN_NOISE

        nd, ne, max_line, n_ops = _ints()
        H, W = (int(v) for v in atlas_hw)
        self.src = (desc, ops, grids, noise)
        desc, ops = _host(desc, np.int32).astype(np.int64), _host(ops, np.int32)
        n_grid, n_noise = int(np.prod(grids.shape)), int(np.prod(noise.shape))
        if desc.ndim != 2 or desc.shape[1] != nd or not 1 <= desc.shape[0] <= 65535 or ops.ndim != 2 or ops.shape[1] != ne or len(ops) < 1:
            raise ValueError(f"color_augment: descriptors {desc.shape}, entries {ops.shape}")
        if n_grid < 1 or n_noise < 1 or grids.dtype not in (np.uint8, torch.uint8) or noise.dtype not in (np.float32, torch.float32):
            raise ValueError("color_augment: grids must be a non-empty uint8 table, noise a non-empty float32 one")
        y0, h, w, length, first, g0, z0 = (desc[:, c] for c in range(7))
        if (y0 < 0).any() or (h < 1).any() or (w < 1).any() or (y0 + h > H).any() or (w > W).any():
            raise ValueError(f"color_augment: a crop outside the {H} x {W} atlas")
        order = np.argsort(y0, kind="stable")
        if (y0[order][1:] < (y0 + h)[order][:-1]).any():
            raise ValueError("color_augment: crops share atlas rows")
        if (length < 0).any() or (first < 0).any() or (first + length > len(ops)).any() or (g0 < 0).any() or (z0 < 0).any():
            raise ValueError("color_augment: a chain outside the entry table")
        if int((h * w).max()) >= 2 ** 31 // 3:
            raise ValueError("color_augment: crop too large")
        self.n, self.steps, self.max_pixels = len(desc), int(length.max()), int((h * w).max())
        self.contrast = [False] * self.steps
        self.blur = [None] * self.steps  # (max h, max w) of the crops that blur at this position
        slots = []
        for c in range(self.n):
            for pos in range(int(length[c])):
                e = ops[first[c] + pos]
                op = int(e[0])
                if not 0 <= op < n_ops:
                    raise ValueError(f"color_augment: opcode {op}")
                if op == OP_COARSE_DROPOUT:
                    if e[1] < 1 or e[2] < 1 or e[3] < 0 or g0[c] + e[3] + int(e[1]) * int(e[2]) > n_grid:
                        raise ValueError("color_augment: drop grid outside its table")
                elif op == OP_GAUSSIAN_NOISE:
                    if e[1] < 0 or z0[c] + e[1] + 3 * h[c] * w[c] > n_noise:
                        raise ValueError("color_augment: noise field outside its table")
                elif op == OP_GAUSSIAN_BLUR:
                    if not 0 <= e[1] <= MAX_BLUR_RADIUS or max(h[c], w[c]) > max_line:
                        raise ValueError(f"color_augment: blur radius {e[1]} on a {h[c]} x {w[c]} crop (sides up to {max_line})")
                    mh, mw = self.blur[pos] or (0, 0)
                    self.blur[pos] = (max(mh, int(h[c])), max(mw, int(w[c])))
                elif op == OP_CONTRAST:
                    slots.append(int(e[2]))
                    self.contrast[pos] = True
        if sorted(slots) != list(range(len(slots))):
            raise ValueError("color_augment: contrast entries must own the sum slots 0 .. n - 1, one each")
        self.n_sums, self.boxes = len(slots), np.stack([y0, h, w], axis=1)

    def upload(self, device):
        desc, ops, grids, noise = self.src
        nd, ne = _ints()[:2]
        ints = torch.cat([torch.as_tensor(_host(desc, np.int32)).reshape(-1), torch.as_tensor(_host(ops, np.int32)).reshape(-1)])
        ints = ints.to(device, non_blocking=True)
        return (ints[:self.n * nd], ints[self.n * nd:], torch.as_tensor(grids).reshape(-1).to(device, non_blocking=True),
                torch.as_tensor(noise).reshape(-1).to(device, non_blocking=True))


def color_augment(atlas, desc, plans, out=None):
    """`ColorAugmentor.apply(crop, plan)` for every crop of a batch.  atlas: (H, W, 3) uint8 on the device, the crops one under the other
    (crop c on rows y0 .. y0 + h - 1, columns 0 .. w - 1; `provider_train.build_atlas`).  desc: one (y0, h, w) per crop, host integers.
    plans: one `AugPlan` (or None) per crop, or the four packed tables of `provider_train.pack_plans` (then `desc` may be None: the
    tables hold the boxes).  -> the augmented atlas (`out`, or a new one whose padding is zero); `atlas` is only read."""
    from ..provider_train import pack_plans

    _require(atlas, "color_augment: atlas", torch.uint8)
    if atlas.dim() != 3 or atlas.shape[2] != 3 or atlas.numel() == 0:
        raise RuntimeError(f"color_augment: atlas {tuple(atlas.shape)} is not (H, W, 3)")
    H, W = int(atlas.shape[0]), int(atlas.shape[1])
    if isinstance(plans, tuple) and len(plans) == 4 and not hasattr(plans[0], "ops"):
        tables = AugTables(*plans, (H, W))
        if desc is not None and not np.array_equal(np.asarray(desc, dtype=np.int64).reshape(-1, 3), tables.boxes):
            raise ValueError("color_augment: desc differs from the boxes of the packed tables")
    else:
        boxes = np.asarray(desc, dtype=np.int64).reshape(-1, 3)
        if len(boxes) != len(plans):
            raise ValueError(f"color_augment: {len(boxes)} crops, {len(plans)} plans")
        tables = AugTables(*pack_plans([tuple(int(v) for v in b) for b in boxes], plans), (H, W))
    dev = atlas.device
    if out is None:
        out = torch.zeros_like(atlas)
    else:
        out = _result(out, "color_augment: out", torch.uint8, tuple(atlas.shape), dev)
        if out.data_ptr() == atlas.data_ptr():
            raise RuntimeError("color_augment: out must not be the atlas")
    d_desc, d_ops, d_grids, d_noise = tables.upload(dev)
    sums = torch.zeros(max(tables.n_sums, 1), dtype=torch.int64, device=dev)
    steps = max(tables.steps, 1)  # an all-empty batch still takes one launch: every crop is copied through
    tmp = torch.empty_like(atlas) if steps > 1 else None
    src = atlas
    with on_device(dev):
        s = stream_ptr(dev)
        for pos in range(steps):
            dst = out if (steps - 1 - pos) % 2 == 0 else tmp
            if pos < tables.steps and tables.contrast[pos]:
                call("unopose_coloraug_luma_sum", ptr(src), H, W, ptr(d_desc), ptr(d_ops), tables.n, tables.max_pixels, pos, ptr(sums), s)
            call("unopose_coloraug_step", ptr(src), ptr(dst), H, W, ptr(d_desc), ptr(d_ops), ptr(d_grids), ptr(d_noise), ptr(sums), tables.n,
                 tables.max_pixels, pos, s)
            if pos < tables.steps and tables.blur[pos] is not None:
                mh, mw = tables.blur[pos]
                call("unopose_coloraug_blur_lines", ptr(src), ptr(dst), H, W, ptr(d_desc), ptr(d_ops), tables.n, mh, mw, pos, 0, s)
                call("unopose_coloraug_blur_lines", ptr(dst), ptr(dst), H, W, ptr(d_desc), ptr(d_ops), tables.n, mw, mh, pos, 1, s)
            src = dst
    return out


def finish_crops(batch, device):
    """A `provider_train.collate_pairs_device` batch -> the batch the training step takes, on `device`: the crop atlas is uploaded,
    augmented (`color_augment`), then masked, resized and normalised (`PrepPlan` + `prep_crop_resize`; windows = the crops' atlas rows)
    into `rgb` and `tem1_rgb` (B, 3, S, S) float32.  Every other key is moved to the device; the `crop_*` helper keys are dropped."""
    from ..provider_train import CROP_KEYS

    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("finish_crops: CPU not supported")
    missing = [k for k in CROP_KEYS if k not in batch]
    if missing:
        raise KeyError(f"finish_crops: the batch lacks {missing} (collate with provider_train.collate_pairs_device)")
    with torch.cuda.device(device):
        atlas = batch["crop_atlas"].to(device, non_blocking=True)
        masks = batch["crop_masks"].to(device, non_blocking=True)
        done = color_augment(atlas, None, tuple(batch[k] for k in ("crop_desc", "crop_ops", "crop_grids", "crop_noise")))
        size, use_mask = (int(v) for v in batch["crop_cfg"].tolist())
        boxes = batch["crop_desc"].numpy()[:, :3].astype(np.int64)
        windows = [(int(y0), int(y0 + h), 0, int(w)) for y0, h, w in boxes]
        plan = PrepPlan.from_device(tuple(atlas.shape[:2]), windows, masks, batch["crop_rows"].numpy(), size, device)
        crops = prep_crop_resize(done, plan, use_mask=bool(use_mask))
    if len(windows) % 2:
        raise ValueError(f"finish_crops: {len(windows)} crops are not pairs")
    out = {k: v.to(device, non_blocking=True) for k, v in batch.items() if k not in CROP_KEYS}
    out["rgb"], out["tem1_rgb"] = crops[:len(windows) // 2], crops[len(windows) // 2:]
    return out
