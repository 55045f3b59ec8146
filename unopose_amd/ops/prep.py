"""Query-side instance preparation of the BOP test provider on the device (csrc/prep.hip): the per-pixel work of
`provider.BOPTestsetOneRef.get_instance` for all detections of an image -- crop -> mask -> resize -> normalise
(`provider._normalised_crop`), `np.flatnonzero` + `provider.lift_depth` + distance to the centroid, and the gather of the drawn
samples with `provider.Window.to_resized`.  Results equal the host provider's; the provider's own functions fill the tables the
kernels read (resize taps, normalisation values), so there is one definition of that arithmetic.

The kernels trust the descriptors they are given: `PrepPlan` builds them on the host from the windows and masks and checks every
range against the image and the buffers BEFORE anything is uploaded.  Inputs are CUDA tensors; there is no CPU path."""
import functools

import numpy as np
import torch

from .._lib import _D, call, lib, on_device, ptr, stream_ptr
from .common import note_mutation


@functools.lru_cache(maxsize=None)
def _desc_ints():
    return int(lib().unopose_prep_desc_ints())


@functools.lru_cache(maxsize=512)
def _tap_table(dst, src, axis):
    """`provider.resize_bilinear_u8`'s taps of one axis as 4*dst int32 [index 0 | index 1 | weight 0 | weight 1] (weights x 2048).
    axis 0 = columns: an index left of 0 or at / after the last column collapses to that one pixel; axis 1 = rows: clamped."""
    from ..provider import _linear_taps

    s, f = _linear_taps(dst, src)
    if axis == 0:
        lo, hi = s < 0, s >= src - 1
        f = np.where(lo | hi, np.float32(0), f)
        s = np.where(lo, 0, np.where(hi, src - 1, s))
        i0, i1 = s, np.minimum(s + 1, src - 1)
    else:
        i0, i1 = np.clip(s, 0, src - 1), np.clip(s + 1, 0, src - 1)
    w0 = np.rint((np.float32(1) - f) * np.float32(2048))
    w1 = np.rint(f * np.float32(2048))
    return np.concatenate([i0, i1, w0, w1]).astype(np.int32)


_NORM_TABLES = {}


def prep_norm_table(device, mean=None, std=None):
    """(3 * 256) float32 on `device`: value v of channel k after ToTensor + Normalize, computed by `provider.to_tensor_normalize`
    itself (x * (1 / 255) would differ in the last bit from its x / 255).  Built once per device and statistics."""
    from ..provider import IMAGENET_MEAN, IMAGENET_STD, to_tensor_normalize

    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("prep_norm_table: CPU not supported")
    mean, std = tuple(mean or IMAGENET_MEAN), tuple(std or IMAGENET_STD)
    key = (device, mean, std)
    if key not in _NORM_TABLES:
        values = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, axis=2)  # (256, 1, 3): an image with one column
        _NORM_TABLES[key] = to_tensor_normalize(values, mean, std).reshape(3 * 256).contiguous().to(device)
    return _NORM_TABLES[key]


class PrepPlan:
    """The detections of one image as the kernels read them: one descriptor per detection, the window masks back to back, per-row
    prefix counts of the masks and the resize taps of every distinct window side -- built and range-checked on the host, uploaded
    in two copies.  `windows`: (y0, y1, x0, x1) tuples or `provider.Window`s; `masks`: the (h, w) window masks (non-zero = set)."""

    def __init__(self, image_hw, windows, masks, img_size, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("PrepPlan: CPU not supported")
        if len(windows) != len(masks):
            raise ValueError(f"PrepPlan: {len(windows)} windows, {len(masks)} masks")
        boxes = self._boxes(image_hw, windows, img_size)
        flat, rows = [], []
        for (y0, y1, x0, x1), mask in zip(boxes, masks):
            h, w = y1 - y0, x1 - x0
            m = np.ascontiguousarray(np.asarray(mask) != 0)
            if m.shape != (h, w):
                raise ValueError(f"PrepPlan: mask {m.shape} for a {h} x {w} window")
            flat.append(m.reshape(-1))
            rows.append(m.sum(axis=1, dtype=np.int64))
        self._assemble(image_hw, boxes, rows, img_size, device)
        self.masks = torch.from_numpy(np.concatenate(flat).view(np.uint8)).to(device)

    @classmethod
    def from_device(cls, image_hw, windows, packed_masks, row_counts, img_size, device):
        """The same plan from window masks that are already on the device (`ops.window_masks`): `packed_masks` = the windows' 0 / 1
        bytes back to back in window order (kept, not copied), `row_counts` = their set pixels per row in the same order, int32 on the
        device (read back here in one pinned copy) or already on the host."""
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("PrepPlan: CPU not supported")
        boxes = cls._boxes(image_hw, windows, img_size)
        heights = [y1 - y0 for y0, y1, _, _ in boxes]
        _require(packed_masks, "PrepPlan: packed_masks", torch.uint8, (sum((y1 - y0) * (x1 - x0) for y0, y1, x0, x1 in boxes),))
        if torch.is_tensor(row_counts):
            _require(row_counts, "PrepPlan: row_counts", torch.int32, (sum(heights),))
            from .rle import _to_host

            with torch.cuda.device(device):
                row_counts = _to_host(row_counts)
        row_counts = np.asarray(row_counts).reshape(-1).astype(np.int64)
        if len(row_counts) != sum(heights):
            raise ValueError(f"PrepPlan: {len(row_counts)} row counts for {sum(heights)} window rows")
        widths = np.repeat([x1 - x0 for _, _, x0, x1 in boxes], heights)
        if (row_counts < 0).any() or (row_counts > widths).any():
            raise ValueError("PrepPlan: row count outside its window row")
        plan = cls.__new__(cls)
        plan._assemble(image_hw, boxes, np.split(row_counts, np.cumsum(heights)[:-1]), img_size, device)
        plan.masks = packed_masks
        return plan

    @staticmethod
    def _boxes(image_hw, windows, img_size):
        """The windows as (y0, y1, x0, x1) integers, checked against the image."""
        H, W = (int(v) for v in image_hw)
        S, D = int(img_size), len(windows)
        if D < 1 or D > 65535:
            raise ValueError(f"PrepPlan: {D} windows")
        if not 1 <= S <= 4096:
            raise ValueError(f"PrepPlan: img_size {S}")
        boxes = []
        for win in windows:
            y0, y1, x0, x1 = (int(v) for v in (win.as_list() if hasattr(win, "as_list") else win))
            if not (0 <= y0 < y1 <= H and 0 <= x0 < x1 <= W):
                raise ValueError(f"PrepPlan: window {(y0, y1, x0, x1)} outside the {H} x {W} image")
            boxes.append((y0, y1, x0, x1))
        return boxes

    def _assemble(self, image_hw, boxes, rows, img_size, device):
        """Descriptors, row prefixes and tap tables from the checked windows and their per-row set counts; one upload."""
        H, W = (int(v) for v in image_hw)
        S, D = int(img_size), len(boxes)
        nd = _desc_ints()
        desc = np.zeros((D, nd), dtype=np.int64)
        bases, taps, tap_at = [], [], {}
        mask_off = pt_off = row_off = tap_off = 0
        for d, ((y0, y1, x0, x1), row) in enumerate(zip(boxes, rows)):
            h, w = y1 - y0, x1 - x0
            n = int(row.sum())
            if n < 1:
                raise ValueError("PrepPlan: empty mask")
            mode = 0 if (h, w) == (S, S) else 1 if (h, w) == (2 * S, 2 * S) else 2
            at = [0, 0]
            if mode == 2:
                for axis, src in ((0, w), (1, h)):
                    if (src, axis) not in tap_at:
                        tap_at[(src, axis)] = tap_off
                        taps.append(_tap_table(S, src, axis))
                        tap_off += 4 * S
                    at[axis] = tap_at[(src, axis)]
            desc[d, :11] = (y0, x0, h, w, mask_off, pt_off, n, row_off, mode, at[0], at[1])
            bases.append(np.cumsum(row) - row)
            mask_off, pt_off, row_off = mask_off + h * w, pt_off + n, row_off + h
        if max(mask_off, 3 * pt_off, tap_off) >= 2 ** 31:
            raise ValueError("PrepPlan: too many pixels for 32-bit offsets")
        ints = np.concatenate([desc.reshape(-1), *bases, *taps]).astype(np.int32)
        ints_dev = torch.from_numpy(ints).to(device)
        self.desc, self.row_base = ints_dev[:D * nd], ints_dev[D * nd:D * nd + row_off]
        self.taps = ints_dev[D * nd + row_off:] if taps else ints_dev[:1]  # never read without bilinear windows
        self.device, self.H, self.W, self.S, self.D = device, H, W, S, D
        self.h, self.w, self.n, self.pt_off = (desc[:, c].copy() for c in (2, 3, 6, 5))
        self.n_points, self.n_rows = pt_off, row_off


def _require(x, name, dtype, shape=None):
    if not torch.is_tensor(x) or not x.is_cuda:
        raise RuntimeError(f"{name}: CPU not supported")
    if x.dtype != dtype or not x.is_contiguous():
        raise RuntimeError(f"{name} must be a contiguous {dtype} tensor")
    if shape is not None and tuple(x.shape) != tuple(shape):
        raise RuntimeError(f"{name} must have shape {tuple(shape)}, not {tuple(x.shape)}")


def _result(out, name, dtype, shape, device):
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    _require(out, name, dtype, shape)
    note_mutation()
    return out


def prep_crop_resize(img, plan, lut=None, bgr=False, use_mask=True, out=None):
    """`provider._normalised_crop` of every window of `plan`: img (H, W) or (H, W, C) uint8 -> (D, 3, S, S) float32."""
    _require(img, "prep_crop_resize: img", torch.uint8)
    if img.dim() not in (2, 3) or tuple(img.shape[:2]) != (plan.H, plan.W) or (img.dim() == 3 and img.shape[2] not in (1, 3, 4)):
        raise RuntimeError(f"prep_crop_resize: img {tuple(img.shape)} for a plan over {plan.H} x {plan.W}")
    lut = prep_norm_table(img.device) if lut is None else lut
    _require(lut, "prep_crop_resize: lut", torch.float32, (3 * 256,))
    out = _result(out, "prep_crop_resize: out", torch.float32, (plan.D, 3, plan.S, plan.S), img.device)
    with on_device(img.device):
        call("unopose_prep_crop_resize", ptr(img), plan.H, plan.W, 1 if img.dim() == 2 else int(img.shape[2]), ptr(plan.desc), ptr(plan.taps),
             ptr(plan.masks), ptr(lut), plan.D, plan.S, int(bool(bgr)), int(bool(use_mask)), ptr(out), stream_ptr(img.device))
    return out


def prep_lift(depth, K, plan, out=None):
    """depth (H, W) float64 (metres), K the 3 x 3 intrinsics (host) -> (pix int32, cloud float64 (n_points, 3), dist float64): per detection,
    back to back in `plan.pt_off` order, the set window pixels in row-major order, their back-projection and distance to the centroid."""
    _require(depth, "prep_lift: depth", torch.float64, (plan.H, plan.W))
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    dev, N = depth.device, plan.n_points
    o = out if out is not None else (None, None, None)
    pix = _result(o[0], "prep_lift: pix", torch.int32, (N,), dev)
    cloud = _result(o[1], "prep_lift: cloud", torch.float64, (N, 3), dev)
    dist = _result(o[2], "prep_lift: dist", torch.float64, (N,), dev)
    row_sums = torch.empty(plan.n_rows * 3, dtype=torch.float64, device=dev)
    with on_device(dev):
        call("unopose_prep_compact_lift", ptr(depth), plan.H, plan.W, ptr(plan.desc), ptr(plan.masks), ptr(plan.row_base), _D(K[0, 0]), _D(K[1, 1]),
             _D(K[0, 2]), _D(K[1, 2]), plan.D, int(plan.h.max()), ptr(pix), ptr(cloud), ptr(row_sums), stream_ptr(dev))
        call("unopose_prep_distances", ptr(plan.desc), ptr(cloud), ptr(row_sums), plan.D, int(plan.n.max()), ptr(dist), stream_ptr(dev))
    return pix, cloud, dist


def prep_gather(plan, picked, index, pix, cloud, out=None):
    """The drawn samples: `picked` = detection numbers of `plan` (host), `index` (P, n) host integers = positions in the compacted
    arrays (each row inside its detection's range) -> pts (P, n, 3) float32 = cloud rows rounded once, choose (P, n) int64 =
    `Window.to_resized` of the drawn pixels."""
    _require(pix, "prep_gather: pix", torch.int32, (plan.n_points,))
    _require(cloud, "prep_gather: cloud", torch.float64, (plan.n_points, 3))
    picked = np.asarray(picked, dtype=np.int64).reshape(-1)
    index = np.asarray(index)
    P = len(picked)
    if P < 1 or P > 65535 or index.ndim != 2 or index.shape[0] != P or index.shape[1] < 1 or index.dtype.kind not in "iu":
        raise ValueError(f"prep_gather: {P} picked detections, index {index.shape} {index.dtype}")
    if picked.min() < 0 or picked.max() >= plan.D:
        raise ValueError("prep_gather: picked detection outside the plan")
    first = plan.pt_off[picked][:, None]
    if (index < first).any() or (index >= first + plan.n[picked][:, None]).any():
        raise ValueError("prep_gather: index outside its detection's points")
    n, dev = int(index.shape[1]), pix.device
    o = out if out is not None else (None, None)
    pts = _result(o[0], "prep_gather: pts", torch.float32, (P, n, 3), dev)
    choose = _result(o[1], "prep_gather: choose", torch.int64, (P, n), dev)
    hw = np.stack([plan.h[picked], plan.w[picked]], axis=1).reshape(-1)
    ints = torch.from_numpy(np.concatenate([hw, index.reshape(-1)]).astype(np.int32)).to(dev)
    with on_device(dev):
        call("unopose_prep_gather", ptr(ints[:2 * P]), ptr(ints[2 * P:]), ptr(pix), ptr(cloud), P, n, plan.S, ptr(pts), ptr(choose), stream_ptr(dev))
    return pts, choose
