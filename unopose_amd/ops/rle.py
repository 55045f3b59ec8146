"""COCO run-length masks on the device (csrc/rle.hip), both directions, for all masks of a call at once.

`rle_decode` is `provider.rle_decode` (pycocotools' `frPyObjects` + `decode`) for the detections of an image, with the `depth > 0`
restriction, the pixel count and the bounding extents `provider.BOPTestsetOneRef.get_instance` derives from the mask; `window_masks`
crops the decoded masks to their windows in the layout `PrepPlan` keeps; `rle_encode` is the BOP toolkit's
`pycoco_utils.binary_mask_to_rle` with the area and `bbox_from_binary_mask` (`scene_gt_coco.json`).  Results equal the host
functions'.  The host only packs: strings into one byte buffer, lists into one int32 buffer, sizes of every buffer known before the
launch (`pack_segs`, numpy, no loop over characters).  Inputs are CUDA tensors; there is no CPU path."""
import functools

import numpy as np
import torch

from .._lib import call, lib, on_device, ptr, stream_ptr
from .prep import _result

FLAG_NEGATIVE, FLAG_OVERLONG, FLAG_MALFORMED = 1, 2, 4


@functools.lru_cache(maxsize=None)
def _desc_ints():
    return int(lib().unopose_rle_desc_ints())


@functools.lru_cache(maxsize=None)
def _stats_ints():
    return int(lib().unopose_rle_stats_ints())


def pack_segs(segs, desc_ints=8):
    """[{"size": [H, W], "counts": list | str | bytes}] -> (H, W, desc (D, desc_ints) int32, bytes uint8, lists int32, n_starts): the
    decode kernels' input.  Raises ValueError for sizes that differ, bytes outside 48..111, a string that ends inside a number, and
    more than 2^31 - 1 pixels or buffer entries.  Host only (numpy)."""
    D = len(segs)
    if D < 1 or D > 65535:
        raise ValueError(f"rle: {D} masks")
    sizes = {(int(s["size"][0]), int(s["size"][1])) for s in segs}
    if len(sizes) != 1:
        raise ValueError(f"rle: masks of different sizes in one call: {sorted(sizes)}")
    (H, W), = sizes
    if H < 1 or W < 1 or H * W >= 2 ** 31:
        raise ValueError(f"rle: mask size {H} x {W}")
    desc = np.zeros((D, desc_ints), dtype=np.int64)
    strings, lists = [], []
    for d, seg in enumerate(segs):
        counts = seg["counts"]
        if isinstance(counts, str):
            try:
                counts = counts.encode("ascii")
            except UnicodeEncodeError:
                raise ValueError(f"rle: mask {d}: character outside 48..111 in the count string") from None
        if isinstance(counts, (bytes, bytearray)):
            desc[d, 0], desc[d, 2] = 1, len(counts)
            strings.append((d, bytes(counts)))
        else:
            arr = np.asarray(counts if len(counts) else [], dtype=np.int64).reshape(-1)
            # the kernel flags a negative count and a total above H * W: values beyond either are clipped to the nearest flagged one
            lists.append((d, np.clip(arr, -1, min(H * W + 1, 2 ** 31 - 1))))
            desc[d, 2] = desc[d, 3] = len(arr)
    if strings:
        which = np.array([d for d, _ in strings])
        desc[which, 1] = np.cumsum(desc[which, 2]) - desc[which, 2]
        buf = np.frombuffer(b"".join(s for _, s in strings), dtype=np.uint8)
        bad = np.flatnonzero((buf < 48) | (buf > 111))
        if len(bad):
            d = which[np.searchsorted(desc[which, 1], bad[0], side="right") - 1]
            raise ValueError(f"rle: mask {d}: byte {int(buf[bad[0]])} outside 48..111 in the count string")
        ends = ((buf.astype(np.int64) - 48) & 0x20) == 0  # the last byte of every number
        before = np.concatenate([[0], np.cumsum(ends)])
        first, last = desc[which, 1], desc[which, 1] + desc[which, 2]
        desc[which, 3] = before[last] - before[first]
        open_end = np.flatnonzero((desc[which, 2] > 0) & ~ends[np.maximum(last - 1, 0)]) if len(buf) else []
        if len(open_end):
            raise ValueError(f"rle: mask {which[open_end[0]]}: the count string ends inside a number")
    else:
        buf = np.zeros(0, dtype=np.uint8)
    if lists:
        which = np.array([d for d, _ in lists])
        desc[which, 1] = np.cumsum(desc[which, 2]) - desc[which, 2]
        ints = np.concatenate([a for _, a in lists]).astype(np.int32)
    else:
        ints = np.zeros(0, dtype=np.int32)
    desc[:, 4] = np.cumsum(desc[:, 3] + 1) - (desc[:, 3] + 1)
    n_starts = int(desc[-1, 4] + desc[-1, 3] + 1)
    if max(n_starts, len(buf), len(ints)) >= 2 ** 31:
        raise ValueError("rle: too many counts for 32-bit offsets")
    return H, W, desc.astype(np.int32), buf, ints, n_starts


_PINNED = {}


def _to_host(t):
    """Device tensor -> numpy through a pinned buffer kept per dtype; waits for this copy alone (one event)."""
    n = t.numel()
    buf = _PINNED.get(t.dtype)
    if buf is None or buf.numel() < n:
        buf = _PINNED[t.dtype] = torch.empty(max(n, 1 << 12), dtype=t.dtype).pin_memory()
    view = buf[:n]
    view.copy_(t.reshape(-1), non_blocking=True)
    event = torch.cuda.Event()
    event.record()
    event.synchronize()
    return view.numpy().reshape(tuple(t.shape)).copy()


def rle_decode(segs, device, depth=None, with_host_stats=False, out=None):
    """`provider.rle_decode` of every entry of `segs` (lists and compressed strings may be mixed; one size) -> masks (D, H, W) uint8 in
    {0, 1} and stats (D, 6) int32 [n_set, y_first, y_last + 1, x_first, x_last + 1, flags] on `device`; an empty mask has extents
    [H, 0, W, 0].  depth: the image's (H, W) float64 map on the device: masks and stats are then those of `mask AND depth > 0`
    (`valid` of `get_instance`).  Counts that sum short of H * W leave the rest 0.  A negative count or counts summing above H * W
    raise ValueError naming the mask (nothing is written outside `masks` before that).  The stats come back to the host once for
    that check; `with_host_stats` returns that copy as a third value.  out: (masks, stats) to write into."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("rle_decode: CPU not supported")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    H, W, desc, buf, ints, n_starts = pack_segs(segs, _desc_ints())
    if depth is not None:
        if not torch.is_tensor(depth) or not depth.is_cuda:
            raise RuntimeError("rle_decode: depth: CPU not supported")
        if depth.dtype != torch.float64 or not depth.is_contiguous() or tuple(depth.shape) != (H, W) or depth.device != device:
            raise RuntimeError(f"rle_decode: depth must be a contiguous float64 ({H}, {W}) tensor on {device}")
    D = len(desc)
    n_bytes = len(buf)
    host = np.concatenate([desc.reshape(-1), ints, np.zeros(1, np.int32)]).view(np.uint8)  # one upload: int32 part first (aligned)
    up = torch.from_numpy(np.concatenate([host, buf, np.zeros(1, np.uint8)])).to(device)
    n_desc, n_ints = desc.size * 4, (len(ints) + 1) * 4
    desc_dev, ints_dev, bytes_dev = up[:n_desc], up[n_desc:n_desc + n_ints], up[n_desc + n_ints:n_desc + n_ints + n_bytes + 1]
    starts = torch.empty(n_starts, dtype=torch.int32, device=device)
    o = out if out is not None else (None, None)
    masks = _result(o[0], "rle_decode: masks", torch.uint8, (D, H, W), device)
    stats = _result(o[1], "rle_decode: stats", torch.int32, (D, _stats_ints()), device)
    with torch.cuda.device(device):
        call("unopose_rle_parse", ptr(bytes_dev), ptr(ints_dev), ptr(desc_dev), D, H, W, ptr(starts), ptr(stats), stream_ptr(device))
        call("unopose_rle_fill", ptr(desc_dev), ptr(starts), ptr(depth) if depth is not None else None, D, H, W, ptr(masks), ptr(stats),
             stream_ptr(device))
        stats_host = _to_host(stats)
    bad = np.flatnonzero(stats_host[:, 5])
    if len(bad):
        d, f = int(bad[0]), int(stats_host[bad[0], 5])
        what = [w for bit, w in ((FLAG_NEGATIVE, "a negative count"), (FLAG_OVERLONG, f"counts summing above {H} x {W}"),
                                 (FLAG_MALFORMED, "a number without end or outside 32 bits")) if f & bit]
        raise ValueError(f"rle_decode: mask {d}: " + ", ".join(what))
    return (masks, stats, stats_host) if with_host_stats else (masks, stats)


def _require_masks(masks, name):
    if not torch.is_tensor(masks) or not masks.is_cuda:
        raise RuntimeError(f"{name}: CPU not supported")
    if masks.dtype not in (torch.uint8, torch.bool) or masks.dim() != 3 or not masks.is_contiguous():
        raise RuntimeError(f"{name}: masks must be a contiguous (D, H, W) uint8 or bool tensor")
    D, H, W = (int(v) for v in masks.shape)
    if D < 1 or D > 65535 or H < 1 or W < 1 or H * W >= 2 ** 31:
        raise ValueError(f"{name}: masks {tuple(masks.shape)}")
    return D, H, W


def rle_encode(masks, out=None):
    """masks (D, H, W) uint8 or bool on the device, non-zero = set -> (counts, area, bbox): per mask the uncompressed count list of
    `pycoco_utils.binary_mask_to_rle` (int32 array; leading 0 when the first column-major pixel is set), the number of set pixels
    (int64 array) and `bbox_from_binary_mask`'s [x, y, w, h] (None for an empty mask).  Two passes: the totals come back once, then
    the boundaries are compacted into a buffer of exactly the summed length.  out: an int32 device tensor of exactly that length for the
    counts of all masks back to back."""
    D, H, W = _require_masks(masks, "rle_encode")
    device = masks.device
    col_count = torch.empty((D, W), dtype=torch.int32, device=device)
    totals = torch.zeros((D, _stats_ints()), dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        call("unopose_rle_column_scan", ptr(masks), D, H, W, ptr(col_count), ptr(totals), stream_ptr(device))
        tot = _to_host(totals).astype(np.int64)
        n = tot[:, 0] + 1
        off = np.concatenate([[0], np.cumsum(n)])
        if off[-1] >= 2 ** 31:
            raise ValueError("rle_encode: too many runs for 32-bit offsets")
        off_dev = torch.from_numpy(off).to(device)
        pos = torch.empty(int(off[-1]), dtype=torch.int32, device=device)
        counts = _result(out, "rle_encode: out", torch.int32, (int(off[-1]),), device)
        call("unopose_rle_compact", ptr(masks), ptr(col_count), ptr(off_dev), D, H, W, ptr(pos), stream_ptr(device))
        call("unopose_rle_diff", ptr(pos), ptr(off_dev), D, int(n.max()), H, W, ptr(counts), stream_ptr(device))
        flat = _to_host(counts)
    area = tot[:, 1].copy()
    bbox = []
    for d in range(D):
        if area[d] < 1:
            bbox.append(None)
        else:
            y0, y1, x0, x1 = H - tot[d, 2], tot[d, 3], W - tot[d, 4], tot[d, 5]
            bbox.append([int(x0), int(y0), int(x1 - x0), int(y1 - y0)])
    return [flat[off[d]:off[d + 1]] for d in range(D)], area, bbox


def window_masks(masks, windows, index=None, out=None):
    """The crop of decoded masks to their windows -> (packed uint8, row_counts int32) on the device: window k = (y0, y1, x0, x1) (or a
    `provider.Window`) of mask `index[k]` (default k), its h * w bytes (0 / 1, row-major) back to back in window order -- the layout
    `PrepPlan.masks` has -- and its set pixels per row, h entries per window in the same order (`row_off` order).  out: (packed,
    row_counts) to write into."""
    D, H, W = _require_masks(masks, "window_masks")
    K = len(windows)
    index = np.arange(K) if index is None else np.asarray(index, dtype=np.int64).reshape(-1)
    if K < 1 or K > 65535 or len(index) != K:
        raise ValueError(f"window_masks: {K} windows, {len(index)} mask numbers")
    if index.min() < 0 or index.max() >= D:
        raise ValueError("window_masks: mask number outside the masks")
    win = np.array([w.as_list() if hasattr(w, "as_list") else [int(v) for v in w] for w in windows], dtype=np.int64).reshape(K, 4)
    y0, y1, x0, x1 = win.T
    if not ((0 <= y0) & (y0 < y1) & (y1 <= H) & (0 <= x0) & (x0 < x1) & (x1 <= W)).all():
        raise ValueError(f"window_masks: window outside the {H} x {W} masks")
    h, w = y1 - y0, x1 - x0
    desc = np.zeros((K, _desc_ints()), dtype=np.int64)
    desc[:, 0], desc[:, 1], desc[:, 2], desc[:, 3], desc[:, 4] = index, y0, x0, h, w
    desc[:, 5], desc[:, 6] = np.cumsum(h * w) - h * w, np.cumsum(h) - h
    n_bytes, n_rows = int((h * w).sum()), int(h.sum())
    if n_bytes >= 2 ** 31:
        raise ValueError("window_masks: too many pixels for 32-bit offsets")
    device = masks.device
    desc_dev = torch.from_numpy(desc.astype(np.int32)).to(device)
    o = out if out is not None else (None, None)
    packed = _result(o[0], "window_masks: packed", torch.uint8, (n_bytes,), device)
    row_counts = _result(o[1], "window_masks: row_counts", torch.int32, (n_rows,), device)
    with on_device(device):
        call("unopose_window_masks", ptr(masks), ptr(desc_dev), K, int(h.max()), H, W, ptr(packed), ptr(row_counts), stream_ptr(device))
    return packed, row_counts
