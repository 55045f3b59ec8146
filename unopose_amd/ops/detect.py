"""Scoring mask proposals against reference views on the device (csrc/detmatch.hip): the kernels behind `unopose_amd.match_dets`, whose
numpy functions state the rule.  `patch_valid` and `mask_nms` equal `match_dets.patch_valid_host` / `nms_host` in every byte, flag and
count; `token_unit_rows`, `patch_match_score` and `class_cosine` are `unit_rows_host` / `appearance_host` / the class-token product in
bf16 data with fp32 accumulation.  No atomics: two calls return the same bits.  Inputs are CUDA tensors; there is no CPU path."""
import functools

import numpy as np
import torch

from .._lib import _D, call, lib, on_device, ptr, stream_ptr
from .prep import _require, _result

PATCH = 14


@functools.lru_cache(maxsize=None)
def _max_tokens():
    return int(lib().unopose_patch_match_max_tokens())


@functools.lru_cache(maxsize=None)
def _max_masks():
    return int(lib().unopose_mask_nms_max_masks())


def patch_valid(packed_masks, windows, img_size, out=None):
    """Which patches of the resized crops lie on their masks: `packed_masks` = the 0 / 1 bytes of K square windows back to back
    (`ops.window_masks` / `PrepPlan.masks`), `windows` = their (y0, y1, x0, x1) or `provider.Window`s -> (K, (img_size / 14)^2) uint8.
    Pixel (Y, X) of the resized crop reads window pixel (Y s // img_size, X s // img_size); a patch is valid iff twice the set pixels
    among its 14 x 14 reach 196."""
    _require(packed_masks, "patch_valid: packed_masks", torch.uint8)
    img_size = int(img_size)
    if img_size < PATCH or img_size > 4096 or img_size % PATCH:
        raise ValueError(f"patch_valid: img_size {img_size} is not a multiple of {PATCH} in [{PATCH}, 4096]")
    K = len(windows)
    if K < 1 or K > 65535:
        raise ValueError(f"patch_valid: {K} windows")
    win = np.array([w.as_list() if hasattr(w, "as_list") else [int(v) for v in w] for w in windows], dtype=np.int64).reshape(K, 4)
    h, w = win[:, 1] - win[:, 0], win[:, 3] - win[:, 2]
    if (h < 1).any() or (h != w).any():
        raise ValueError("patch_valid: windows must be square with a side of at least 1")
    off = np.cumsum(h * w) - h * w
    if packed_masks.dim() != 1 or int(packed_masks.numel()) != int((h * w).sum()) or packed_masks.numel() >= 2 ** 31:
        raise ValueError(f"patch_valid: {packed_masks.numel()} mask bytes for windows of {int((h * w).sum())} pixels")
    dev = packed_masks.device
    desc = torch.from_numpy(np.stack([off, h], axis=1).astype(np.int32)).to(dev)
    side = img_size // PATCH
    out = _result(out, "patch_valid: out", torch.uint8, (K, side * side), dev)
    with on_device(dev):
        call("unopose_patch_valid", ptr(packed_masks), ptr(desc), K, img_size, ptr(out), stream_ptr(dev))
    return out


def token_unit_rows(tokens, out=None):
    """tokens (N, T, D) bf16 or fp32 -> (N, T, D) bf16 rows of unit length: x / |x| with the norm in fp32 and one rounding; a row of
    norm 0 gives zeros."""
    if not torch.is_tensor(tokens) or not tokens.is_cuda:
        raise RuntimeError("token_unit_rows: tokens: CPU not supported")
    if tokens.dtype not in (torch.bfloat16, torch.float32) or tokens.dim() != 3 or not tokens.is_contiguous():
        raise RuntimeError("token_unit_rows: tokens must be a contiguous (N, T, D) bfloat16 or float32 tensor")
    N, T, D = (int(v) for v in tokens.shape)
    if N * T < 1 or D < 1 or N * T >= 2 ** 31:
        raise ValueError(f"token_unit_rows: tokens {tuple(tokens.shape)}")
    out = _result(out, "token_unit_rows: out", torch.bfloat16, (N, T, D), tokens.device)
    with on_device(tokens.device):
        call("unopose_token_unit_rows", ptr(tokens), int(tokens.dtype == torch.bfloat16), N * T, D, ptr(out), stream_ptr(tokens.device))
    return out


def _require_units(q_unit, q_valid, r_unit, r_valid, name):
    _require(q_unit, f"{name}: q_unit", torch.bfloat16)
    _require(r_unit, f"{name}: r_unit", torch.bfloat16)
    if q_unit.dim() != 3 or r_unit.dim() != 3 or q_unit.shape[1:] != r_unit.shape[1:]:
        raise RuntimeError(f"{name}: q_unit (P, T, D) and r_unit (O, T, D), not {tuple(q_unit.shape)} and {tuple(r_unit.shape)}")
    P, T, D = (int(v) for v in q_unit.shape)
    O = int(r_unit.shape[0])
    _require(q_valid, f"{name}: q_valid", torch.uint8, (P, T))
    _require(r_valid, f"{name}: r_valid", torch.uint8, (O, T))
    if r_unit.device != q_unit.device or q_valid.device != q_unit.device or r_valid.device != q_unit.device:
        raise RuntimeError(f"{name}: tensors on different devices")
    return P, O, T, D


def patch_match_score(q_unit, q_valid, r_unit, r_valid, out=None):
    """The appearance score s_appe (P, O) fp32 of P proposals against O objects: q_unit (P, T, D), r_unit (O, T, D) bf16 unit patch rows
    (`token_unit_rows`), q_valid (P, T), r_valid (O, T) uint8 (`patch_valid`): the mean over the valid patches i of p of the maximum over
    the valid patches j of o of q[p, i] . r[o, j]; 0 when either side has no valid patch.  The T x T products run on the matrix cores
    and are never stored.  D a multiple of 32."""
    P, O, T, D = _require_units(q_unit, q_valid, r_unit, r_valid, "patch_match_score")
    if min(P, O, T) < 1 or max(P, O) > 65535 or T > _max_tokens() or D < 32 or D % 32:
        raise ValueError(f"patch_match_score: P {P}, O {O}, T {T} (at most {_max_tokens()}), D {D} (a multiple of 32)")
    out = _result(out, "patch_match_score: out", torch.float32, (P, O), q_unit.device)
    with on_device(q_unit.device):
        call("unopose_patch_match_score", ptr(q_unit), ptr(q_valid), ptr(r_unit), ptr(r_valid), P, O, T, D, ptr(out), stream_ptr(q_unit.device))
    return out


def class_cosine(q_cls, r_cls, out=None):
    """The semantic score s_sem (P, O) fp32: q_cls (P, D), r_cls (O, D) bf16 unit class-token rows -> q_cls[p] . r_cls[o]."""
    _require(q_cls, "class_cosine: q_cls", torch.bfloat16)
    _require(r_cls, "class_cosine: r_cls", torch.bfloat16)
    if q_cls.dim() != 2 or r_cls.dim() != 2 or q_cls.shape[1] != r_cls.shape[1] or q_cls.device != r_cls.device:
        raise RuntimeError(f"class_cosine: q_cls (P, D) and r_cls (O, D) on one device, not {tuple(q_cls.shape)} and {tuple(r_cls.shape)}")
    P, D = (int(v) for v in q_cls.shape)
    O = int(r_cls.shape[0])
    if min(P, O, D) < 1 or max(P, O) > 65535:
        raise ValueError(f"class_cosine: P {P}, O {O}, D {D}")
    out = _result(out, "class_cosine: out", torch.float32, (P, O), q_cls.device)
    with on_device(q_cls.device):
        call("unopose_class_cosine", ptr(q_cls), ptr(r_cls), P, O, D, ptr(out), stream_ptr(q_cls.device))
    return out


def mask_nms(masks, category, score, nms_iou=0.5, max_per_object=0):
    """Suppression of overlapping proposals per category -> (keep (N,) uint8, area (N,) int32, inter (N, N) int32), all on the device.
    masks (N, H, W) uint8 or bool, non-zero = set; category (N,) int32; score (N,) float32 or float64 (compared as float64).  The
    proposals are walked by (score descending, number ascending); one is kept iff no kept proposal of its category has
    float(inter) > nms_iou * float(union) with it, and keep = 1 for the first `max_per_object` (0: all) kept ones of a category.
    area = set pixels; inter[i, j] = pixels set in both for two proposals of one category (the area on the diagonal), 0 otherwise."""
    from .rle import _require_masks

    N, H, W = _require_masks(masks, "mask_nms")
    dev = masks.device
    _require(category, "mask_nms: category", torch.int32, (N,))
    if not torch.is_tensor(score) or not score.is_cuda or score.dtype not in (torch.float32, torch.float64) or tuple(score.shape) != (N,):
        raise RuntimeError(f"mask_nms: score must be a float32 or float64 CUDA tensor of shape ({N},)")
    if category.device != dev or score.device != dev:
        raise RuntimeError("mask_nms: tensors on different devices")
    nms_iou, max_per_object = float(nms_iou), int(max_per_object)
    if N > _max_masks() or max_per_object < 0 or nms_iou != nms_iou:
        raise ValueError(f"mask_nms: {N} masks (at most {_max_masks()}), max_per_object {max_per_object}, nms_iou {nms_iou}")
    score = score.to(torch.float64).contiguous()
    bits = torch.empty((N, (H * W + 63) // 64), dtype=torch.int64, device=dev)
    area = torch.empty(N, dtype=torch.int32, device=dev)
    inter = torch.empty((N, N), dtype=torch.int32, device=dev)
    keep = torch.empty(N, dtype=torch.uint8, device=dev)
    with on_device(dev):
        call("unopose_mask_pair_counts", ptr(masks), ptr(category), N, H, W, ptr(bits), ptr(area), ptr(inter), stream_ptr(dev))
        call("unopose_mask_nms_walk", ptr(score), ptr(category), ptr(area), ptr(inter), N, _D(nms_iou), max_per_object, ptr(keep), stream_ptr(dev))
    return keep, area, inter
