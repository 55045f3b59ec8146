"""Per-image composition of the pose visualisation on the device (csrc/vis.hip): the toolkit's `visualization.vis_object_poses`
(third_party/bop_toolkit/bop_toolkit_lib/visualization.py:93-235) for renders that `render.HipColorRenderer` left on the GPU.  The stacks and
the photo are CUDA tensors; there is no CPU path.  Captions are not drawn here (`vis_poses` draws them on the host)."""
import functools

import torch

from .._lib import call, lib, on_device, ptr, stream_ptr

_INT_MAX = 2 ** 31 - 1


@functools.lru_cache(maxsize=None)
def _workspace_ints():
    return int(lib().unopose_vis_workspace_ints())


def _check(x, name, dtype, shape):
    if not torch.is_tensor(x) or not x.is_cuda:
        raise RuntimeError(f"{name}: CPU not supported")
    if x.dtype != dtype or not x.is_contiguous() or (shape is not None and tuple(x.shape) != tuple(shape)):
        raise RuntimeError(f"{name} must be a contiguous {dtype} tensor{'' if shape is None else ' ' + str(tuple(shape))}, not {x.dtype} {tuple(x.shape)}")
    return x


def compose_poses(rgbs, depths, photo, depth=None, resolve_visib=True, delta=15.0):
    """rgbs (P,H,W,3) uint8 and depths (P,H,W) float32: the renders of one image's poses, in pose order; photo (H,W,3) uint8; depth (H,W)
    float32: the captured depth in mm, or None.
    -> vis_rgb (H,W,3) uint8 (0.5 photo + 0.5 rendered layer + box outlines), boxes: per pose [x, y, w, h] as `misc.calc_2d_bbox` (None for a
    pose that draws nothing), ren_depth (H,W) float32 (depth of the nearest pose), depth_diff_rgb (H,W,3) uint8 or None without `depth`, stats
    = dict(min, max, mean) of rendered minus captured depth over the pixels where both are valid, or None without `depth` or without such a pixel.
    resolve_visib: each pixel of the rendered layer takes the nearest pose (the earliest at equal depth); False: the saturating sum of all renders.
    delta: the tolerance in mm below which the depth-difference image is red (`bop_eval.VSD_DELTA`, ITODD 5)."""
    _check(rgbs, "compose_poses: rgbs", torch.uint8, None)
    if rgbs.dim() != 4 or rgbs.shape[3] != 3 or rgbs.shape[0] < 1:
        raise RuntimeError(f"compose_poses: rgbs must be (P, H, W, 3), not {tuple(rgbs.shape)}")
    P, H, W, _ = rgbs.shape
    if P > 65535:
        raise ValueError(f"compose_poses: {P} poses per call (1 .. 65535)")
    _check(depths, "compose_poses: depths", torch.float32, (P, H, W))
    _check(photo, "compose_poses: photo", torch.uint8, (H, W, 3))
    if depth is not None:
        _check(depth, "compose_poses: depth", torch.float32, (H, W))
    dev = rgbs.device
    if any(t.device != dev for t in (depths, photo) + ((depth,) if depth is not None else ())):
        raise RuntimeError("compose_poses: the tensors live on different devices")
    boxes = torch.empty(P, 4, dtype=torch.int32, device=dev)
    ren_rgb = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
    vis_rgb = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
    ren_depth = torch.empty(H, W, dtype=torch.float32, device=dev)
    diff_rgb = stats_d = None
    with on_device(dev):
        call("unopose_vis_compose", ptr(rgbs), ptr(depths), P, H, W, ptr(photo), int(bool(resolve_visib)), ptr(boxes), ptr(ren_rgb), ptr(ren_depth),
             ptr(vis_rgb), stream_ptr(dev))
        if depth is not None:
            work = torch.empty(_workspace_ints() // 2, dtype=torch.int64, device=dev)
            diff_rgb = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
            stats_d = torch.empty(4, dtype=torch.float64, device=dev)
            call("unopose_vis_depth_diff", ptr(ren_depth), ptr(depth), H, W, float(delta), ptr(work), ptr(diff_rgb), ptr(stats_d), stream_ptr(dev))
    out_boxes = [None if b[2] < b[0] else [b[0], b[1], b[2] - b[0], b[3] - b[1]] for b in boxes.cpu().tolist()]
    stats = None
    if stats_d is not None:
        s = stats_d.cpu().tolist()
        if s[3] > 0:
            stats = dict(min=s[0], max=s[1], mean=s[2])
    return vis_rgb, out_boxes, ren_depth, diff_rgb, stats
