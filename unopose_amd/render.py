"""Depth renderer for BOP's VSD error on the HIP rasteriser (csrc/raster.hip, C ABI unopose_render_depth).

The reference's evaluation (bop_toolkit `eval_bop19_pose.py`, tabulated by core/unopose/engine/bop_eval_utils.py:340-454) hands
`pose_error.vsd` a renderer object with `render_object(obj_id, R, t, fx, fy, cx, cy) -> {"depth": (H,W)}`; this class offers that
call (so it can also be passed to the toolkit itself) plus a batched form for many poses of one object."""
import numpy as np
import torch

from ._lib import call, on_device, ptr, stream_ptr


class HipDepthRenderer:
    def __init__(self, width, height, device="cuda:0"):
        self.W, self.H, self.device = int(width), int(height), torch.device(device)
        self.models = {}

    def add_object(self, obj_id, verts, faces):
        """verts (V,3) in model units (mm for BOP), faces (F,3) vertex indices."""
        v = torch.as_tensor(np.asarray(verts, np.float32)).contiguous().to(self.device)
        f = torch.as_tensor(np.asarray(faces, np.int32)).contiguous().to(self.device)
        assert v.dim() == 2 and v.shape[1] == 3 and f.dim() == 2 and f.shape[1] == 3 and int(f.max()) < v.shape[0]
        self.models[obj_id] = (v, f)

    def render_batch(self, obj_id, Rs, ts, K4, out=None):
        """Rs (P,3,3), ts (P,3), K4 (P,4) or (4,) = fx, fy, cx, cy -> depth (P,H,W) float32 tensor on the device: a new one, or `out`
        (contiguous, of that shape, on the device) for a caller that renders several objects into one stack."""
        v, f = self.models[obj_id]
        Rs = torch.as_tensor(np.asarray(Rs, np.float32)).reshape(-1, 9)
        ts = torch.as_tensor(np.asarray(ts, np.float32)).reshape(-1, 3)
        P = Rs.shape[0]
        Rt = torch.cat([Rs, ts], 1).contiguous().to(self.device)
        K4 = torch.as_tensor(np.asarray(K4, np.float32)).reshape(-1, 4)
        K4 = (K4.expand(P, 4) if K4.shape[0] == 1 else K4).contiguous().to(self.device)
        if out is None:
            depth = torch.empty(P, self.H, self.W, dtype=torch.float32, device=self.device)
        else:
            if out.dtype != torch.float32 or tuple(out.shape) != (P, self.H, self.W) or not out.is_contiguous() or out.device != Rt.device:
                raise RuntimeError(f"render_batch: out must be a contiguous float32 tensor {(P, self.H, self.W)} on {Rt.device}, not {out.dtype} {tuple(out.shape)} on {out.device}")
            depth = out
        with on_device(self.device):
            call("unopose_render_depth", ptr(v), v.shape[0], ptr(f), f.shape[0], ptr(Rt), ptr(K4), P, self.H, self.W, ptr(depth),
                 stream_ptr(self.device))
        return depth

    def render_object(self, obj_id, R, t, fx, fy, cx, cy):
        """bop_toolkit's renderer interface."""
        d = self.render_batch(obj_id, np.asarray(R).reshape(1, 3, 3), np.asarray(t).reshape(1, 3), [fx, fy, cx, cy])
        return {"depth": d[0].cpu().numpy()}


class HipColorRenderer:
    """Colour + depth renderer for the pose visualisation on csrc/raster_color.hip (C ABI unopose_render_color): what the toolkit's
    `visualization.vis_object_poses` asks of its renderer (`render_object(...) -> {"rgb", "depth"}`), flat-shaded as the toolkit's OpenGL
    renderer shades (light at the camera, `ambient` 0.5), plus the batched form.  The depth equals `HipDepthRenderer`'s bit for bit."""

    def __init__(self, width, height, device="cuda:0", ambient=0.5):
        self.W, self.H, self.device, self.ambient = int(width), int(height), torch.device(device), float(ambient)
        self.models = {}

    def add_object(self, obj_id, verts, faces, colors=None, surf_color=None):
        """verts (V,3) in model units, faces (F,3) vertex indices; `colors` (V,3) floats in [0,1], interpolated over a face, or one
        `surf_color` (3 floats in [0,1]) used as is; neither: mid grey, both: an error."""
        if colors is not None and surf_color is not None:
            raise ValueError("add_object: colors or surf_color, not both")
        v = torch.as_tensor(np.asarray(verts, np.float32)).contiguous().to(self.device)
        f = torch.as_tensor(np.asarray(faces, np.int32)).contiguous().to(self.device)
        assert v.dim() == 2 and v.shape[1] == 3 and v.shape[0] >= 3 and f.dim() == 2 and f.shape[1] == 3 and f.shape[0] >= 1
        assert int(f.min()) >= 0 and int(f.max()) < v.shape[0]
        c = None
        if colors is not None:
            c = np.asarray(colors, np.float32)
            if c.shape != (v.shape[0], 3) or not (np.isfinite(c).all() and c.min() >= 0 and c.max() <= 1):
                raise ValueError(f"add_object: colors must be {(v.shape[0], 3)} floats in [0, 1]")
            c = torch.as_tensor(c).contiguous().to(self.device)
        s = np.asarray((0.5, 0.5, 0.5) if surf_color is None else surf_color, np.float32).reshape(-1)
        if s.shape != (3,) or not (np.isfinite(s).all() and s.min() >= 0 and s.max() <= 1):
            raise ValueError("add_object: surf_color must be 3 floats in [0, 1]")
        self.models[obj_id] = (v, f, c, tuple(float(x) for x in s))

    def render_batch(self, obj_id, Rs, ts, K4, out=None):
        """Rs (P,3,3), ts (P,3), K4 (P,4) or (4,) = fx, fy, cx, cy -> (depth (P,H,W) float32, rgb (P,H,W,3) uint8) on the device: new
        tensors, or `out` = (depth, rgb), contiguous and of those shapes (slices of one stack for a caller that renders several objects)."""
        v, f, c, s = self.models[obj_id]
        Rs = torch.as_tensor(np.asarray(Rs, np.float32)).reshape(-1, 9)
        ts = torch.as_tensor(np.asarray(ts, np.float32)).reshape(-1, 3)
        P = Rs.shape[0]
        Rt = torch.cat([Rs, ts], 1).contiguous().to(self.device)
        K4 = torch.as_tensor(np.asarray(K4, np.float32)).reshape(-1, 4)
        K4 = (K4.expand(P, 4) if K4.shape[0] == 1 else K4).contiguous().to(self.device)
        if out is None:
            depth = torch.empty(P, self.H, self.W, dtype=torch.float32, device=self.device)
            rgb = torch.empty(P, self.H, self.W, 3, dtype=torch.uint8, device=self.device)
        else:
            depth, rgb = out
            for t, dt, shape in ((depth, torch.float32, (P, self.H, self.W)), (rgb, torch.uint8, (P, self.H, self.W, 3))):
                if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or t.device != Rt.device:
                    raise RuntimeError(f"render_batch: out must hold a contiguous {dt} tensor {shape} on {Rt.device}, not {t.dtype} {tuple(t.shape)} on {t.device}")
        keys = torch.empty(P * self.H * self.W, dtype=torch.int64, device=self.device)
        with on_device(self.device):
            call("unopose_render_color", ptr(v), v.shape[0], ptr(f), f.shape[0], ptr(c) if c is not None else None, s[0], s[1], s[2], self.ambient,
                 ptr(Rt), ptr(K4), P, self.H, self.W, ptr(keys), ptr(depth), ptr(rgb), stream_ptr(self.device))
        return depth, rgb

    def render_object(self, obj_id, R, t, fx, fy, cx, cy):
        """bop_toolkit's renderer interface."""
        d, c = self.render_batch(obj_id, np.asarray(R).reshape(1, 3, 3), np.asarray(t).reshape(1, 3), [fx, fy, cx, cy])
        return {"rgb": c[0].cpu().numpy(), "depth": d[0].cpu().numpy()}
