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


SHADED_CHUNK_BYTES = 256 << 20  # of key workspace alive at a time: 8 bytes per sample, ssaa^2 H W samples per view


class HipShadedRenderer:
    """Training views of an object model on csrc/raster_shade.hip (C ABI unopose_render_shaded): what the toolkit's
    scripts/render_train_imgs.py asks of its RGB renderer and of cv2 -- a Phong (or flat) shaded render of vertex colours, a surface colour
    or the model's texture at `ssaa` times the resolution, area-averaged down to (height, width) -- without the large image ever being
    stored.  `width`, `height` and the intrinsics handed to `render_batch` are those of the OUTPUT image; the kernel scales them.
    With shading="flat", ssaa=1 and no texture the bytes equal `HipColorRenderer`'s.  Depth stays with `HipDepthRenderer`."""

    def __init__(self, width, height, device="cuda:0", ambient=0.5, shading="phong", ssaa=4, chunk_bytes=SHADED_CHUNK_BYTES):
        if shading not in ("phong", "flat"):
            raise ValueError(f"HipShadedRenderer: shading {shading!r} (phong or flat)")
        if int(ssaa) != ssaa or not 1 <= int(ssaa) <= 4:
            raise ValueError(f"HipShadedRenderer: ssaa {ssaa!r} (an integer from 1 to 4)")
        self.W, self.H, self.device, self.ambient = int(width), int(height), torch.device(device), float(ambient)
        self.shading, self.ssaa, self.chunk_bytes = shading, int(ssaa), int(chunk_bytes)
        self.models = {}

    def add_object(self, obj_id, verts, faces, normals=None, colors=None, texture=None, texture_uv=None, surf_color=None):
        """verts (V,3), faces (F,3) as for `HipColorRenderer`; `normals` (V,3), any length (a zero normal leaves a vertex without a diffuse
        share), required for Phong shading; the colour is ONE of `texture` (Ht,Wt,3 or 4) uint8 as read from the image file (top row first)
        with `texture_uv` (V,2), `colors` (V,3) floats in [0,1], `surf_color` (3 floats in [0,1]), or mid grey."""
        if self.device.type != "cuda":
            raise RuntimeError("HipShadedRenderer: CPU not supported")
        if sum(x is not None for x in (colors, texture, surf_color)) > 1:
            raise ValueError("add_object: one of colors, texture, surf_color")
        if (texture is None) != (texture_uv is None):
            raise ValueError("add_object: texture and texture_uv go together")
        v = np.ascontiguousarray(np.asarray(verts, np.float32))
        f = np.ascontiguousarray(np.asarray(faces, np.int32))
        if v.ndim != 2 or v.shape[1] != 3 or v.shape[0] < 3 or f.ndim != 2 or f.shape[1] != 3 or f.shape[0] < 1 or not np.isfinite(v).all():
            raise ValueError("add_object: verts must be (V >= 3, 3) finite floats and faces (F >= 1, 3)")
        if int(f.min()) < 0 or int(f.max()) >= v.shape[0]:
            raise ValueError(f"add_object: face index outside the {v.shape[0]} vertices")

        def per_vertex(a, width, name, unit):
            a = np.ascontiguousarray(np.asarray(a, np.float32))
            if a.shape != (v.shape[0], width) or not np.isfinite(a).all() or (unit and (a.min() < 0 or a.max() > 1)):
                raise ValueError(f"add_object: {name} must be {(v.shape[0], width)} finite floats" + (" in [0, 1]" if unit else ""))
            return torch.as_tensor(a).to(self.device)

        n = c = uv = tex = None
        if normals is not None:
            n = per_vertex(normals, 3, "normals", False)
        elif self.shading == "phong":
            raise ValueError("add_object: Phong shading needs normals (bop_eval.read_ply_model computes them where the file has none)")
        if colors is not None:
            c = per_vertex(colors, 3, "colors", True)
        if texture is not None:
            uv = per_vertex(texture_uv, 2, "texture_uv", False)
            t = np.asarray(texture)
            if t.dtype != np.uint8 or t.ndim != 3 or t.shape[2] not in (3, 4) or t.shape[0] < 1 or t.shape[1] < 1:
                raise ValueError("add_object: texture must be a (Ht, Wt, 3 or 4) uint8 image")
            tex = torch.as_tensor(np.ascontiguousarray(t[:, :, :3].astype(np.float32) / np.float32(255.0))).to(self.device)
        s = np.asarray((0.5, 0.5, 0.5) if surf_color is None else surf_color, np.float32).reshape(-1)
        if s.shape != (3,) or not (np.isfinite(s).all() and s.min() >= 0 and s.max() <= 1):
            raise ValueError("add_object: surf_color must be 3 floats in [0, 1]")
        self.models[obj_id] = (torch.as_tensor(v).to(self.device), torch.as_tensor(f).to(self.device), n, c, uv, tex, tuple(float(x) for x in s))

    def views_per_chunk(self):
        """Views rendered per launch: as many as keep the key workspace within `chunk_bytes`, one at least."""
        return int(min(max(1, self.chunk_bytes // (8 * self.ssaa * self.ssaa * self.H * self.W)), 65535))

    def render_batch(self, obj_id, Rs, ts, K4, out=None):
        """Rs (P,3,3), ts (P,3), K4 (P,4) or (4,) = fx, fy, cx, cy of the output image -> rgb (P,H,W,3) uint8 on the device: a new tensor, or
        `out`, contiguous and of that shape.  Inputs are host arrays or tensors on the renderer's device.  The views go through the kernel in
        chunks of `views_per_chunk()`; the result does not depend on the chunking."""
        for name, x in (("Rs", Rs), ("ts", ts), ("K4", K4)):
            if torch.is_tensor(x) and not x.is_cuda:
                raise RuntimeError(f"render_batch: {name}: CPU not supported")
        v, f, n, c, uv, tex, s = self.models[obj_id]

        def dev(x, width):
            x = x.detach().to(torch.float32) if torch.is_tensor(x) else torch.as_tensor(np.asarray(x, np.float32))
            return x.reshape(-1, width)

        Rs, ts = dev(Rs, 9), dev(ts, 3)
        P = Rs.shape[0]
        if P < 1 or ts.shape[0] != P:
            raise RuntimeError(f"render_batch: {P} rotations and {ts.shape[0]} translations")
        Rt = torch.cat([Rs.to(self.device), ts.to(self.device)], 1).contiguous()
        K4 = dev(K4, 4)
        K4 = (K4.expand(P, 4) if K4.shape[0] == 1 else K4).contiguous().to(self.device)
        if K4.shape[0] != P:
            raise RuntimeError(f"render_batch: {K4.shape[0]} intrinsics for {P} views")
        shape = (P, self.H, self.W, 3)
        if out is None:
            rgb = torch.empty(shape, dtype=torch.uint8, device=self.device)
        else:
            if not torch.is_tensor(out) or not out.is_cuda:
                raise RuntimeError("render_batch: out: CPU not supported")
            if out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous() or out.device != Rt.device:
                raise RuntimeError(f"render_batch: out must be a contiguous torch.uint8 tensor {shape} on {Rt.device}, not {out.dtype} {tuple(out.shape)} on {out.device}")
            rgb = out
        step = self.views_per_chunk()
        keys = torch.empty(min(step, P) * self.ssaa * self.ssaa * self.H * self.W, dtype=torch.int64, device=self.device)
        with on_device(self.device):
            for a in range(0, P, step):
                b = min(a + step, P)
                call("unopose_render_shaded", ptr(v), v.shape[0], ptr(f), f.shape[0], ptr(n) if n is not None else None,
                     ptr(c) if c is not None else None, ptr(uv) if uv is not None else None, ptr(tex) if tex is not None else None,
                     tex.shape[0] if tex is not None else 0, tex.shape[1] if tex is not None else 0, s[0], s[1], s[2], self.ambient,
                     int(self.shading == "phong"), self.ssaa, ptr(Rt[a:b]), ptr(K4[a:b]), b - a, self.H, self.W, ptr(keys), ptr(rgb[a:b]),
                     stream_ptr(self.device))
        return rgb

    def render_object(self, obj_id, R, t, fx, fy, cx, cy):
        """bop_toolkit's renderer interface, with the intrinsics of the output image."""
        c = self.render_batch(obj_id, np.asarray(R).reshape(1, 3, 3), np.asarray(t).reshape(1, 3), [fx, fy, cx, cy])
        return {"rgb": c[0].cpu().numpy()}
