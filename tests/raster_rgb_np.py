"""Test infrastructure: numpy mirrors of the colour rasteriser (csrc/raster_color.hip) and of the per-image composition (csrc/vis.hip),
in float32 -- float64 where csrc/vis.hip says so -- operation for operation (same expression order, no fused multiply-adds, division and
square root correctly rounded on both sides): the HIP kernels must reproduce these arrays bit for bit.  `NumpyColorRenderer` is also the
`renderer` handed to bop_toolkit_lib.visualization.vis_object_poses when tests/golden/vis_poses.npz is generated
(tests/golden/make_vis_poses_golden.py), so that the toolkit and `compose` work on the SAME renders."""
import numpy as np

f32 = np.float32
AMBIENT = 0.5
GREY = (0.5, 0.5, 0.5)


def render_rgbd(verts, faces, R, t, fx, fy, cx, cy, H, W, colors=None, surf_color=GREY, ambient=AMBIENT):
    """-> depth (H,W) float32 (equal to raster_np.render_depth), rgb (H,W,3) uint8.  The nearest face wins a pixel, the lowest face
    index at equal depth; flat shading with the light at the camera origin, w = min(1, ambient + |n . Pc| / (|n| |Pc|))."""
    verts, R, t = np.asarray(verts, f32), np.asarray(R, f32).reshape(3, 3), np.asarray(t, f32).reshape(3)
    faces = np.asarray(faces).reshape(-1, 3)
    fx, fy, cx, cy, ambient = f32(fx), f32(fy), f32(cx), f32(cy), f32(ambient)
    q = verts
    X = R[0, 0] * q[:, 0] + R[0, 1] * q[:, 1] + R[0, 2] * q[:, 2] + t[0]
    Y = R[1, 0] * q[:, 0] + R[1, 1] * q[:, 1] + R[1, 2] * q[:, 2] + t[1]
    Z = R[2, 0] * q[:, 0] + R[2, 1] * q[:, 1] + R[2, 2] * q[:, 2] + t[2]
    with np.errstate(divide="ignore", invalid="ignore"):
        U = fx * X / Z + cx
        V = fy * Y / Z + cy
    zbuf = np.full((H, W), np.inf, f32)
    winner = np.full((H, W), -1, np.int64)
    one = f32(1.0)
    for fi, tri in enumerate(faces):
        z3 = Z[tri]
        if not (z3 > f32(1e-6)).all():
            continue
        u, v = U[tri], V[tri]
        area = (u[1] - u[0]) * (v[2] - v[0]) - (u[2] - u[0]) * (v[1] - v[0])
        if abs(area) < f32(1e-12):
            continue
        x0, x1 = max(0, int(np.ceil(u.min()))), min(W - 1, int(np.floor(u.max())))
        y0, y1 = max(0, int(np.ceil(v.min()))), min(H - 1, int(np.floor(v.max())))
        if x1 < x0 or y1 < y0:
            continue
        inv = one / area
        iz = one / z3
        px, py = np.meshgrid(np.arange(x0, x1 + 1, dtype=f32), np.arange(y0, y1 + 1, dtype=f32))
        b0 = ((u[1] - px) * (v[2] - py) - (u[2] - px) * (v[1] - py)) * inv
        b1 = ((u[2] - px) * (v[0] - py) - (u[0] - px) * (v[2] - py)) * inv
        b2 = one - b0 - b1
        inside = (b0 >= 0) & (b1 >= 0) & (b2 >= 0)
        with np.errstate(divide="ignore"):
            z = one / (b0 * iz[0] + b1 * iz[1] + b2 * iz[2])
        sub, wsub = zbuf[y0:y1 + 1, x0:x1 + 1], winner[y0:y1 + 1, x0:x1 + 1]
        upd = inside & (z > 0) & (z < sub)  # faces in index order: at equal depth the lower index stays
        sub[upd] = z[upd]
        wsub[upd] = fi
    rgb = np.zeros((H, W, 3), np.uint8)
    ys, xs = (winner >= 0).nonzero()
    if len(ys):
        tri = faces[winner[ys, xs]]  # (n, 3)
        Xc, Yc, Zc, u, v = X[tri], Y[tri], Z[tri], U[tri], V[tri]
        area = (u[:, 1] - u[:, 0]) * (v[:, 2] - v[:, 0]) - (u[:, 2] - u[:, 0]) * (v[:, 1] - v[:, 0])
        inv = one / area
        iz = one / Zc
        px, py = xs.astype(f32), ys.astype(f32)
        b0 = ((u[:, 1] - px) * (v[:, 2] - py) - (u[:, 2] - px) * (v[:, 1] - py)) * inv
        b1 = ((u[:, 2] - px) * (v[:, 0] - py) - (u[:, 0] - px) * (v[:, 2] - py)) * inv
        b2 = one - b0 - b1
        z = one / (b0 * iz[:, 0] + b1 * iz[:, 1] + b2 * iz[:, 2])
        assert np.array_equal(z, zbuf[ys, xs])
        e1x, e1y, e1z = Xc[:, 1] - Xc[:, 0], Yc[:, 1] - Yc[:, 0], Zc[:, 1] - Zc[:, 0]
        e2x, e2y, e2z = Xc[:, 2] - Xc[:, 0], Yc[:, 2] - Yc[:, 0], Zc[:, 2] - Zc[:, 0]
        nx, ny, nz = e1y * e2z - e1z * e2y, e1z * e2x - e1x * e2z, e1x * e2y - e1y * e2x
        pcx, pcy = (px - cx) / fx * z, (py - cy) / fy * z
        dot = nx * pcx + ny * pcy + nz * z
        length = np.sqrt(nx * nx + ny * ny + nz * nz) * np.sqrt(pcx * pcx + pcy * pcy + z * z)
        with np.errstate(divide="ignore", invalid="ignore"):
            cosine = np.where(length > 0, np.abs(dot) / length, f32(0.0)).astype(f32)
        w = np.minimum(one, ambient + cosine)
        if colors is None:
            col = np.broadcast_to(np.asarray(surf_color, f32).reshape(1, 3), (len(ys), 3))
        else:
            c = np.asarray(colors, f32)[tri]  # (n, 3 vertices, 3 channels)
            w0, w1, w2 = (b0 * iz[:, 0])[:, None], (b1 * iz[:, 1])[:, None], (b2 * iz[:, 2])[:, None]
            col = (w0 * c[:, 0] + w1 * c[:, 1] + w2 * c[:, 2]) * z[:, None]
        s = np.minimum(np.maximum(w[:, None] * col, f32(0.0)), one)
        val = s * f32(255.0) + f32(0.5)
        assert val.dtype == f32
        rgb[ys, xs] = val.astype(np.int32).astype(np.uint8)
    zbuf[np.isinf(zbuf)] = 0
    return zbuf, rgb


class NumpyColorRenderer:
    """bop_toolkit renderer interface ({"rgb", "depth"}) on top of `render_rgbd`."""

    def __init__(self, width, height, ambient=AMBIENT):
        self.W, self.H, self.ambient, self.models = width, height, ambient, {}

    def add_object(self, obj_id, verts, faces, colors=None, surf_color=None):
        self.models[obj_id] = (np.asarray(verts, f32), np.asarray(faces, np.int32), None if colors is None else np.asarray(colors, f32),
                               GREY if surf_color is None else tuple(surf_color))

    def render_object(self, obj_id, R, t, fx, fy, cx, cy):
        v, f, c, s = self.models[obj_id]
        d, rgb = render_rgbd(v, f, R, np.asarray(t).reshape(3), fx, fy, cx, cy, self.H, self.W, colors=c, surf_color=s, ambient=self.ambient)
        return {"rgb": rgb, "depth": d}


def depth_diff_image(ren_depth, depth, delta=15.0):
    """The depth-difference image of csrc/vis.hip -> (image (H,W,3) uint8, stats dict(min, max, mean) or None)."""
    ren_depth, depth = np.asarray(ren_depth, f32), np.asarray(depth, f32)
    valid = (depth > 0) & (ren_depth > 0)
    diff = valid.astype(f32) * (ren_depth - depth)
    image = np.zeros(depth.shape + (3,), np.uint8)
    if not valid.any():
        return image, None
    image[..., 0] = np.where(valid & (diff < f32(delta)), 255, 0)
    shifted = diff - diff.min()
    mask = shifted > 0
    lo = float(shifted[mask].min()) if mask.any() else 0.0
    rng = float(shifted[mask].max()) - lo if mask.any() else 0.0
    if not rng > 0.0:
        g = np.full(depth.shape, 51, np.uint8)  # the toolkit is undefined here: 255 * valid_start
    else:
        v = shifted.astype(np.float64)
        v[mask] -= lo
        v[mask] /= rng / (1.0 - 0.2)
        v[mask] += 0.2
        g = (255.0 * v).astype(np.uint8)
    g = np.where(valid, g, 0).astype(np.uint8)
    image[..., 1] = image[..., 2] = g
    d = diff[valid]
    return image, dict(min=float(d.min()), max=float(d.max()), mean=float(d.astype(np.float64).sum() / d.size))


def compose(rgbs, depths, photo, depth=None, resolve_visib=True, delta=15.0):
    """The composition of csrc/vis.hip for the (P,H,W,3) uint8 / (P,H,W) float32 renders of one image, pose by pose
    -> vis_rgb, boxes ([x, y, w, h] or None per pose), ren_depth, depth_diff_rgb or None, stats or None."""
    rgbs, depths, photo = np.asarray(rgbs, np.uint8), np.asarray(depths, f32), np.asarray(photo, np.uint8)
    P, H, W, _ = rgbs.shape
    ren = np.zeros((H, W, 3), np.uint8)
    info = np.zeros((H, W), f32)
    ren_depth = np.zeros((H, W), f32)
    boxes = []
    yy, xx = np.mgrid[0:H, 0:W]
    for p in range(P):
        m = depths[p]
        take = (m != 0) & ((ren_depth == 0) | (m < ren_depth))
        ren_depth[take] = m[take]
        if resolve_visib:
            ren[take] = rgbs[p][take]
        else:
            s = ren.astype(f32) + rgbs[p].astype(f32)
            ren = np.where(s > 255, f32(255), s).astype(np.uint8)
        drawn = (rgbs[p] > 0).any(axis=2)
        if not drawn.any():
            boxes.append(None)
            continue
        ys, xs = drawn.nonzero()
        x0, y0, x1, y1 = int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())
        boxes.append([x0, y0, x1 - x0, y1 - y0])
        within = (xx >= x0) & (xx <= x1) & (yy >= y0) & (yy <= y1)
        info[within & ((xx == x0) | (xx == x1) | (yy == y0) | (yy == y1))] = 76  # int(0.3 * 255)
    blend = f32(0.5) * photo.astype(f32) + f32(0.5) * ren.astype(f32) + f32(1.0) * info[..., None]
    vis = np.where(blend > 255, f32(255), blend).astype(np.uint8)
    if depth is None:
        return vis, boxes, ren_depth, None, None
    image, stats = depth_diff_image(ren_depth, depth, delta)
    return vis, boxes, ren_depth, image, stats
