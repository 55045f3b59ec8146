"""The host form of the shaded, textured, supersampled rasteriser (csrc/raster_shade.hip): numpy in float32, operation for operation -- the
expression order of csrc/raster_keys.h and of the resolve kernel, no fused multiply-adds, division and square root correctly rounded on both
sides.  It is the specification the HIP kernel reproduces bit for bit (tests/test_render_train_gpu.py, through tests/raster_shade_np.py) and
the renderer of `python -m unopose_amd.render_train --host`.  `dt=np.float64` runs the same chain in double precision on the float32
inputs, to see how far float32's rounding carries."""
import numpy as np

AMBIENT = 0.5
GREY = (0.5, 0.5, 0.5)
f32 = np.float32


def _unit(x, y, z, dt):
    """v / |v|, the zero vector where |v| is not positive."""
    length = np.sqrt(x * x + y * y + z * z)
    ok = length > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        return [np.where(ok, c / length, dt(0.0)).astype(dt) for c in (x, y, z)]


def _visibility(verts, faces, R, t, fx, fy, cx, cy, sH, sW, dt):
    """csrc/raster_keys.h on an sH x sW grid: the camera-space vertices X, Y, Z, their projections U, V, the depth of the nearest face per
    sample (inf: none) and its index (-1: none; the lowest index at equal depth)."""
    one = dt(1.0)
    q = verts
    X = R[0, 0] * q[:, 0] + R[0, 1] * q[:, 1] + R[0, 2] * q[:, 2] + t[0]
    Y = R[1, 0] * q[:, 0] + R[1, 1] * q[:, 1] + R[1, 2] * q[:, 2] + t[1]
    Z = R[2, 0] * q[:, 0] + R[2, 1] * q[:, 1] + R[2, 2] * q[:, 2] + t[2]
    with np.errstate(divide="ignore", invalid="ignore"):
        U = fx * X / Z + cx
        V = fy * Y / Z + cy
    zbuf = np.full((sH, sW), np.inf, dt)
    winner = np.full((sH, sW), -1, np.int64)
    for fi, tri in enumerate(faces):
        z3 = Z[tri]
        if not (z3 > dt(f32(1e-6))).all():
            continue
        u, v = U[tri], V[tri]
        area = (u[1] - u[0]) * (v[2] - v[0]) - (u[2] - u[0]) * (v[1] - v[0])
        if abs(area) < dt(f32(1e-12)):
            continue
        x0, x1 = max(0, int(np.ceil(u.min()))), min(sW - 1, int(np.floor(u.max())))
        y0, y1 = max(0, int(np.ceil(v.min()))), min(sH - 1, int(np.floor(v.max())))
        if x1 < x0 or y1 < y0:
            continue
        inv = one / area
        iz = one / z3
        px, py = np.meshgrid(np.arange(x0, x1 + 1).astype(dt), np.arange(y0, y1 + 1).astype(dt))
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
    return X, Y, Z, U, V, zbuf, winner


def render_depth(verts, faces, R, t, fx, fy, cx, cy, H, W):
    """-> depth (H,W) float32, 0 where nothing projects: the values csrc/raster.hip (`render.HipDepthRenderer`) writes."""
    verts, R, t = np.asarray(verts, f32), np.asarray(R, f32).reshape(3, 3), np.asarray(t, f32).reshape(3)
    zbuf = _visibility(verts, np.asarray(faces).reshape(-1, 3), R, t, f32(fx), f32(fy), f32(cx), f32(cy), H, W, f32)[5]
    zbuf[np.isinf(zbuf)] = 0
    return zbuf


def render_shaded(verts, faces, R, t, fx, fy, cx, cy, H, W, normals=None, colors=None, texture=None, texture_uv=None, surf_color=GREY,
                  ambient=AMBIENT, shading="phong", ssaa=1, dt=f32, samples=False):
    """-> rgb (H,W,3) uint8 of one view, the intrinsics those of the H x W output; with `samples` the (ssaa H, ssaa W, 3) sample bytes instead.
    `texture` (Ht,Wt,3) uint8 as read from the file (top row first)."""
    assert shading in ("phong", "flat") and ssaa in (1, 2, 3, 4)
    assert sum(x is not None for x in (colors, texture)) <= 1 and (texture is None) == (texture_uv is None)
    verts, R, t = np.asarray(verts, f32).astype(dt), np.asarray(R, f32).reshape(3, 3).astype(dt), np.asarray(t, f32).reshape(3).astype(dt)
    faces = np.asarray(faces).reshape(-1, 3)
    s = dt(f32(ssaa))
    fx, fy, cx, cy, ambient = dt(f32(fx)) * s, dt(f32(fy)) * s, dt(f32(cx)) * s, dt(f32(cy)) * s, dt(f32(ambient))
    sH, sW = H * ssaa, W * ssaa
    one, zero = dt(1.0), dt(0.0)
    X, Y, Z, U, V, zbuf, winner = _visibility(verts, faces, R, t, fx, fy, cx, cy, sH, sW, dt)
    # resolve: the covered samples
    img = np.zeros((sH, sW, 3), np.uint8)
    ys, xs = (winner >= 0).nonzero()
    if len(ys):
        tri = faces[winner[ys, xs]]  # (n, 3)
        Xc, Yc, Zc, u, v = X[tri], Y[tri], Z[tri], U[tri], V[tri]
        area = (u[:, 1] - u[:, 0]) * (v[:, 2] - v[:, 0]) - (u[:, 2] - u[:, 0]) * (v[:, 1] - v[:, 0])
        inv = one / area
        iz = one / Zc
        px, py = xs.astype(dt), ys.astype(dt)
        b0 = ((u[:, 1] - px) * (v[:, 2] - py) - (u[:, 2] - px) * (v[:, 1] - py)) * inv
        b1 = ((u[:, 2] - px) * (v[:, 0] - py) - (u[:, 0] - px) * (v[:, 2] - py)) * inv
        b2 = one - b0 - b1
        z = one / (b0 * iz[:, 0] + b1 * iz[:, 1] + b2 * iz[:, 2])
        assert np.array_equal(z, zbuf[ys, xs])
        w0, w1, w2 = b0 * iz[:, 0], b1 * iz[:, 1], b2 * iz[:, 2]
        if shading == "phong":
            n = np.asarray(normals, f32).astype(dt)
            nh = _unit(R[0, 0] * n[:, 0] + R[0, 1] * n[:, 1] + R[0, 2] * n[:, 2], R[1, 0] * n[:, 0] + R[1, 1] * n[:, 1] + R[1, 2] * n[:, 2],
                       R[2, 0] * n[:, 0] + R[2, 1] * n[:, 1] + R[2, 2] * n[:, 2], dt)
            lh = _unit(-X, -Y, -Z, dt)
            a0, a1, a2 = w0 * z, w1 * z, w2 * z
            N = _unit(*[a0 * c[tri[:, 0]] + a1 * c[tri[:, 1]] + a2 * c[tri[:, 2]] for c in nh], dt)
            L = _unit(*[a0 * c[tri[:, 0]] + a1 * c[tri[:, 1]] + a2 * c[tri[:, 2]] for c in lh], dt)
            w = np.minimum(one, ambient + np.maximum(zero, N[0] * L[0] + N[1] * L[1] + N[2] * L[2]))
        else:  # csrc/raster_keys.h raster_flat_weight
            e1x, e1y, e1z = Xc[:, 1] - Xc[:, 0], Yc[:, 1] - Yc[:, 0], Zc[:, 1] - Zc[:, 0]
            e2x, e2y, e2z = Xc[:, 2] - Xc[:, 0], Yc[:, 2] - Yc[:, 0], Zc[:, 2] - Zc[:, 0]
            nx, ny, nz = e1y * e2z - e1z * e2y, e1z * e2x - e1x * e2z, e1x * e2y - e1y * e2x
            pcx, pcy = (px - cx) / fx * z, (py - cy) / fy * z
            dot = nx * pcx + ny * pcy + nz * z
            length = np.sqrt(nx * nx + ny * ny + nz * nz) * np.sqrt(pcx * pcx + pcy * pcy + z * z)
            with np.errstate(divide="ignore", invalid="ignore"):
                cosine = np.where(length > 0, np.abs(dot) / length, zero).astype(dt)
            w = np.minimum(one, ambient + cosine)
        if texture is not None:
            tex = np.asarray(texture)
            assert tex.dtype == np.uint8 and tex.ndim == 3
            tex = (tex[:, :, :3].astype(f32) / f32(255.0)).astype(dt)
            Ht, Wt = tex.shape[:2]
            uv = np.asarray(texture_uv, f32).astype(dt)[tri]  # (n, 3 vertices, 2)
            tu = (w0 * uv[:, 0, 0] + w1 * uv[:, 1, 0] + w2 * uv[:, 2, 0]) * z
            tv = (w0 * uv[:, 0, 1] + w1 * uv[:, 1, 1] + w2 * uv[:, 2, 1]) * z
            col = np.fmin(np.fmax(np.floor(tu * dt(f32(Wt))), zero), dt(f32(Wt - 1))).astype(np.int64)
            row = Ht - 1 - np.fmin(np.fmax(np.floor(tv * dt(f32(Ht))), zero), dt(f32(Ht - 1))).astype(np.int64)
            colour = tex[row, col]
        elif colors is not None:
            c = np.asarray(colors, f32).astype(dt)[tri]  # (n, 3 vertices, 3 channels)
            colour = (w0[:, None] * c[:, 0] + w1[:, None] * c[:, 1] + w2[:, None] * c[:, 2]) * z[:, None]
        else:
            colour = np.broadcast_to(np.asarray(surf_color, f32).astype(dt).reshape(1, 3), (len(ys), 3))
        val = np.minimum(np.maximum(w[:, None] * colour, zero), one) * dt(255.0) + dt(0.5)
        assert val.dtype == dt
        img[ys, xs] = val.astype(np.int32).astype(np.uint8)
    if samples:
        return img
    # area mean, always in float32: PARITY UNPINNED (cv2.resize INTER_AREA for an integer factor, restated)
    sums = img.reshape(H, ssaa, W, ssaa, 3).astype(np.int32).sum(axis=(1, 3))
    mean = sums.astype(f32) * (f32(1.0) / f32(ssaa * ssaa))
    assert mean.dtype == f32
    return np.rint(mean).astype(np.int32).astype(np.uint8)


class NumpyShadedRenderer:
    """`render.HipShadedRenderer`'s interface on `render_shaded`, host arrays in and out."""

    def __init__(self, width, height, ambient=AMBIENT, shading="phong", ssaa=4):
        self.W, self.H, self.ambient, self.shading, self.ssaa, self.models = int(width), int(height), ambient, shading, int(ssaa), {}

    def add_object(self, obj_id, verts, faces, normals=None, colors=None, texture=None, texture_uv=None, surf_color=None):
        self.models[obj_id] = dict(verts=verts, faces=faces, normals=normals, colors=colors, texture=texture, texture_uv=texture_uv,
                                   surf_color=GREY if surf_color is None else tuple(surf_color))

    def render_batch(self, obj_id, Rs, ts, K4, out=None):
        Rs, ts = np.asarray(Rs).reshape(-1, 3, 3), np.asarray(ts).reshape(-1, 3)
        K4 = np.broadcast_to(np.asarray(K4, np.float64).reshape(-1, 4), (len(Rs), 4))
        return np.stack([render_shaded(R=R, t=t, fx=k[0], fy=k[1], cx=k[2], cy=k[3], H=self.H, W=self.W, ambient=self.ambient,
                                       shading=self.shading, ssaa=self.ssaa, **self.models[obj_id]) for R, t, k in zip(Rs, ts, K4)])

    def render_object(self, obj_id, R, t, fx, fy, cx, cy):
        return {"rgb": self.render_batch(obj_id, [R], [t], [fx, fy, cx, cy])[0]}


class NumpyDepthRenderer:
    """`render.HipDepthRenderer`'s interface on `render_depth`."""

    def __init__(self, width, height):
        self.W, self.H, self.models = int(width), int(height), {}

    def add_object(self, obj_id, verts, faces):
        self.models[obj_id] = (verts, faces)

    def render_batch(self, obj_id, Rs, ts, K4, out=None):
        Rs, ts = np.asarray(Rs).reshape(-1, 3, 3), np.asarray(ts).reshape(-1, 3)
        K4 = np.broadcast_to(np.asarray(K4, np.float64).reshape(-1, 4), (len(Rs), 4))
        return np.stack([render_depth(*self.models[obj_id], R, t, *k, self.H, self.W) for R, t, k in zip(Rs, ts, K4)])
