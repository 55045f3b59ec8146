"""Models, views and a dataset folder for the training-view renderer (unopose_amd/render_train.py, render.HipShadedRenderer,
csrc/raster_shade.hip), shared by tests/test_render_train_cpu.py and tests/test_render_train_gpu.py."""
import functools
import json
import os
import os.path as osp

import numpy as np

from gt_info_case import make_models

CAMERA = dict(fx=44.0, fy=45.1, cx=19.3, cy=15.6, depth_scale=0.1, width=40, height=32)
SIZES = ((40, 32), (37, 29))
SURF = (0.95, 0.35, 0.1)


def write_model_ply(path, verts, faces, normals=None, colors=None, uv=None, texture_file=None, binary=True, face_texcoord=False):
    """A PLY as BOP's `models/` files are laid out: float x, y, z [nx, ny, nz] [texture_u, texture_v] [uchar red, green, blue], triangular
    faces, the texture named by a comment.  `colors` are bytes.  `face_texcoord`: the faces carry a `texcoord` list of six floats as well."""
    verts, faces = np.asarray(verts, np.float64), np.asarray(faces, np.int32)
    cols = [("x", "<f4", verts[:, 0]), ("y", "<f4", verts[:, 1]), ("z", "<f4", verts[:, 2])]
    if normals is not None:
        cols += [(k, "<f4", np.asarray(normals)[:, i]) for i, k in enumerate(("nx", "ny", "nz"))]
    if uv is not None:
        cols += [(k, "<f4", np.asarray(uv)[:, i]) for i, k in enumerate(("texture_u", "texture_v"))]
    if colors is not None:
        cols += [(k, "u1", np.asarray(colors)[:, i]) for i, k in enumerate(("red", "green", "blue"))]
    head = ["ply", "format %s 1.0" % ("binary_little_endian" if binary else "ascii"), "comment written by tests/render_train_case.py"]
    if texture_file is not None:
        head.append("comment TextureFile " + texture_file)
    head.append("element vertex %d" % len(verts))
    head += ["property %s %s" % ("uchar" if t == "u1" else "float", k) for k, t, _ in cols]
    head += ["element face %d" % len(faces), "property list uchar int vertex_indices"]
    if face_texcoord:
        head.append("property list uchar float texcoord")
    head.append("end_header")
    os.makedirs(osp.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        if binary:
            rec = np.zeros(len(verts), dtype=[(k, t) for k, t, _ in cols])
            for k, _, a in cols:
                rec[k] = a
            f.write(rec.tobytes())
            frec = np.zeros(len(faces), dtype=[("n", "u1"), ("v", "<i4", (3,))] + ([("m", "u1"), ("t", "<f4", (6,))] if face_texcoord else []))
            frec["n"], frec["v"] = 3, faces
            if face_texcoord:
                frec["m"] = 6
            f.write(frec.tobytes())
        else:
            for i in range(len(verts)):
                f.write((" ".join(str(int(a[i])) if t == "u1" else repr(float(np.float32(a[i]))) for _, t, a in cols) + "\n").encode("ascii"))
            for tri in faces:
                f.write(("3 %d %d %d" % tuple(tri) + (" 6 0 0 1 0 0 1" if face_texcoord else "") + "\n").encode("ascii"))


def sphere_uv(verts):
    """Longitude / latitude texture coordinates in [0, 1]."""
    d = verts / np.linalg.norm(verts, axis=1, keepdims=True)
    return np.stack([np.arctan2(d[:, 1], d[:, 0]) / (2 * np.pi) + 0.5, np.arcsin(np.clip(d[:, 2], -1, 1)) / np.pi + 0.5], axis=1)


def texture_image(h=5, w=7, seed=4):
    """A small bright texture of odd size: every texel another colour."""
    return np.random.RandomState(seed).randint(60, 256, size=(h, w, 3)).astype(np.uint8)


def analytic_normals(verts, axes):
    """Normals of the ellipsoid x^2/a^2 + y^2/b^2 + z^2/c^2 = 1 at its points: the gradient."""
    n = verts / np.asarray(axes, np.float64) ** 2
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def write_dataset(root, name="synth"):
    """<root>/<name>: camera.json (40 x 32) and models/ with object 1 -- binary, normals, texture coordinates, a texture image -- and object
    2 -- ASCII, vertex colours, NO normals.  -> the dataset folder."""
    from PIL import Image

    base, models = osp.join(root, name), make_models()
    os.makedirs(osp.join(base, "models"), exist_ok=True)
    json.dump(CAMERA, open(osp.join(base, "camera.json"), "w"))
    v1, v2 = models[1]["verts"], models[2]["verts"]
    Image.fromarray(texture_image()).save(osp.join(base, "models", "obj_000001.png"))
    write_model_ply(osp.join(base, "models", "obj_000001.ply"), v1, models[1]["faces"], normals=analytic_normals(v1, (100.0, 90.0, 80.0)), uv=sphere_uv(v1),
                    texture_file="obj_000001.png", binary=True)
    cols = np.random.RandomState(9).randint(30, 256, size=(len(v2), 3))
    write_model_ply(osp.join(base, "models", "obj_000002.ply"), v2, models[2]["faces"], colors=cols, binary=False)
    return base


RENDER_ARGS = ["--radii", "420", "--min-views", "12", "--ssaa", "2"]


@functools.lru_cache(maxsize=None)
def tricky_model():
    """The 80-face ellipsoid of gt_info_case with everything the kernel has a rule for:
    * face 0 repeats a vertex (degenerate), face 1 is a sliver of zero area in front of the object;
    * face 2 lies behind the camera in view 0 (it is dropped there: no clipping);
    * the last two faces are the ellipsoid's faces 10 and 11 again on vertices of their own -- coplanar, equal depth at every sample, other
      colours and texture coordinates: the original, of the lower index, must win;
    * vertex 3 has a zero-length normal, vertex 4 one of length 7;
    * texture coordinates exactly 0 and exactly 1 (vertices 6, 7) and slightly outside [0, 1] (vertices 8, 9).
    -> dict(verts, faces, normals, colors, texture_uv, texture)."""
    m = make_models()[1]
    base, f = m["verts"], m["faces"]
    n = len(base)
    extra = np.array([[0.0, 0.0, -150.0], [10.0, 0.0, -150.0], [20.0, 0.0, -150.0], [-30.0, -20.0, -900.0], [30.0, -20.0, -900.0], [0.0, 30.0, -900.0]])
    again = base[f[[10, 11]].reshape(-1)]  # six vertices of their own
    verts = np.concatenate([base, extra, again])
    faces = np.concatenate([[[0, 0, 5], [n, n + 1, n + 2], [n + 3, n + 4, n + 5]], f, np.arange(n + 6, n + 12).reshape(2, 3)]).astype(np.int32)
    normals = np.concatenate([analytic_normals(base, (100.0, 90.0, 80.0)), np.tile([0.0, 0.0, -1.0], (6, 1)), analytic_normals(again, (100.0, 90.0, 80.0))])
    normals[3] = 0.0
    normals[4] *= 7.0
    rs = np.random.RandomState(12)
    colors = rs.uniform(0.15, 1.0, size=(len(verts), 3))
    colors[n + 6:] = [0.0, 0.0, 1.0]
    uv = np.concatenate([sphere_uv(base), np.tile([0.5, 0.5], (6, 1)), np.tile([0.1, 0.1], (6, 1))])
    uv[6], uv[7], uv[8], uv[9] = [0.0, 1.0], [1.0, 0.0], [-0.01, 1.02], [1.02, -0.01]
    return dict(verts=verts, faces=faces, normals=normals, colors=colors, texture_uv=uv, texture=texture_image())


def colour_kwargs(colour):
    """`add_object` arguments of the tricky model coloured by "texture", "colors" or "surf"."""
    m = tricky_model()
    kw = dict(verts=m["verts"], faces=m["faces"], normals=m["normals"])
    if colour == "texture":
        kw.update(texture=m["texture"], texture_uv=m["texture_uv"])
    elif colour == "colors":
        kw["colors"] = m["colors"]
    else:
        kw["surf_color"] = SURF
    return kw


@functools.lru_cache(maxsize=None)
def views(W, H):
    """Three views for a W x H image -> k4, Rs (3,3,3), ts (3,3): the object in the middle seen along its z axis (the far triangle behind
    the camera), turned about two axes, and pushed over the left and upper border."""
    f = 44.0 * W / 40.0
    k4 = [f, f * 1.025, (W - 1) / 2.0 - 0.2, (H - 1) / 2.0 + 0.1]

    def rot(ax, ay):
        cx_, sx_, cy_, sy_ = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay)
        return np.array([[1, 0, 0], [0, cx_, -sx_], [0, sx_, cx_]]) @ np.array([[cy_, 0, sy_], [0, 1, 0], [-sy_, 0, cy_]])

    Rs = np.stack([np.eye(3), rot(0.7, 2.4), rot(-0.4, 0.9)])
    ts = np.array([[3.0, -2.0, 420.0], [-8.0, 5.0, 380.0], [-160.0, -120.0, 400.0]])
    return k4, Rs, ts
