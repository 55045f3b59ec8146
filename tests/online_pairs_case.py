"""Hand-made canvases for the online training pairs (tests/test_online_pairs_cpu.py, tests/test_online_pairs_gpu.py): a chunk of
(query, reference) pairs, one per case the item rule has to get right, with the recipe that goes with them.  Built once."""
import functools

import numpy as np

H, W = 56, 72  # W is no multiple of 64: a row spans two wavefront steps
S, N_OBS, N_TPL = 28, 64, 96
CFG = dict(img_size=S, n_sample_observed_point=N_OBS, n_sample_template_point=N_TPL, min_px_count_visib=20, min_visib_fract=0.3, dilate_mask=True,
           rgb_mask_flag=True, shift_range=0.01, batch_size=4,
           online=dict(canvas=(H, W), focal=80.0, fill=(0.45, 0.8), offset=0.3, occluder_prob=0.5, ssaa=1, shading="phong", ambient=0.5, max_chunks=8))
MODELS = {1: dict(diameter=100.0, centre=np.zeros(3)), 2: dict(diameter=60.0, centre=np.array([1.0, -2.0, 0.5]))}

YY, XX = np.mgrid[0:H, 0:W]


def ellipse(cy, cx, ry, rx):
    return ((YY - cy) / ry) ** 2 + ((XX - cx) / rx) ** 2 <= 1.0


def box(y0, y1, x0, x1):
    return (YY >= y0) & (YY < y1) & (XX >= x0) & (XX < x1)


def plane(mask, z0, gx=0.0, gy=0.0):
    """A tilted plane of depth (model units) where the mask is set, 0 elsewhere."""
    return np.where(mask, z0 + gx * XX + gy * YY, 0.0).astype(np.float32)


BIG_REF = plane(ellipse(28, 36, 21, 25), 400.0, 0.5, 0.3)  # a reference whose radius admits everything near 400

# name -> (reference depth, query object depth, occluder depth or None, dilation coin)
CASES = {
    "plain": (BIG_REF, plane(ellipse(27, 35, 16, 19), 410.0, 0.4, -0.2), None, False),
    "top_left_odd": (plane(box(0, 23, 0, 31), 400.0, 0.3), plane(box(0, 25, 0, 17), 405.0, 0.1, 0.2), None, False),
    "bottom_right": (plane(ellipse(50, 66, 14, 11), 400.0), plane(ellipse(49, 63, 12, 15), 395.0, 0.2), None, False),
    "tall_full_height": (plane(box(0, H, 30, 41), 400.0), plane(box(0, H, 3, 20), 400.0, 0.0, 0.1), None, False),
    "fewer_than_wanted": (plane(box(20, 28, 30, 40), 400.0), plane(box(22, 28, 31, 38), 400.0), None, False),  # 80 and 42 set pixels
    "exactly_as_many": (plane(box(20, 28, 30, 42), 400.0), plane(box(20, 28, 31, 39), 400.0), None, False),  # 96 and 64: with replacement
    "kept_31": (BIG_REF, np.maximum(plane(box(24, 28, 30, 38) & ~box(24, 25, 30, 31), 400.0), plane(box(24, 25, 40, 42), 1000.0)), None, False),
    "kept_32": (BIG_REF, np.maximum(plane(box(24, 28, 30, 38), 400.0), plane(box(24, 25, 40, 42), 1000.0)), None, False),
    "occluder_all": (BIG_REF, plane(ellipse(27, 35, 12, 14), 410.0), plane(box(5, 50, 10, 60), 200.0), False),
    "occluder_part": (BIG_REF, plane(ellipse(27, 35, 16, 19), 410.0, 0.4), np.maximum(plane(box(0, H, 0, 30), 250.0), plane(box(0, 24, 30, W), 900.0)), False),
    "object_outside": (BIG_REF, plane(box(0, 0, 0, 0), 1.0), None, False),
    "reference_outside": (plane(box(0, 0, 0, 0), 1.0), plane(ellipse(27, 35, 16, 19), 410.0), None, False),
    "dilate_edge_occluder": (BIG_REF, plane(ellipse(27, 58, 21, 17), 410.0, 0.2), plane(box(10, 40, 20, 44), 300.0), True),
    "dilate_plain": (BIG_REF, plane(ellipse(27, 35, 20, 24), 410.0), None, True),
}
NAMES = tuple(CASES)
VALID = {"plain", "top_left_odd", "bottom_right", "tall_full_height", "fewer_than_wanted", "exactly_as_many", "kept_32", "occluder_part",
         "dilate_edge_occluder", "dilate_plain"}


@functools.lru_cache(maxsize=None)
def chunk():
    """-> (views, recipe): every case as one candidate of one chunk; colours are noise, the coins are the cases'."""
    from unopose_amd.provider_online import draw_recipe

    C = len(NAMES)
    rs = np.random.RandomState(11)
    views = {k: rs.randint(1, 256, size=(C, H, W, 3)).astype(np.uint8) for k in ("ref_rgb", "q_rgb", "occ_rgb")}
    views.update({k: np.zeros((C, H, W), np.float32) for k in ("ref_depth", "q_depth", "occ_depth")})
    recipe = draw_recipe(7, 0, 3, C, MODELS, CFG)
    for k, name in enumerate(NAMES):
        ref, query, occ, coin = CASES[name]
        views["ref_depth"][k], views["q_depth"][k] = ref, query
        recipe["occ"][k], recipe["dilate"][k] = occ is not None, coin
        if occ is not None:
            views["occ_depth"][k] = occ
    for v in views.values():
        v.setflags(write=False)
    return views, recipe


@functools.lru_cache(maxsize=None)
def mirror():
    """`items_from_views_host` on the chunk -> (items, intermediates).  Shared: do not change."""
    from unopose_amd.provider_online import items_from_views_host

    return items_from_views_host(*chunk(), CFG, with_intermediates=True)
