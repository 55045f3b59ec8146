"""The scene stage on the hand-made chunk of online_pairs_case (tests/test_online_scene_cpu.py, tests/test_online_scene_gpu.py): the
configuration, the scene draw with the planes the tests set by hand, and the host rule's results.  Built once."""
import functools

import numpy as np

import online_pairs_case as case

CFG = dict(case.CFG, online=dict(case.CFG["online"], scene={}))  # the stage at its defaults
QUIET = dict(background="plane", noise=(0.0, 0.0, 0.0), disparity_steps=0, edge_drop=0.0, hole_prob=0.0)  # the plane alone
CFG_QUIET = dict(case.CFG, online=dict(case.CFG["online"], scene=QUIET))
PLANE_BEHIND = 40.0  # model units between the farthest visible object pixel and the fronto-parallel plane of the two dilated cases
STEEP = "plain"  # its plane is tilted 80 degrees about the image's y axis: it faces away from the rays right of column 50
NO_PLANE = "object_outside"  # an all-zero query without a plane


def visible_object(name):
    """(visible mask, object depth) of a hand case's query."""
    k = case.NAMES.index(name)
    views, _ = case.chunk()
    qd, cd = views["q_depth"][k], views["occ_depth"][k]
    return (qd > 0) & ((cd == 0) | (qd <= cd)), qd


@functools.lru_cache(maxsize=None)
def scene():
    """`draw_scene` for the hand chunk with the planes of four cases overwritten (as the chunk overwrites the recipe's coins)."""
    from unopose_amd.provider_online import draw_scene

    _, recipe = case.chunk()
    sc = draw_scene(7, 0, 3, len(case.NAMES), recipe, case.MODELS, CFG)
    for name in ("dilate_plain", "dilate_edge_occluder"):
        k = case.NAMES.index(name)
        vis, qd = visible_object(name)
        sc["n"][k], sc["p0"][k] = (0.0, 0.0, -1.0), (0.0, 0.0, float(qd[vis].max()) + PLANE_BEHIND)
        sc["u"][k], sc["v"][k] = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)
    k = case.NAMES.index(STEEP)
    tilt = np.deg2rad(80.0)
    sc["n"][k], sc["p0"][k] = (np.sin(tilt), 0.0, -np.cos(tilt)), (0.0, 0.0, 500.0)
    sc["u"][k], sc["v"][k] = (np.cos(tilt), 0.0, np.sin(tilt)), (0.0, 1.0, 0.0)
    sc["plane"][case.NAMES.index(NO_PLANE)] = False
    for v in sc.values():
        v.setflags(write=False)
    return sc


@functools.lru_cache(maxsize=None)
def mirror(quiet=False):
    """`items_from_views_host` on the chunk with the scene -> (items, intermediates).  Shared: do not change."""
    from unopose_amd.provider_online import items_from_views_host

    return items_from_views_host(*case.chunk(), CFG_QUIET if quiet else CFG, with_intermediates=True, scene=scene())


@functools.lru_cache(maxsize=None)
def canvases():
    """The 28 views the stage sees in the hand chunk -> (depth (28, H, W), rgb (28, H, W, 3), descriptors (28, words)): the 14 composed queries
    (scene depth and colour of the item rule WITHOUT the stage), then the 14 references."""
    from unopose_amd.provider_online import online_cfg, scene_rows

    views, _ = case.chunk()
    _, info = case.mirror()
    oc = online_cfg(CFG)
    depth = np.concatenate([np.stack([i["scene_depth"] for i in info]), views["ref_depth"]])
    rgb = np.concatenate([np.stack([i["scene_rgb"] for i in info]), views["ref_rgb"]])
    desc = np.concatenate([scene_rows(scene(), oc, "query"), scene_rows(scene(), oc, "reference")])
    for a in (depth, rgb, desc):
        a.setflags(write=False)
    return depth, rgb, desc


@functools.lru_cache(maxsize=None)
def sensed():
    """`sense_views_host` on `canvases()` -> (depth, rgb, intermediates).  Shared: do not change."""
    from unopose_amd.provider_online import sense_views_host

    return sense_views_host(*canvases(), with_intermediates=True)
