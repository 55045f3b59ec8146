"""Inputs shared by the reference-target tests (tests/test_ref_targets_cpu.py, tests/test_ref_targets_gpu.py): seeded rotations with scenes and
keys, symmetry sets of 1, 2 and 315 rotations, an independent restatement of the selection rule, and the files `tests/bop_synth.py`'s dataset
lacks for the command line (`scene_gt_info.json` from its masks)."""
import functools
import json
import os
import os.path as osp

import numpy as np

from unopose_amd import bop_eval, ref_targets
from unopose_amd.provider import read_image

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15


def rotations(rs, n):
    """n rotations, uniform over SO(3), from unit quaternions."""
    q = rs.randn(n, 4)
    w, x, y, z = (q / np.linalg.norm(q, axis=1, keepdims=True)).T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1).reshape(n, 3, 3)


@functools.lru_cache(maxsize=None)
def symmetries(S):
    """(S, 3, 3): the identity; with the half turn about z; or one continuous z-axis symmetry at the project's discretisation (315)."""
    info = {1: {}, 2: {"symmetries_discrete": [[-1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]]},
            315: {"symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}}[S]
    out = np.stack([s["R"] for s in bop_eval.symmetry_transformations(info)])
    assert out.shape == (S, 3, 3)
    out.setflags(write=False)
    return out


def make_case(seed, Q, C, S, scenes=3):
    """dict(Rq, q_scene, q_key, Rc, c_scene, c_key, syms): every view has a scene of `scenes` and an image number of its own."""
    rs = np.random.RandomState(seed)
    q_scene, c_scene = rs.randint(0, scenes, Q).astype(np.int64), rs.randint(0, scenes, C).astype(np.int64)
    ims = rs.permutation(Q + C)
    key = lambda scene, im: ((scene.astype(np.uint64) << np.uint64(32)) | im.astype(np.uint64))
    return dict(Rq=rotations(rs, Q), q_scene=q_scene, q_key=key(q_scene, ims[:Q]), Rc=rotations(rs, C), c_scene=c_scene, c_key=key(c_scene, ims[Q:]),
                syms=symmetries(S))


def mix64_int(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def priority_int(seed, q_key, c_key):
    return mix64_int(mix64_int(seed + G + int(q_key)) + G + int(c_key))


def plain_best(case):
    """best[q, c] with numpy's own matrix products and np.trace: the arithmetic order is numpy's, so only values away from a threshold compare."""
    T = case["Rc"][:, None] @ case["syms"][None]  # (C, S, 3, 3)
    return np.stack([np.minimum(np.trace(Rq @ np.swapaxes(T, -1, -2), axis1=-2, axis2=-1), 3.0).max(axis=1) for Rq in case["Rq"]])


def plain_select(case, best, trace_min, seed, cross_scene):
    """The rule restated with Python loops and Python integers on a given `best` -> (pick, n_eligible, nearest) lists."""
    picks, counts, nearests = [], [], []
    for q in range(len(case["Rq"])):
        pick, prio, count, nearest = -1, None, 0, -1
        for c in range(len(case["Rc"])):
            if (case["c_scene"][c] == case["q_scene"][q]) if cross_scene else (case["c_key"][c] == case["q_key"][q]):
                continue
            if nearest < 0 or best[q, c] > best[q, nearest]:
                nearest = c
            if best[q, c] >= trace_min:
                count += 1
                p = priority_int(seed, case["q_key"][q], case["c_key"][c])
                if prio is None or p < prio:
                    pick, prio = c, p
        picks.append(pick), counts.append(count), nearests.append(nearest)
    return picks, counts, nearests


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def host(case, max_rot, seed=0, cross_scene=True):
    return ref_targets.select_host(case["Rq"], case["q_scene"], case["q_key"], case["Rc"], case["c_scene"], case["c_key"], case["syms"],
                                   ref_targets.trace_min_of(max_rot), seed, cross_scene)


def write_gt_info(root, dataset="ycbv"):
    """`scene_gt_info.json` for every scene of the synthetic dataset: each ground truth fully visible, its pixel count from its mask."""
    for split in ("test", "train_real"):
        base = osp.join(root, dataset, split)
        for scene in sorted(os.listdir(base)) if osp.isdir(base) else ():
            gt = json.load(open(osp.join(base, scene, "scene_gt.json")))
            info = {}
            for im, gts in gt.items():
                px = [int((read_image(osp.join(base, scene, "mask_visib", f"{int(im):06d}_{j:06d}.png")) > 0).sum()) for j in range(len(gts))]
                info[im] = [dict(px_count_all=n, px_count_valid=n, px_count_visib=n, visib_fract=1.0, bbox_obj=[0, 0, 1, 1], bbox_visib=[0, 0, 1, 1]) for n in px]
            json.dump(info, open(osp.join(base, scene, "scene_gt_info.json"), "w"))
