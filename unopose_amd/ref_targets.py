"""The one-reference target list of a BOP split: for every test target (scene, image, object) the reference view (ref_scene, ref_image) whose
crop and cloud form the pair's other half -- the file `BOPTestsetOneRef.load_ref` reads (`cfg.ref_targets_name`, in the reference's
configuration `test_ref_targets_crossscene_rot50.json`).

The reference provides that file for YCB-V and publishes no generator, so THE RULE BELOW IS THIS PROJECT'S OWN STATEMENT of what the file's name
says -- a view of the same object from another scene, within 50 degrees of the target's rotation up to the object's symmetries -- and not the
authors' procedure; `--check` audits any list, the published one included, against it.

For one object, with queries (R_q, scene, key), candidate views (R_c, scene, key) and the rotation parts S_s of
`bop_eval.symmetry_transformations` (a key is scene_identity << 32 | im_id; a scene identity stands for a (split folder, scene id) pair and is a function of that pair alone:
the scene id in the split's own folder, 2^24 + scene id under train_real):
    T[c,s]    = R_c S_s, each element by `bop_eval._dot3`                         (as `re_sym` forms R_gt S)
    tr[q,c,s] = min((d0 + d1) + d2, 3.0), d_r = _dot3 over row r of R_q and T     (`_rotation_degrees`' trace)
    best[q,c] = max over s of tr[q,c,s]
    allowed   : c_scene != q_scene (cross-scene), or c_key != q_key (same-scene: only the view itself is excluded)
    eligible  : allowed and best[q,c] >= trace_min, trace_min = 1 + 2 cos(radians(max_rot)) computed once and handed to both routes as a number
                -- a comparison of traces; no arccos is on either side of the threshold
    pick      : the eligible candidate with the smallest priority = mix64(mix64(seed + G + q_key) + G + c_key) in uint64 wrap-around
                arithmetic (splitmix64's finaliser and increment); equal priorities go to the lower candidate index; -1 without one
    nearest   : the allowed candidate with the largest best, the lower index among equals; -1 if nothing is allowed (its trace is -inf then)
The pick is random and keyed: a nearest-view rule would make the benchmark easy, and a keyed one depends neither on the file order nor on how
the work is split, and stays put when a scene is added elsewhere.

`select_host` is that rule in float64 numpy; `ops.ref_select` (csrc/reftargets.hip) gives the same four outputs with equal bits.
`build_ref_targets` applies it to a dataset, `check_ref_targets` audits an existing list, `python -m unopose_amd.ref_targets` is the command line."""
import argparse
import json
import math
import os
import os.path as osp
import sys

import numpy as np

GOLDEN = 0x9E3779B97F4A7C15
HOST_BLOCK = 1 << 19  # (query, candidate, symmetry) triples the host route forms at a time
ENTRY_KEYS = ("scene_id", "im_id", "obj_id", "ref_scene_id", "ref_im_id")  # exactly what `load_ref` reads
SCENE_IDS = 1 << 24     # scene ids per split folder: a scene identity is scene_id, or 2^24 + scene_id for a train_real scene
ENTRY_LIMIT = 1e100     # |matrix entry| up to which no product of the three matrices can overflow
_U = np.uint64


def mix64(z):
    """splitmix64's finaliser on uint64 (arrays or numbers), wrap-around arithmetic -> uint64 array of the same shape."""
    z = np.asarray(z, dtype=_U)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U(27))) * _U(0x94D049BB133111EB)
        return z ^ (z >> _U(31))


def priority(seed, q_key, c_key):
    """mix64(mix64(seed + G + q_key) + G + c_key), broadcasting over q_key and c_key -> uint64 array."""
    with np.errstate(over="ignore"):
        half = mix64(np.asarray(seed, _U) + _U(GOLDEN) + np.asarray(q_key, _U))
        return mix64(half + _U(GOLDEN) + np.asarray(c_key, _U))


def trace_min_of(max_rot):
    """The smallest trace of a rotation by at most `max_rot` degrees: 1 + 2 cos(radians(max_rot))."""
    return 1.0 + 2.0 * math.cos(math.radians(float(max_rot)))


def _rotations(R, name):
    R = np.ascontiguousarray(np.asarray(R, dtype=np.float64).reshape(-1, 3, 3))
    if not (np.abs(R) <= ENTRY_LIMIT).all():  # False for NaN too
        raise ValueError(f"ref_targets: {name} holds an entry that is not finite or beyond {ENTRY_LIMIT:g}")
    return R


def check_inputs(Rq, q_scene, q_key, Rc, c_scene, c_key, syms, trace_min, seed=0):
    """The checks both routes make before any work, in one place -> (Rq (Q,3,3), q_scene int64, q_key uint64, Rc (C,3,3), c_scene, c_key,
    syms (S,3,3), trace_min float, seed int), contiguous: finite entries of magnitude <= 1e100, S >= 1, lengths that agree, a trace_min that is
    a number, a seed in 0 .. 2^64 - 1."""
    Rq, Rc, syms = _rotations(Rq, "Rq"), _rotations(Rc, "Rc"), _rotations(syms, "syms")
    q_scene, c_scene = np.ascontiguousarray(q_scene, np.int64).reshape(-1), np.ascontiguousarray(c_scene, np.int64).reshape(-1)
    q_key, c_key = np.ascontiguousarray(q_key, _U).reshape(-1), np.ascontiguousarray(c_key, _U).reshape(-1)
    if len(syms) < 1:
        raise ValueError("ref_targets: no symmetries (the identity is one)")
    if not (len(q_scene) == len(q_key) == len(Rq) and len(c_scene) == len(c_key) == len(Rc)):
        raise ValueError(f"ref_targets: {len(Rq)} / {len(q_scene)} / {len(q_key)} queries and {len(Rc)} / {len(c_scene)} / {len(c_key)} candidates (R / scene / key)")
    trace_min, seed = float(trace_min), int(seed)
    if math.isnan(trace_min) or not 0 <= seed < 1 << 64:
        raise ValueError(f"ref_targets: trace_min {trace_min}, seed {seed} (a number; 0 .. 2^64 - 1)")
    return Rq, q_scene, q_key, Rc, c_scene, c_key, syms, trace_min, seed


def compose(Rc, syms):
    """T[c,s] = R_c S_s (C, S, 3, 3), each element by `bop_eval._dot3`."""
    from .bop_eval import _dot3

    A, B = Rc[:, None], syms[None]
    return np.stack([np.stack([_dot3(A[..., r, 0], B[..., 0, k], A[..., r, 1], B[..., 1, k], A[..., r, 2], B[..., 2, k]) for k in range(3)], axis=-1)
                     for r in range(3)], axis=-2)


def best_traces(Rq, Rc, syms, block=HOST_BLOCK):
    """best[q,c] = max over s of min(trace(R_q T[c,s]^T), 3) in the module docstring's order of arithmetic -> (Q, C) float64."""
    from .bop_eval import _dot3

    Rq, Rc, syms = _rotations(Rq, "Rq"), _rotations(Rc, "Rc"), _rotations(syms, "syms")
    Q, C, S = len(Rq), len(Rc), len(syms)
    best = np.empty((Q, C), dtype=np.float64)
    rows = max(1, int(block) // max(1, Q * S))
    for a in range(0, C, rows):
        T = compose(Rc[a:a + rows], syms)[None]  # (1, c, S, 3, 3)
        A = Rq[:, None, None]
        d = [_dot3(A[..., r, 0], T[..., r, 0], A[..., r, 1], T[..., r, 1], A[..., r, 2], T[..., r, 2]) for r in range(3)]
        best[:, a:a + rows] = np.minimum((d[0] + d[1]) + d[2], 3.0).max(axis=2)
    return best


def select_host(Rq, q_scene, q_key, Rc, c_scene, c_key, syms, trace_min, seed=0, cross_scene=True, block=HOST_BLOCK):
    """The rule of the module docstring for one object -> (pick (Q,) int64, n_eligible (Q,) int64, nearest (Q,) int64, nearest_trace (Q,) float64).
    Q or C of zero gives empty or all -1 results."""
    Rq, q_scene, q_key, Rc, c_scene, c_key, syms, trace_min, seed = check_inputs(Rq, q_scene, q_key, Rc, c_scene, c_key, syms, trace_min, seed)
    Q, C = len(Rq), len(Rc)
    pick, nearest = np.full(Q, -1, np.int64), np.full(Q, -1, np.int64)
    count, nearest_trace = np.zeros(Q, np.int64), np.full(Q, -np.inf)
    if Q == 0 or C == 0:
        return pick, count, nearest, nearest_trace
    best = best_traces(Rq, Rc, syms, block)
    allowed = (c_scene[None] != q_scene[:, None]) if cross_scene else (c_key[None] != q_key[:, None])
    eligible = allowed & (best >= trace_min)
    prio = priority(seed, q_key[:, None], c_key[None])
    count[:] = eligible.sum(axis=1)
    for q in range(Q):
        idx = np.flatnonzero(eligible[q])
        if len(idx):
            pick[q] = idx[np.argmin(prio[q, idx])]  # the first of equal priorities: the lower index
        idx = np.flatnonzero(allowed[q])
        if len(idx):
            nearest[q] = idx[np.argmax(best[q, idx])]
            nearest_trace[q] = best[q, nearest[q]] + 0.0  # a trace of -0.0 leaves as +0.0 on both routes
    return pick, count, nearest, nearest_trace


def select(Rq, q_scene, q_key, Rc, c_scene, c_key, syms, trace_min, seed=0, cross_scene=True, device=None):
    """`select_host` without a device, `ops.ref_select` on a CUDA `device`: equal bits."""
    if device is None:
        return select_host(Rq, q_scene, q_key, Rc, c_scene, c_key, syms, trace_min, seed, cross_scene)
    from .bop_eval import _cuda_device
    from .ops.score import ref_select

    return ref_select(Rq, q_scene, q_key, Rc, c_scene, c_key, syms, trace_min, seed, cross_scene, _cuda_device(device))


# ------------------------------------------------------------------------------------------------
# the dataset side
# ------------------------------------------------------------------------------------------------
def default_name(max_rot, cross_scene):
    return f"test_ref_targets_{'crossscene' if cross_scene else 'samescene'}_rot{max_rot:g}.json"


def _scene_ids(folder):
    if not osp.isdir(folder):
        return []
    return sorted(int(d) for d in os.listdir(folder) if d.isdigit() and osp.exists(osp.join(folder, d, "scene_gt.json")))


class _Dataset:
    """The scene files of one dataset, read once, and the identity of its (split folder, scene id) pairs."""

    def __init__(self, data_dir, dataset, split):
        self.data_dir, self.dataset, self.split = data_dir, dataset, split
        self.test_folder = osp.join(data_dir, dataset, split)
        self._json = {}

    def ref_folder(self, scene_id):
        from .provider import ref_split_folder

        return ref_split_folder(self.data_dir, self.dataset, scene_id, self.test_folder)

    def identity(self, folder, scene_id):
        """The scene identity of (split folder, scene id): the scene id, plus 2^24 outside the split's own folder (train_real).  It depends on
        the scene alone -- not on which targets are listed, their order, or which other scenes exist -- because it is hashed into every
        priority."""
        scene_id = int(scene_id)
        if not 0 <= scene_id < SCENE_IDS:
            raise ValueError(f"ref_targets: scene id {scene_id} (0 .. 2^24 - 1)")
        return scene_id if osp.normpath(folder) == osp.normpath(self.test_folder) else SCENE_IDS + scene_id

    def scene_json(self, folder, scene_id, name):
        from .provider import load_json

        key = (folder, scene_id, name)
        if key not in self._json:
            path = osp.join(folder, f"{scene_id:06d}", name)
            if not osp.exists(path):
                hint = ": write it with `python -m unopose_amd.gt_info`" if name == "scene_gt_info.json" else ""
                raise FileNotFoundError(f"ref_targets: {path} is missing{hint}")
            self._json[key] = {int(k): v for k, v in load_json(path).items()}
        return self._json[key]

    def first_instance(self, folder, scene_id, im_id, obj_id):
        """(slot, rotation, instances) of the object's first ground truth in the image in `scene_gt` order -- the one `ReferenceViews._build`
        takes -- or None when the scene, the image or the object does not exist."""
        if not osp.exists(osp.join(folder, f"{scene_id:06d}", "scene_gt.json")):
            return None
        gts = self.scene_json(folder, scene_id, "scene_gt.json").get(int(im_id))
        slots = [i for i, g in enumerate(gts or []) if int(g["obj_id"]) == int(obj_id)]
        if not slots:
            return None
        return slots[0], np.asarray(gts[slots[0]]["cam_R_m2c"], np.float64).reshape(3, 3), len(slots)

    def candidate_scenes(self):
        """[(folder, scene_id)] of every scene the provider would load as a reference: found under the split or under train_real, and
        `provider.ref_split_folder` resolves its id to the folder it was found in."""
        folders = [self.test_folder]
        train_real = osp.join(self.data_dir, self.dataset, "train_real")
        if osp.normpath(train_real) != osp.normpath(self.test_folder):
            folders.append(train_real)
        return [(f, sid) for f in folders for sid in _scene_ids(f) if osp.normpath(self.ref_folder(sid)) == osp.normpath(f)]

    def visibility(self, folder, scene_id, im_id, slot):
        """(visib_fract, px_count_visib) of a ground truth from `scene_gt_info.json`; the scene's `mask_visib/` has to exist too."""
        if not osp.isdir(osp.join(folder, f"{scene_id:06d}", "mask_visib")):
            raise FileNotFoundError(f"ref_targets: {osp.join(folder, f'{scene_id:06d}', 'mask_visib')} is missing: write it with `python -m unopose_amd.gt_info`")
        info = self.scene_json(folder, scene_id, "scene_gt_info.json")[int(im_id)][slot]
        return float(info["visib_fract"]), int(info["px_count_visib"])

    def symmetries(self):
        """obj_id -> (S, 3, 3) rotation parts of `bop_eval.symmetry_transformations`, from models_eval/ or models/ models_info.json; the
        identity alone for an object without an entry (and for every object when the dataset has no such file: the caller says so)."""
        from .bop_eval import symmetry_transformations
        from .provider import load_json

        path = next((p for p in (osp.join(self.data_dir, self.dataset, m, "models_info.json") for m in ("models_eval", "models")) if osp.exists(p)), None)
        info = load_json(path) if path else {}
        return path, lambda obj_id: np.stack([np.asarray(s["R"], np.float64).reshape(3, 3) for s in symmetry_transformations(info.get(str(obj_id), {}))])


def _key(identity, im_id):
    return (int(identity) << 32) | int(im_id)


def _queries(ds, targets_path, all_images):
    """[(scene_id, im_id, obj_id)] in list order (or scene, image, `scene_gt` order with `all_images`), duplicates dropped."""
    from .provider import load_json

    if all_images:
        rows = [(sid, iid, int(g["obj_id"])) for sid in _scene_ids(ds.test_folder)
                for iid, gts in sorted(ds.scene_json(ds.test_folder, sid, "scene_gt.json").items()) for g in gts]
    else:
        if not osp.exists(targets_path):
            raise FileNotFoundError(f"ref_targets: {targets_path} is missing (--targets names the file, --all-images takes every image of the split)")
        rows = [(int(t["scene_id"]), int(t["im_id"]), int(t["obj_id"])) for t in load_json(targets_path)]
    return list(dict.fromkeys(rows))


def _pool(ds, min_visib):
    """obj_id -> [(folder, scene_id, im_id, rotation, visib_fract)] of the candidate views, in folder, scene, image order."""
    pool = {}
    for folder, sid in ds.candidate_scenes():
        for iid, gts in sorted(ds.scene_json(folder, sid, "scene_gt.json").items()):
            for obj_id in dict.fromkeys(int(g["obj_id"]) for g in gts):
                slot, R, _ = ds.first_instance(folder, sid, iid, obj_id)
                visib, px = ds.visibility(folder, sid, iid, slot)
                if visib >= min_visib and px > 0:
                    pool.setdefault(obj_id, []).append((folder, sid, iid, R, visib))
    return pool


def build_ref_targets(data_dir, dataset, split="test", targets="test_targets_bop19.json", all_images=False, max_rot=50.0, min_visib=0.8,
                      cross_scene=True, seed=0, fallback="nearest", device="cuda", out=None):
    """The list for the dataset's split -> (entries in query order, per-object statistics, number of keys whose object occurs several times,
    the queries [(scene_id, im_id, obj_id)]).
    device=None: the host rule; a CUDA device: `ops.ref_select` per object (equal bits).  fallback: "nearest" gives a target without an
    eligible view its nearest allowed one, "skip" leaves it out (the provider drops such detections)."""
    from .bop_eval import re_sym

    if fallback not in ("nearest", "skip"):
        raise ValueError(f"ref_targets: fallback {fallback!r} (nearest or skip)")
    out = sys.stdout if out is None else out
    ds = _Dataset(data_dir, dataset, split)
    queries = _queries(ds, osp.join(data_dir, dataset, targets), all_images)
    pool = _pool(ds, min_visib)
    sym_path, syms_of = ds.symmetries()
    if sym_path is None:
        print(f"no models_info.json under {osp.join(data_dir, dataset)}: every object is taken as asymmetric", file=out)
    trace_min = trace_min_of(max_rot)
    by_obj, repeated = {}, 0
    for n, (sid, iid, obj_id) in enumerate(queries):
        found = ds.first_instance(ds.test_folder, sid, iid, obj_id)
        if found is None:
            raise ValueError(f"ref_targets: target scene {sid} image {iid} object {obj_id} is not in {ds.test_folder}'s scene_gt.json")
        repeated += found[2] > 1
        by_obj.setdefault(obj_id, []).append((n, sid, iid, found[1]))
    chosen, stats = {}, {}
    for obj_id in sorted(by_obj):
        rows, cands, syms = by_obj[obj_id], pool.get(obj_id, []), syms_of(obj_id)
        q_scene = np.array([ds.identity(ds.test_folder, r[1]) for r in rows], np.int64)
        c_scene = np.array([ds.identity(c[0], c[1]) for c in cands], np.int64)
        q_key = np.array([_key(s, r[2]) for s, r in zip(q_scene, rows)], _U)
        c_key = np.array([_key(s, c[2]) for s, c in zip(c_scene, cands)], _U)
        Rq, Rc = np.stack([r[3] for r in rows]), np.stack([c[3] for c in cands]) if cands else np.zeros((0, 3, 3))
        pick, count, nearest, _ = select(Rq, q_scene, q_key, Rc, c_scene, c_key, syms, trace_min, seed, cross_scene, device)
        use = np.where(pick >= 0, pick, nearest if fallback == "nearest" else -1)
        sym_list, angle = [dict(R=S) for S in syms], 0.0
        for (n, sid, iid, R), c in zip(rows, use):
            if c >= 0:
                chosen[n] = (cands[c][1], cands[c][2])
                angle = max(angle, re_sym(R, cands[c][3], sym_list))
        stats[obj_id] = dict(targets=len(rows), candidates=len(cands), no_eligible=int((pick < 0).sum()), written=int((use >= 0).sum()),
                             median_eligible=float(np.median(count)), largest_angle=angle)
        print(f"obj {obj_id:6d}: {len(rows)} targets, {len(cands)} candidate views, {len(syms)} symmetries; {stats[obj_id]['no_eligible']} without an eligible "
              f"view, median n_eligible {stats[obj_id]['median_eligible']:g}, largest chosen angle {angle:.2f} deg", file=out)
    entries = [dict(scene_id=sid, im_id=iid, obj_id=obj_id, ref_scene_id=int(chosen[n][0]), ref_im_id=int(chosen[n][1]))
               for n, (sid, iid, obj_id) in enumerate(queries) if n in chosen]
    none = sum(s["no_eligible"] for s in stats.values())
    print(f"total: {len(queries)} targets, {none} without an eligible view ({'given their nearest view' if fallback == 'nearest' else 'left out'}), "
          f"{len(entries)} written; {repeated} key(s) whose object occurs several times in the image (first instance used); "
          f"largest chosen angle {max([s['largest_angle'] for s in stats.values()], default=0.0):.2f} deg", file=out)
    return entries, stats, int(repeated), queries


def _save_json(path, entries):
    """One entry per line, as the toolkit's `inout.save_json` lays a list out."""
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join("  " + json.dumps(e) for e in entries) + "\n]")


def check_ref_targets(path, data_dir, dataset, split="test", max_rot=50.0, min_visib=0.8, cross_scene=True, out=None):
    """Audit an existing list against the rule, writing nothing: one line per entry with the symmetry-aware angle, whether the reference is in
    another scene and the reference's visib_fract, then the totals.  -> the number of entries that break `max_rot`, `min_visib` or the scene
    rule, or name a view that does not exist."""
    from .bop_eval import re_sym
    from .provider import load_json

    out = sys.stdout if out is None else out
    ds = _Dataset(data_dir, dataset, split)
    _, syms_of = ds.symmetries()
    trace_min, bad, angles, n = trace_min_of(max_rot), 0, [], 0
    for n, t in enumerate(load_json(path), 1):
        sid, iid, obj_id, rsid, riid = (int(t[k]) for k in ENTRY_KEYS)
        q = ds.first_instance(ds.test_folder, sid, iid, obj_id)
        folder = ds.ref_folder(rsid)
        c = ds.first_instance(folder, rsid, riid, obj_id)
        head = f"scene {sid} image {iid} object {obj_id} -> scene {rsid} image {riid}:"
        if q is None or c is None:
            bad += 1
            print(f"{head} the {'target' if q is None else 'reference view'} does not exist  BROKEN", file=out)
            continue
        syms = syms_of(obj_id)
        angle = re_sym(q[1], c[1], [dict(R=S) for S in syms])
        within = bool(best_traces(q[1], c[1], syms)[0, 0] >= trace_min)  # the rule's own comparison, not the displayed angle
        other = ds.identity(folder, rsid) != ds.identity(ds.test_folder, sid)
        itself = not other and riid == iid
        visib, px = ds.visibility(folder, rsid, riid, c[0])
        faults = [w for w, broken in (("rotation", not within), ("visibility", not (visib >= min_visib and px > 0)),
                                      ("scene", not other if cross_scene else itself)) if broken]
        bad += bool(faults)
        angles.append(angle)
        print(f"{head} {angle:.3f} deg, {'another' if other else 'the same'} scene, visib_fract {visib:.4f}{'  BROKEN: ' + ', '.join(faults) if faults else ''}", file=out)
    print(f"total: {n} entries, {bad} break the rule (max-rot {max_rot:g}, min-visib {min_visib:g}, {'cross-scene' if cross_scene else 'same-scene'}); "
          f"largest angle {max(angles, default=0.0):.3f} deg", file=out)
    return bad


def write_gt_detections(path, data_dir, dataset, split, queries):
    """A detection file with ground-truth segmentation for the queries [(scene_id, im_id, obj_id)]: the `mask_visib` PNG of the object's first
    instance, as a compressed COCO RLE `provider.rle_decode` accepts, its box (xywh), score 1 and time 0.  A mask without a pixel is left
    out.  -> the number of detections written."""
    from .provider import read_image, rle_counts_to_string, rle_encode

    ds, dets = _Dataset(data_dir, dataset, split), []
    for sid, iid, obj_id in queries:
        slot = ds.first_instance(ds.test_folder, sid, iid, obj_id)[0]
        png = osp.join(ds.test_folder, f"{sid:06d}", "mask_visib", f"{iid:06d}_{slot:06d}.png")
        if not osp.exists(png):
            raise FileNotFoundError(f"ref_targets: {png} is missing: write it with `python -m unopose_amd.gt_info`")
        mask = np.asarray(read_image(png)) > 0
        if mask.ndim == 3:
            mask = mask.any(axis=2)
        if not mask.any():
            continue
        ys, xs = np.nonzero(mask)
        seg = rle_encode(mask)
        dets.append(dict(scene_id=sid, image_id=iid, category_id=obj_id, bbox=[int(xs.min()), int(ys.min()), int(xs.max() - xs.min()) + 1, int(ys.max() - ys.min()) + 1],
                         score=1.0, time=0.0, segmentation=dict(size=seg["size"], counts=rle_counts_to_string(seg["counts"]))))
    _save_json(path, dets)
    return len(dets)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m unopose_amd.ref_targets", description="Write the one-reference target list of a BOP split (the file "
                                 "BOPTestsetOneRef reads as ref_targets_name): per target a keyed-random reference view of the same object within --max-rot "
                                 "degrees up to the object's symmetries, with the HIP all-pairs kernel; --check audits an existing list.")
    ap.add_argument("--data-dir", required=True, help="the folder that holds the dataset folder")
    ap.add_argument("--dataset", required=True)
    ap.add_argument("--split", default="test")
    ap.add_argument("--targets", default="test_targets_bop19.json", help="the targets file inside the dataset folder")
    ap.add_argument("--all-images", action="store_true", help="every (scene, image, object) of the split's scene_gt.json files instead of a targets file")
    ap.add_argument("--max-rot", type=float, default=50.0, help="largest rotation between target and reference, degrees, up to the symmetries")
    ap.add_argument("--min-visib", type=float, default=0.8, help="smallest visib_fract of a reference view")
    ap.add_argument("--same-scene", action="store_true", help="references may come from the target's scene (only the view itself is excluded)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--fallback", choices=("nearest", "skip"), default="nearest", help="a target without an eligible view: its nearest allowed view, or left out")
    ap.add_argument("--out", default=None, help="file name inside the dataset folder (default: test_ref_targets_{crossscene|samescene}_rot{max-rot}.json)")
    ap.add_argument("--overwrite", action="store_true")
    ap.add_argument("--host", action="store_true", help="numpy instead of the kernel: same file, for comparison")
    ap.add_argument("--check", metavar="FILE", default=None, help="write nothing: audit FILE against --max-rot, --min-visib and the scene rule; exit 1 if an entry breaks them")
    ap.add_argument("--gt-dets", metavar="PATH", default=None, help="also write a detection file with the targets' ground-truth visible masks")
    args = ap.parse_args(argv)
    cross = not args.same_scene
    if args.check is not None:
        path = args.check if osp.exists(args.check) else osp.join(args.data_dir, args.dataset, args.check)
        return 1 if check_ref_targets(path, args.data_dir, args.dataset, args.split, args.max_rot, args.min_visib, cross) else 0
    if not 0 <= args.seed < 1 << 64:
        ap.error("--seed is a 64-bit unsigned number")
    path = osp.join(args.data_dir, args.dataset, args.out or default_name(args.max_rot, cross))
    taken = [p for p in (path, args.gt_dets) if p and osp.exists(p)]
    if taken and not args.overwrite:
        raise FileExistsError(f"ref_targets: {', '.join(taken)} exist(s); pass --overwrite to replace")
    entries, _, _, queries = build_ref_targets(args.data_dir, args.dataset, args.split, args.targets, args.all_images, args.max_rot, args.min_visib, cross, args.seed,
                                      args.fallback, None if args.host else "cuda")
    _save_json(path, entries)
    print(f"{len(entries)} entries -> {path}")
    if args.gt_dets:
        n = write_gt_detections(args.gt_dets, args.data_dir, args.dataset, args.split, queries)
        print(f"{n} ground-truth detections -> {args.gt_dets}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
