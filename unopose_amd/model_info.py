"""`models_info.json` of a folder of object models: the 3-D box and the exact diameter of every `obj_XXXXXX.ply`.

The toolkit makes the file with `scripts/calc_model_info.py`: `min_*` / `size_*` are the vertices' minimum and `max - min`, the diameter
is `misc.calc_pts_diameter` -- a Python loop over the vertices, each step a numpy pass over the rest: the square root of the largest
`(pts_diff * pts_diff).sum(axis=1)`, the pair (i, i) included.  The diameter scales the MSSD and ADD(-S) thresholds, the VSD tolerances,
the sphere rule and the discretisation of continuous symmetries, and a user's own meshes come without the file.

`extent_host` is the numpy specification for one object: float64, a squared distance formed as (dx*dx + dy*dy) + dz*dz -- which is how
numpy's `.sum(axis=1)` over three terms rounds -- the maximum over all pairs, `math.sqrt` last; equal to the toolkit's value bit for bit.
`prune_keep` is an exact pruning step both routes take before the all-pairs pass: with c the mean, r_i = |p_i - c|, r_max the largest and
L the distance of an actual pair (found by two farthest-point sweeps starting at the point farthest from c), a point with
(r_i + r_max) (1 + 2^-40) < L cannot belong to a pair at distance >= L:
    |p_i - p_j| <= r_i + r_j <= r_i + r_max < L   (triangle inequality; the margin 2^-40 is ~10^4 times the rounding of the terms compared);
    the pair that gave L is not dropped (its own r_i + r_j >= L), so the maximum over the survivors is the global maximum;
    it is computed from the same pair by the same expression, so it has the same bits.
`compute_models_info` does a set of objects, on the host or -- with a CUDA `device` -- with csrc/modelinfo.hip through `ops.pts_extent`
(same bits).  `write_models_info` writes the file for a folder, `python -m unopose_amd.model_info` is its command line, and
`bop_eval.load_dataset(..., models_info="compute")` scores a dataset that has no such file."""
import argparse
import json
import math
import os
import os.path as osp
import re
import sys

import numpy as np

INFO_KEYS = ("diameter", "min_x", "min_y", "min_z", "size_x", "size_y", "size_z")
SYMMETRY_KEYS = ("symmetries_discrete", "symmetries_continuous")  # annotations: carried over, never computed here (model_sym.py finds and writes them)
PRUNE_MARGIN = 1.0 + 2.0 ** -40
HOST_BLOCK = 1 << 21  # squared distances the host route forms at a time
_PLY_NAME = re.compile(r"^obj_(\d{6})\.ply$")


def _points(pts):
    p = np.ascontiguousarray(np.asarray(pts, dtype=np.float64))
    if p.ndim != 2 or p.shape[1] != 3 or p.shape[0] < 1 or not np.isfinite(p).all():
        raise ValueError(f"model_info: points of shape {p.shape}: (V, 3) with V >= 1, all finite")
    return p


def _d2_to(p, q):
    """Squared distance of every point of p (V, 3) to the point q, in the association of the specification."""
    dx, dy, dz = p[:, 0] - q[0], p[:, 1] - q[1], p[:, 2] - q[2]
    return (dx * dx + dy * dy) + dz * dz


def prune_keep(pts):
    """The points that may belong to a farthest pair (module docstring) -> bool (V,).  At least the pair behind L is kept."""
    p = _points(pts)
    r = np.sqrt(_d2_to(p, p.mean(axis=0)))
    a = int(np.argmax(r))
    b = int(np.argmax(_d2_to(p, p[a])))
    L = math.sqrt(float(_d2_to(p, p[b]).max()))
    return ~((r + r[a]) * PRUNE_MARGIN < L)


def max_d2_host(pts, block=HOST_BLOCK):
    """The largest (dx*dx + dy*dy) + dz*dz over all pairs (i, j >= i) of pts (V, 3), `block` distances at a time: O(block) memory."""
    p = _points(pts)
    x, y, z = (np.ascontiguousarray(p[:, c]) for c in range(3))
    V, best = len(p), 0.0
    a = 0
    while a < V:
        rows = max(1, int(block) // (V - a))
        d2 = np.square(x[a:a + rows, None] - x[None, a:])
        d2 += np.square(y[a:a + rows, None] - y[None, a:])
        d2 += np.square(z[a:a + rows, None] - z[None, a:])
        best = max(best, float(d2.max()))
        a += rows
    return best


def extent_host(pts, prune=True, block=HOST_BLOCK):
    """The toolkit's box and diameter of pts (V, 3) float64 -> (min (3,), size (3,) = max - min, diameter).  `prune` only saves time: both
    settings give the same bits.  One point, or only duplicates, gives 0.0."""
    p = _points(pts)
    lo = p.min(axis=0)
    return lo, p.max(axis=0) - lo, math.sqrt(max_d2_host(p[prune_keep(p)] if prune else p, block))


def _entry(lo, size, diameter):
    return dict(diameter=float(diameter), min_x=float(lo[0]), min_y=float(lo[1]), min_z=float(lo[2]), size_x=float(size[0]), size_y=float(size[1]),
                size_z=float(size[2]))


def compute_models_info(models, device=None, prune=True):
    """models: {obj_id: (V, 3) points, or a dictionary with "pts"} -> {obj_id: {"diameter", "min_x", "min_y", "min_z", "size_x", "size_y",
    "size_z"}}, Python floats.  device=None: the host route (`extent_host`); a CUDA device: one `ops.pts_extent` call for all objects.  The
    two routes give equal bits."""
    ids = list(models)
    pts = [_points(models[o]["pts"] if isinstance(models[o], dict) else models[o]) for o in ids]
    if device is None:
        rows = [extent_host(p, prune=prune) for p in pts]
    elif not ids:
        rows = []
    else:
        from .bop_eval import _cuda_device
        from .ops.score import pts_extent

        rows = list(zip(*pts_extent(pts, _cuda_device(device), prune=prune)))
    return {o: _entry(*row) for o, row in zip(ids, rows)}


def model_files(folder):
    """{obj_id: path} of the folder's `obj_XXXXXX.ply` files, by id."""
    if not osp.isdir(folder):
        raise FileNotFoundError(f"model_info: {folder} is not a folder")
    found = {int(m.group(1)): osp.join(folder, f) for f in os.listdir(folder) for m in [_PLY_NAME.match(f)] if m}
    if not found:
        raise FileNotFoundError(f"model_info: no obj_XXXXXX.ply in {folder}")
    return dict(sorted(found.items()))


def compute_folder(folder, device="cuda", prune=True):
    """`compute_models_info` for every `obj_XXXXXX.ply` of `folder`, read with `bop_eval.read_ply` -> {obj_id: entry}."""
    from .bop_eval import read_ply

    return compute_models_info({o: read_ply(path)["pts"] for o, path in model_files(folder).items()}, device=device, prune=prune)


def _load(path):
    with open(path) as f:
        return {int(k): v for k, v in json.load(f).items()}


def _save_json(path, info):
    """One object per line, keys as strings, as the toolkit's `inout.save_json` lays the file out."""
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f'  "{o}": {json.dumps(info[o])}' for o in sorted(info)) + "\n}")


def write_models_info(folder, device="cuda", prune=True, force=False):
    """Write `<folder>/models_info.json` for every `obj_XXXXXX.ply` of `folder`.  `device`: the GPU of the device route, None = the host route.
    An existing file is an error unless `force`; then each object's `symmetries_discrete` / `symmetries_continuous` entries are carried
    over from it -- they are annotations and cannot be computed.  -> {obj_id: entry} as written."""
    path = osp.join(folder, "models_info.json")
    if osp.exists(path) and not force:
        raise FileExistsError(f"model_info: {path} exists; pass force=True (--force) to replace it (its symmetry entries are kept)")
    old = _load(path) if osp.exists(path) else {}
    info = compute_folder(folder, device=device, prune=prune)
    for o, entry in info.items():
        entry.update({k: old[o][k] for k in SYMMETRY_KEYS if k in old.get(o, {})})
    _save_json(path, info)
    return info


def check_models_info(folder, device="cuda", prune=True, out=None):
    """Compare `<folder>/models_info.json` with the computed values, writing nothing: one line per object with the stored and the computed
    diameter and their relative difference.  -> the ids of the objects that have a model but no entry in the file."""
    out = sys.stdout if out is None else out
    stored, info = _load(osp.join(folder, "models_info.json")), compute_folder(folder, device=device, prune=prune)
    missing = []
    for o, entry in info.items():
        if o not in stored or "diameter" not in stored[o]:
            missing.append(o)
            print(f"obj {o:6d}  stored        missing  computed {entry['diameter']!r}", file=out)
            continue
        was, now = float(stored[o]["diameter"]), entry["diameter"]
        rel = abs(was - now) / now if now > 0 else (0.0 if was == now else float("inf"))
        print(f"obj {o:6d}  stored {was!r}  computed {now!r}  relative difference {rel:.3e}{'' if was == now else '  DIFFERENT'}", file=out)
    return missing


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m unopose_amd.model_info", description="Write models_info.json (3-D box and exact diameter, the toolkit's "
                                 "calc_model_info.py) for the obj_XXXXXX.ply files of a BOP dataset's models folder, with the HIP all-pairs kernel.")
    ap.add_argument("--data-dir", required=True, help="the folder that holds the dataset folder")
    ap.add_argument("--dataset", required=True)
    ap.add_argument("--models", default="models_eval", help="the models folder inside the dataset (default: models_eval)")
    ap.add_argument("--host", action="store_true", help="numpy instead of the kernel: same bits, for comparison")
    ap.add_argument("--force", action="store_true", help="replace an existing models_info.json (its symmetry entries are kept)")
    ap.add_argument("--check", action="store_true", help="write nothing: compare the existing file with the computed values; non-zero exit if an object is missing")
    args = ap.parse_args(argv)
    folder, device = osp.join(args.data_dir, args.dataset, args.models), None if args.host else "cuda"
    if args.check:
        missing = check_models_info(folder, device=device)
        if missing:
            print(f"{len(missing)} object(s) without an entry in {osp.join(folder, 'models_info.json')}: {missing}")
        return 1 if missing else 0
    info = write_models_info(folder, device=device, force=args.force)
    print("%d objects -> %s" % (len(info), osp.join(folder, "models_info.json")))
    return 0


if __name__ == "__main__":
    sys.exit(main())
