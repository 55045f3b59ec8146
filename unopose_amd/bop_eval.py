"""BOP'19 localization scoring of a result CSV at the level this environment allows.

What the reference runs after `save_unopose.sh` is bop_toolkit's `eval_bop19_pose.py`: per estimate the pose errors
VSD, MSSD and MSPD against the ground truth, greedy matching per image / object in order of decreasing score, recall per
correctness threshold, AR = mean of the three average recalls (`core/unopose/engine/bop_eval_utils.py:340-454` then only
tabulates the toolkit's score files).  This module implements all three: **MSSD** (thresholds 0.05 ... 0.5 of the object
diameter), **MSPD** (5 ... 50 px at 640 px image width) and **VSD** (misalignment tolerances tau = 0.05 ... 0.5 of the diameter x
correctness thresholds 0.05 ... 0.5, visibility tolerance delta = 15 mm; `pose_error.py:17-101`, `visibility.py:44-70`,
`misc.py:142-162`), the matching and the recall averaging.  VSD needs depth maps of the object model in the estimated and the
ground-truth pose: `average_recall(..., renderer=..., depth_images=...)` takes any object with the toolkit's `render_object`
call -- `unopose_amd.render.HipDepthRenderer` is the HIP rasteriser (csrc/raster.hip); without a renderer AR_VSD and the BOP AR
are None, never faked.  Pinned against bop_toolkit_lib's own `pose_error.vsd / mssd / mspd`, `pose_matching.match_poses_scene` and
`score.calc_localization_scores` (tests/golden/make_bop_eval_golden.py; for VSD both sides score the same rendered depth).
Two routes to the same numbers: the host route (numpy per estimate; only the rasteriser is a device kernel) and, with
`average_recall(..., device=...)`, the device route: depth maps stay on the GPU and csrc/bopscore.hip turns them into the integer counts
of `vsd` and the `mssd` / `mspd` distances for many pairs per launch; the matching and the recall averaging are the same host code.
`load_dataset` reads a BOP dataset folder for scoring (own PLY reader, symmetries as the toolkit lists them, targets file) and
`score_csv` ties it to a result file, as the reference's test run does after saving (`--eval` of unopose_amd.cli).

Beyond BOP'19, `average_recall(..., error_types=...)` scores the error types of the reference's own script
(`lib/pysixd/scripts/eval_pose_results_more.py:41-156`): `add, adi, ad, ABSadd, ABSadi, ABSad, AUCadd, AUCadi, AUCad, re, te, rete, proj, reS, teS,
reteS, projS` -- `ERROR_TYPES` holds their thresholds, units and normalisation, `add, adi, proj, re, te, proj_sym, re_sym, te_sym` are the host
functions (`lib/pysixd/pose_error.py`), csrc/posemetrics.hip the device route (`ops.pose_metrics`, `ops.adi`), and every such type adds a
block with per-object recalls under `out["errors"]`.  The mask-overlap error `cus` and the other mask / bounding-box errors stay out.
A deliberate difference: which objects take ADI under `ad / ABSad / AUCad` is not read from per-dataset id tables
(`lib/pysixd/dataset_params.py:96-130`) but from the models -- an object whose `models_info.json` entry lists a discrete or continuous
symmetry -- unless `symmetric_obj_ids=` (config key `bop_eval.symmetric_obj_ids`) says otherwise; the ids used are written with the scores.
Which ground truths count: by default every ground truth of a targeted object.  With `gt_info=` (the entries of `scene_gt_info.json`, read by
`load_dataset(..., gt_info=True)` or computed by `unopose_amd.gt_info`) it is the toolkit's rule (`scripts/eval_calc_scores.py:205-238`): the
`inst_count` most visible ground truths of each target object, or with `visib_gt_min >= 0` those visible to at least that fraction;
`score_csv(..., gt_visibility="file" | "compute")` and the config keys `bop_eval.gt_visibility`, `bop_eval.visib_gt_min` select it.
Where the diameters come from: `models_eval/models_info.json`, or with `models_info="compute"` (config key `bop_eval.models_info`) the models'
own vertices (`unopose_amd.model_info`, csrc/modelinfo.hip), for meshes that come without the file."""
import json
import os.path as osp

import numpy as np

MSSD_THRESHOLDS = np.arange(0.05, 0.51, 0.05)  # fractions of the object diameter
MSPD_THRESHOLDS = np.arange(5, 51, 5)          # pixels at 640 px image width
VSD_TAUS = np.arange(0.05, 0.51, 0.05)         # misalignment tolerances, fractions of the object diameter
VSD_THRESHOLDS = np.arange(0.05, 0.51, 0.05)   # correctness thresholds on the VSD error
VSD_DELTA = 15.0                               # visibility tolerance in mm (every BOP dataset but ITODD: bop_eval_utils.py:348-362)
VSD_DELTAS = {"itodd": 5.0}                    # the exception of that table
# budget of the device route's depth maps alive at a time, rendered and test ones: about 218 maps of 480 x 640.  The index and count tensors
# of a launch and one stacked copy of a chunk's test images come on top of it.
DEVICE_CHUNK_BYTES = 256 << 20
MAX_SYM_DISC_STEP = 0.01                       # the toolkit's discretisation of continuous symmetries (eval_bop19_pose.py)


def read_results(path):
    """The runner's CSV (scene_id,im_id,obj_id,score,R 9 values,t 3 values in mm,time) -> list of dicts."""
    out = []
    with open(path) as f:
        for line in f:
            c = line.strip().split(",")
            if len(c) != 7 or c[0] == "scene_id":
                continue
            out.append(dict(scene_id=int(c[0]), im_id=int(c[1]), obj_id=int(c[2]), score=float(c[3]),
                            R=np.array(c[4].split(), dtype=np.float64).reshape(3, 3), t=np.array(c[5].split(), dtype=np.float64),
                            time=float(c[6])))
    return out


def _sym_poses(R_gt, t_gt, syms):
    """Ground-truth pose composed with every symmetry of the object: (S,3,3), (S,3).  syms: list of {"R", "t"}."""
    Rs = np.stack([np.asarray(s["R"], np.float64).reshape(3, 3) for s in syms])
    ts = np.stack([np.asarray(s["t"], np.float64).reshape(3) for s in syms])
    return R_gt @ Rs, ts @ R_gt.T + t_gt.reshape(1, 3)


def mssd(R_est, t_est, R_gt, t_gt, pts, syms):
    """Maximum symmetry-aware surface distance: min over symmetries of the largest point displacement (model units)."""
    est = pts @ R_est.T + t_est.reshape(1, 3)
    Rg, tg = _sym_poses(R_gt, t_gt.reshape(3), syms)
    gt = np.einsum("sij,nj->sni", Rg, pts) + tg[:, None, :]
    return float(np.linalg.norm(gt - est[None], axis=2).max(axis=1).min())


def _project(pts_cam, K):
    uvw = pts_cam @ K.T
    return uvw[..., :2] / uvw[..., 2:3]


def mspd(R_est, t_est, R_gt, t_gt, K, pts, syms):
    """Maximum symmetry-aware projection distance in pixels."""
    est = _project(pts @ R_est.T + t_est.reshape(1, 3), K)
    Rg, tg = _sym_poses(R_gt, t_gt.reshape(3), syms)
    gt = _project(np.einsum("sij,nj->sni", Rg, pts) + tg[:, None, :], K)
    return float(np.linalg.norm(gt - est[None], axis=2).max(axis=1).min())


# ---- the further error types of lib/pysixd/scripts/eval_pose_results_more.py ----------------------------------------------------------
DEFAULT_ERROR_TYPES = ("vsd", "mssd", "mspd")
_AD_TH, _ABS_TH, _RT_TH = [[0.02], [0.05], [0.1]], [[2.0]], [[2.0], [5.0], [10.0]]
_AUC_TH = [[float(th)] for th in np.linspace(10 / 10, 10, num=10)]


def _etype(elements, thresholds, by_diameter=False, sphere_rule=False, cm=False, auc=False):
    return dict(elements=elements, thresholds=thresholds, by_diameter=by_diameter, sphere_rule=sphere_rule, cm=cm, auc=auc)


# type -> elements: the errors that make it up ("ad" = "adi" for a symmetric object, else "add"; `rete` carries two);
#   thresholds: one list per correctness setting, one value per element (eval_pose_results_more.py:74-155);
#   by_diameter: divided by the object diameter before thresholding (eval_calc_scores.py:70);
#   sphere_rule: inf when |t_e - t_g| >= diameter, the spheres around the two poses do not overlap (eval_calc_errors.py:367-426);
#   cm: every element in mm is divided by 10 (ABS*, AUC*; eval_calc_errors.py:473-527) -- "te" / "teS" elements always are (:569-591);
#   auc: an area-under-curve metric, tabulated as the mean over its thresholds (bop_eval_utils.py:191-194).
ERROR_TYPES = {
    "add": _etype(("add",), _AD_TH, by_diameter=True, sphere_rule=True), "adi": _etype(("adi",), _AD_TH, by_diameter=True, sphere_rule=True),
    "ad": _etype(("ad",), _AD_TH, by_diameter=True, sphere_rule=True),
    "ABSadd": _etype(("add",), _ABS_TH, cm=True), "ABSadi": _etype(("adi",), _ABS_TH, cm=True), "ABSad": _etype(("ad",), _ABS_TH, cm=True),
    "AUCadd": _etype(("add",), _AUC_TH, cm=True, auc=True), "AUCadi": _etype(("adi",), _AUC_TH, cm=True, auc=True),
    "AUCad": _etype(("ad",), _AUC_TH, cm=True, auc=True),
    "re": _etype(("re",), _RT_TH), "te": _etype(("te",), _RT_TH), "rete": _etype(("re", "te"), [[2.0, 2.0], [5.0, 5.0], [10.0, 10.0]]),
    "proj": _etype(("proj",), _RT_TH),
    "reS": _etype(("reS",), _RT_TH), "teS": _etype(("teS",), _RT_TH), "reteS": _etype(("reS", "teS"), [[2.0, 2.0], [5.0, 5.0], [10.0, 10.0]]),
    "projS": _etype(("projS",), _RT_TH),
}
KNOWN_ERROR_TYPES = DEFAULT_ERROR_TYPES + tuple(ERROR_TYPES)
ADI_CHUNK = 1 << 21  # distances the host `adi` forms at a time


def parse_error_types(spec):
    """`bop_eval.error_types` as the reference's `val_cfg` spells it -- a comma-separated string -- or a list / tuple -> tuple of names in
    the order given, duplicates dropped; None = the BOP'19 three.  An unknown name is a ValueError that lists the known ones."""
    if spec is None:
        return DEFAULT_ERROR_TYPES
    names = [n.strip() for n in spec.split(",")] if isinstance(spec, str) else [str(n).strip() for n in spec]
    names = list(dict.fromkeys(n for n in names if n))
    unknown = [n for n in names if n not in KNOWN_ERROR_TYPES]
    if unknown or not names:
        raise ValueError(f"bop_eval: unknown error type(s) {unknown} -- known: {', '.join(KNOWN_ERROR_TYPES)}")
    return tuple(names)


def add(R_est, t_est, R_gt, t_gt, pts):
    """Average distance of the model points between the two poses (pose_error.py:255-270), model units."""
    est, gt = pts @ R_est.T + t_est.reshape(1, 3), pts @ R_gt.T + t_gt.reshape(1, 3)
    return float(np.linalg.norm(est - gt, axis=1).mean())


def adi(R_est, t_est, R_gt, t_gt, pts, chunk=ADI_CHUNK):
    """Average distance from each model point in the ground-truth pose to the NEAREST model point in the estimated pose
    (pose_error.py:273-295, a KD-tree there): brute force in float64, `chunk` squared distances at a time formed per coordinate as
    (dx^2 + dy^2) + dz^2, the sqrt after the min."""
    est, gt = pts @ R_est.T + t_est.reshape(1, 3), pts @ R_gt.T + t_gt.reshape(1, 3)
    rows, e = max(1, int(chunk) // len(pts)), np.ascontiguousarray(est.T)
    near = []
    for a in range(0, len(pts), rows):
        g = gt[a:a + rows]
        d2 = np.square(g[:, 0:1] - e[0][None])
        d2 += np.square(g[:, 1:2] - e[1][None])
        d2 += np.square(g[:, 2:3] - e[2][None])
        near.append(np.sqrt(d2.min(axis=1)))
    return float(np.concatenate(near).mean())


def proj(R_est, t_est, R_gt, t_gt, K, pts):
    """Average distance of the model points' projections, px (pose_error.py:438-443 `arp_2d`)."""
    return float(np.linalg.norm(_project(pts @ R_est.T + t_est.reshape(1, 3), K) - _project(pts @ R_gt.T + t_gt.reshape(1, 3), K), axis=1).mean())


def proj_sym(R_est, t_est, R_gt, t_gt, K, pts, syms):
    """`proj`, the minimum over the object's symmetries (pose_error.py:182-192 `arp_2d_sym`)."""
    est = _project(pts @ R_est.T + t_est.reshape(1, 3), K)
    Rg, tg = _sym_poses(R_gt, t_gt.reshape(3), syms)
    gt = _project(np.einsum("sij,nj->sni", Rg, pts) + tg[:, None, :], K)
    return float(np.linalg.norm(gt - est[None], axis=2).mean(axis=1).min())


def _composed_t(R_gt, t_gt, syms):
    """R_gt S_t + t_gt of every symmetry, each sum in the fixed order ((a + b) + c) + t that csrc/posemetrics.hip keeps -> (S,3)."""
    ts = np.stack([np.asarray(s["t"], np.float64).reshape(3) for s in syms])
    Rg, tg = np.asarray(R_gt, np.float64), np.asarray(t_gt, np.float64).reshape(3)
    return np.stack([Rg[r, 0] * ts[:, 0] + Rg[r, 1] * ts[:, 1] + Rg[r, 2] * ts[:, 2] + tg[r] for r in range(3)], axis=1)


def _fma(a, b, c):
    """a b + c with ONE rounding, elementwise on float64 arrays: numpy has no fused multiply-add, so the product is split exactly (Dekker),
    added to c exactly (Knuth) and the two tails are added with rounding to odd, after which the last addition rounds as the fused
    operation does (Boldo and Melquiond, "Emulation of a FMA and correctly rounded sums", 2008).  No overflow or underflow: the operands
    here are entries of rotations."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))

    def split(x):
        t = 134217729.0 * x  # 2^27 + 1
        hi = t - (t - x)
        return hi, x - hi

    def two_sum(x, y):
        s = x + y
        yy = s - x
        return s, (x - (s - yy)) + (y - yy)

    p = a * b
    (ah, al), (bh, bl) = split(a), split(b)
    pl = (((ah * bh - p) + ah * bl) + al * bh) + al * bl  # p + pl = a b exactly
    th, tl = two_sum(c, p)
    v, err = two_sum(tl, pl)
    even = (np.asarray(v).view(np.int64) & 1) == 0
    v = np.where((err != 0) & even, np.nextafter(v, np.where(err > 0, np.inf, -np.inf)), v)  # round to odd
    return th + v


def _dot3(a0, b0, a1, b1, a2, b2):
    """One element of a 3 x 3 product in a fixed order: a0 b0 rounded, then two fused multiply-adds.  This is how the BLAS product of
    pose_error.py:357-372 rounded when tests/golden/pose_metrics.json was recorded; written out, the value no longer depends on the BLAS
    numpy was built with, and csrc/posemetrics.hip's dot3_blas is the same expression."""
    return _fma(a2, b2, _fma(a1, b1, np.asarray(a0, np.float64) * np.asarray(b0, np.float64)))


def _rotation_degrees(R_est, R):
    """arccos of the clamped 0.5 (trace(R_est R^T) - 1) in degrees for R (..., 3, 3): the diagonal by `_dot3`, added in order."""
    d = [_dot3(R_est[r, 0], R[..., r, 0], R_est[r, 1], R[..., r, 1], R_est[r, 2], R[..., r, 2]) for r in range(3)]
    trace = np.minimum((d[0] + d[1]) + d[2], 3.0)
    return np.rad2deg(np.arccos(np.clip(0.5 * (trace - 1.0), -1.0, 1.0)))


def re(R_est, R_gt):
    """Rotation error in degrees: arccos of the clamped 0.5 (trace(R_est R_gt^T) - 1) (pose_error.py:357-372).  Near 0 degrees the result
    moves by 1e-6 degrees per ulp of the trace (an exact copy of a rotation scores 0 or ~2e-6), so the trace is formed by explicit
    arithmetic in one fixed order (`_dot3`), which csrc/posemetrics.hip restates."""
    return float(_rotation_degrees(np.asarray(R_est, np.float64).reshape(3, 3), np.asarray(R_gt, np.float64).reshape(3, 3)))


def re_sym(R_est, R_gt, syms):
    """`re` against R_gt S_R, the minimum over the object's symmetries (pose_error.py:375-394); R_gt S_R by `_dot3` too."""
    Rg, Q = np.asarray(R_gt, np.float64).reshape(3, 3), np.stack([np.asarray(s["R"], np.float64).reshape(3, 3) for s in syms])
    T = np.stack([np.stack([_dot3(Rg[r, 0], Q[:, 0, c], Rg[r, 1], Q[:, 1, c], Rg[r, 2], Q[:, 2, c]) for c in range(3)], axis=1) for r in range(3)], axis=1)
    return float(_rotation_degrees(np.asarray(R_est, np.float64).reshape(3, 3), T).min())


def te(t_est, t_gt):
    """Translation error |t_gt - t_est| in model units (pose_error.py:404-415)."""
    d = np.asarray(t_gt, np.float64).reshape(3) - np.asarray(t_est, np.float64).reshape(3)
    return float(np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))


def te_sym(t_est, t_gt, R_gt, syms):
    """`te`, the minimum over the object's symmetries: |R_gt S_t + t_gt - t_est| (pose_error.py:418-435)."""
    d = _composed_t(R_gt, t_gt, syms) - np.asarray(t_est, np.float64).reshape(1, 3)
    return float(np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]).min()))


def default_symmetric_obj_ids(models):
    """The objects that take ADI under `ad / ABSad / AUCad`: those whose symmetry list holds more than the identity."""
    return sorted(o for o, m in models.items() if len(m["symmetries"]) > 1)


def _bases(types, symmetric):
    """The errors an object's pairs need for `types`."""
    out = set()
    for T in types:
        if T in ERROR_TYPES:
            out.update(("adi" if symmetric else "add") if e == "ad" else e for e in ERROR_TYPES[T]["elements"])
    return out


def _adi_wanted(types, symmetric, apart):
    """Does a pair need its ADI?  `apart`: the sphere rule holds (|t_e - t_g| >= diameter), so the types under it are inf without it."""
    return any("adi" in _bases((T,), symmetric) and not (ERROR_TYPES[T]["sphere_rule"] and apart) for T in types if T in ERROR_TYPES)


def metric_pairs(walk, models, types, symmetric_obj_ids):
    """The pairs the further error types are computed for -> [dict(key, r, g, K, obj_id, apart, bases)], keys as `scored_pairs` documents
    them.  The sphere rule is decided here, on the host, from |t_e - t_g| and the diameter: a pair under it is not handed to ADI."""
    out = []
    for sid, iid, K, obj_id, rows, mine in scored_pairs(walk):
        sym = obj_id in symmetric_obj_ids
        for rank, r in enumerate(rows):
            for gid, g in mine:
                apart = not (np.linalg.norm(np.asarray(r["t"], np.float64).reshape(3) - np.asarray(g["t"], np.float64).reshape(3)) < models[obj_id]["diameter"])
                bases = _bases(types, sym)
                if "adi" in bases and not _adi_wanted(types, sym, apart):
                    bases = bases - {"adi"}
                out.append(dict(key=(sid, iid, obj_id, rank, gid), r=r, g=g, K=K, obj_id=obj_id, apart=apart, bases=bases))
    return out


def host_pose_metrics(pairs, models):
    """The errors each pair needs, with the host functions -> {key: {name: value}}."""
    out = {}
    for p in pairs:
        m, (Re, te_), (Rg, tg) = models[p["obj_id"]], (np.asarray(p["r"]["R"], np.float64), np.asarray(p["r"]["t"], np.float64)), \
            (np.asarray(p["g"]["R"], np.float64), np.asarray(p["g"]["t"], np.float64))
        if not (np.isfinite(Re).all() and np.isfinite(te_).all() and np.isfinite(Rg).all() and np.isfinite(tg).all()):
            out[p["key"]] = {b: float("nan") for b in p["bases"]}
            continue
        fn = dict(add=lambda: add(Re, te_, Rg, tg, m["pts"]), adi=lambda: adi(Re, te_, Rg, tg, m["pts"]), proj=lambda: proj(Re, te_, Rg, tg, p["K"], m["pts"]),
                  re=lambda: re(Re, Rg), te=lambda: te(te_, tg), projS=lambda: proj_sym(Re, te_, Rg, tg, p["K"], m["pts"], m["symmetries"]),
                  reS=lambda: re_sym(Re, Rg, m["symmetries"]), teS=lambda: te_sym(te_, tg, Rg, m["symmetries"]))
        out[p["key"]] = {b: fn[b]() for b in p["bases"]}
    return out


def device_pose_metrics(pairs, models, device):
    """`host_pose_metrics` on the device: one `ops.pose_metrics` launch per object (with the identity alone where no symmetry-aware error is
    asked for, and without the projS pass where projS is not) plus `ops.adi` for the pairs that need ADI, everything queued before the
    first read-back -> {key: {name: value}}."""
    from .ops.score import adi as adi_op, pose_metrics

    dev = _cuda_device(device)
    by_obj = {}
    for p in pairs:
        by_obj.setdefault(p["obj_id"], []).append(p)
    pending = []
    for obj_id, group in by_obj.items():
        m = models[obj_id]
        poses = lambda g: ([p["r"]["R"] for p in g], [p["r"]["t"] for p in g], [p["g"]["R"] for p in g], [p["g"]["t"] for p in g])  # noqa: E731
        several = [p for p in group if p["bases"] - {"adi"}]
        if several:
            syms = m["symmetries"] if any(p["bases"] & {"projS", "reS", "teS"} for p in several) else [dict(R=np.eye(3), t=np.zeros(3))]
            proj_sym = any("projS" in p["bases"] for p in several)  # reS / teS alone do not pay for points x symmetries projections
            pending.append((several, None, pose_metrics(m["pts"], syms, *poses(several), [p["K"] for p in several], dev, proj_sym=proj_sym)))
        nearest = [p for p in group if "adi" in p["bases"]]
        for a in range(0, len(nearest), 65535):  # the launch limit of pairs
            pending.append((nearest[a:a + 65535], "adi", adi_op(m["pts"], *poses(nearest[a:a + 65535]), dev)))
    out = {p["key"]: {} for p in pairs}
    for group, name, res in pending:  # read back after everything is queued
        cols = {name: res.cpu().numpy()} if name else {k: v.cpu().numpy() for k, v in res.items()}
        for i, p in enumerate(group):
            out[p["key"]].update({b: float(cols[b][i]) for b in p["bases"] if b in cols})
    return out


def pair_error(T, values, diameter, symmetric, apart):
    """The error elements of type `T` for one pair, as eval_calc_errors.py stores and eval_calc_scores.py normalises them: list of floats."""
    spec = ERROR_TYPES[T]
    if spec["sphere_rule"] and apart:
        return [float("inf")]
    out = []
    for e in spec["elements"]:
        e = ("adi" if symmetric else "add") if e == "ad" else e
        v = values[e]
        if spec["cm"] or e in ("te", "teS"):
            v = v / 10  # mm to cm
        out.append(v / diameter if spec["by_diameter"] else v)
    return out


def localization_scores(per_image, thresholds, obj_ids, n_top):
    """`pose_matching.match_poses` per image and `score.calc_localization_scores`: greedy matching in order of decreasing score -- an
    estimate takes the free valid ground truth for which EVERY error element is below the threshold and below the best so far -- then
    recall = matched / targets over everything and per object (0 for an object without targets; with n_top > 0 an image holds at most
    n_top targets of an object).  per_image: [(gts, [dict(score, errors={gid: [elements]})])] -> (recall, {obj_id: recall})."""
    tp, tars = {o: 0 for o in obj_ids}, {o: 0 for o in obj_ids}
    for gts, ests in per_image:
        count = {}
        for g in gts:
            if g["valid"]:
                count[g["obj_id"]] = count.get(g["obj_id"], 0) + 1
        for o, c in count.items():
            tars[o] = tars.get(o, 0) + (min(n_top, c) if n_top > 0 else c)
        taken = []
        for e in sorted(ests, key=lambda e: e["score"], reverse=True):
            best, best_err = -1, list(thresholds)
            for gid, err in e["errors"].items():
                if gts[gid]["valid"] and gid not in taken and all(err[i] < best_err[i] for i in range(len(thresholds))):
                    best, best_err = gid, err
            if best >= 0:
                taken.append(best)
        for gid in taken:
            tp[gts[gid]["obj_id"]] = tp.get(gts[gid]["obj_id"], 0) + 1
    n_tars = sum(tars.values())
    return (sum(tp.values()) / float(n_tars) if n_tars else 0.0), {o: (tp[o] / float(tars[o]) if tars[o] else 0.0) for o in tars}


def _error_block(thresholds, tables, weights):
    """One entry of out["errors"] from [(recall, {obj_id: recall})] per threshold.  `weights` {obj_id: instances} weighs the mean over the
    objects (vsd / mssd / mspd: bop_eval_utils.py:197-200, 270-277); None is the plain mean."""
    recalls = [t[0] for t in tables]
    objs = sorted(tables[0][1]) if tables else []
    obj_recalls = {o: [t[1][o] for t in tables] for o in objs}
    per_obj = [float(np.mean(obj_recalls[o])) for o in objs]
    if weights is None or not objs:
        mean_obj = float(np.mean(per_obj)) if objs else 0.0
    else:
        w = np.asarray([weights.get(o, 0) for o in objs], np.float64)
        mean_obj = float((w / w.sum() * np.asarray(per_obj)).sum()) if w.sum() > 0 else 0.0
    return dict(thresholds=thresholds, recalls=recalls, mean_recall=float(np.mean(recalls)), obj_recalls=obj_recalls, mean_obj_recall=mean_obj)


def format_error_table(errors):
    """The per-object table the reference prints after scoring (bop_eval_utils.summary_scores): objects in rows, `type_threshold` in
    columns -- an area-under-curve type (AUC*, vsd, mssd, mspd) as ONE column `type_min:max` with the mean over its thresholds -- recalls
    in percent, and an `Avg(n)` row with the mean over the objects (weighted by the instance counts for vsd / mssd / mspd)."""
    def th_str(th):
        return "-".join(dict.fromkeys("%g" % v for v in th))

    cols, objs = [], []
    for T, blk in errors.items():
        objs = sorted(set(objs) | set(blk["obj_recalls"]))
        rec = {o: np.asarray(v, np.float64).reshape(-1) for o, v in blk["obj_recalls"].items()}
        if T in DEFAULT_ERROR_TYPES or ERROR_TYPES[T]["auc"]:
            lo, hi = (0.05, 0.5) if T in ("vsd", "mssd") else (5, 50) if T == "mspd" else (blk["thresholds"][0][0], blk["thresholds"][-1][0])
            cols.append((f"{T}_{lo:g}:{hi:g}", {o: float(v.mean()) for o, v in rec.items()}, blk["mean_obj_recall"]))
        else:
            for i, th in enumerate(blk["thresholds"]):
                cols.append((f"{T}_{th_str(th)}", {o: float(v[i]) for o, v in rec.items()}, float(np.mean([v[i] for v in rec.values()])) if rec else 0.0))
    rows = [["objects"] + [c[0] for c in cols]]
    rows += [[str(o)] + ["%.2f" % (100.0 * c[1][o]) if o in c[1] else "-" for c in cols] for o in objs]
    rows.append(["Avg(%d)" % len(objs)] + ["%.2f" % (100.0 * c[2]) for c in cols])
    width = [max(len(r[i]) for r in rows) for i in range(len(rows[0]))]
    return "\n".join("  ".join(v.ljust(width[i]) if i == 0 else v.rjust(width[i]) for i, v in enumerate(r)) for r in rows)


def depth_to_dist(depth, K):
    """Depth image (z) -> distance to the camera centre, 0 where there is no depth (misc.py:142-162)."""
    H, W = depth.shape
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    pre_x, pre_y = (xs - K[0, 2]) / np.float64(K[0, 0]), (ys - K[1, 2]) / np.float64(K[1, 1])
    return np.sqrt(np.multiply(pre_x, depth) ** 2 + np.multiply(pre_y, depth) ** 2 + depth.astype(np.float64) ** 2)


def _visib_mask(d_test, d_model, delta):
    """visibility.py:30-41, visib_mode "bop19": the model surface is visible where it is not behind the scene by more than
    delta, or where the scene has no depth."""
    d_diff = d_model.astype(np.float32) - d_test.astype(np.float32)
    return np.logical_and(np.logical_or(d_diff <= delta, d_test == 0), d_model > 0)


def vsd(depth_est, depth_gt, depth_test, K, delta, taus, diameter, normalized_by_diameter=True):
    """Visible Surface Discrepancy for every tau (pose_error.py:17-101, cost_type "step") from the two rendered depth maps."""
    dist_test, dist_gt, dist_est = depth_to_dist(depth_test, K), depth_to_dist(depth_gt, K), depth_to_dist(depth_est, K)
    visib_gt = _visib_mask(dist_test, dist_gt, delta)
    visib_est = np.logical_or(_visib_mask(dist_test, dist_est, delta), np.logical_and(visib_gt, dist_est > 0))
    inter, union = np.logical_and(visib_gt, visib_est), np.logical_or(visib_gt, visib_est)
    n_union = union.sum()
    n_comp = n_union - inter.sum()
    dists = np.abs(dist_gt[inter] - dist_est[inter])
    if normalized_by_diameter:
        dists /= diameter
    if n_union == 0:
        return [1.0] * len(taus)
    return [float((np.sum(dists >= tau) + n_comp) / float(n_union)) for tau in taus]


def _recall_at(per_image, threshold):
    """Greedy matching (decreasing score; an estimate takes the free ground truth of its object with the smallest error
    below the threshold) and recall = matched valid ground truths / valid ground truths."""
    tp = targets = 0
    for gts, ests in per_image:
        targets += sum(1 for g in gts if g["valid"])
        taken = set()
        for e in sorted(ests, key=lambda e: e["score"], reverse=True):
            best, best_err = -1, threshold
            for gid, err in e["errors"].items():
                if gts[gid]["valid"] and gid not in taken and err < best_err:
                    best, best_err = gid, err
            if best >= 0:
                taken.add(best)
        tp += len(taken)
    return tp / targets if targets else 0.0


def _valid_by_visibility(gts, wanted, info, visib_gt_min, where):
    """The toolkit's rule for which ground truths of an image count (eval_calc_scores.py:205-238) -> [bool] per ground truth.  `info`: the
    image's `scene_gt_info.json` entries; only those of target objects are read.  visib_gt_min >= 0: a target whose visib_fract reaches it.
    visib_gt_min < 0: of each target object the inst_count MOST VISIBLE ground truths, equal fractions in ground-truth order (Python's stable
    `sorted(..., reverse=True)`, as the toolkit sorts); this rule needs the targets' instance counts."""
    if info is None or len(info) != len(gts):
        raise ValueError(f"bop_eval: gt_info of image {where} holds {0 if info is None else len(info)} entries for {len(gts)} ground truths")
    mine = [gid for gid, g in enumerate(gts) if wanted is None or g["obj_id"] in wanted]
    if visib_gt_min >= 0:
        ok = {gid for gid in mine if info[gid]["visib_fract"] >= visib_gt_min}
    else:
        if wanted is None:
            raise ValueError("bop_eval: the k-most-visible rule (visib_gt_min < 0) takes k from the targets' inst_count: pass `targets`")
        ok, to_add = set(), dict(wanted)
        for gid in sorted(mine, key=lambda gid: info[gid]["visib_fract"], reverse=True):
            if to_add[gts[gid]["obj_id"]] > 0:
                ok.add(gid)
                to_add[gts[gid]["obj_id"]] -= 1
    return [gid in ok for gid in range(len(gts))]


def _walk(results, scene_gt, cameras, n_top, targets, gt_info=None, visib_gt_min=-1):
    """The images, objects and `n_top` selection both routes score: yields (scene_id, im_id, ground truths with "valid" filled in, K,
    [(obj_id, its estimates, best score first)]).  `targets[(scene_id, im_id)] = {obj_id: inst_count}` (the BOP targets file) limits the
    scoring to these images and objects -- a ground truth of another object is not a target (valid = False) -- and bounds the selection:
    n_top > 0 takes min(n_top, inst_count), n_top = -1 takes inst_count (the toolkit's "given by the number of GT poses"), 0 takes all.
    Without `targets` every image of `scene_gt` is scored and any n_top <= 0 takes all.
    `gt_info[scene_id][im_id]` (the entries of `scene_gt_info.json`, `gt_info.compute_gt_info`) switches "valid" to the toolkit's rule,
    `_valid_by_visibility` with `visib_gt_min`; None keeps every ground truth of a targeted object valid."""
    by_im = {}
    for r in results:
        by_im.setdefault((r["scene_id"], r["im_id"]), []).append(r)
    for sid, ims in scene_gt.items():
        for iid, gts in ims.items():
            wanted = None if targets is None else targets.get((sid, iid))
            if targets is not None and wanted is None:
                continue
            if gt_info is None:
                gts = [dict(g, valid=g.get("valid", True) and (wanted is None or g["obj_id"] in wanted)) for g in gts]
            else:
                ok = _valid_by_visibility(gts, wanted, gt_info.get(sid, {}).get(iid), visib_gt_min, f"{sid}/{iid}")
                gts = [dict(g, valid=g.get("valid", True) and ok[gid]) for gid, g in enumerate(gts)]
            per_obj = {}
            for r in by_im.get((sid, iid), []):
                if wanted is None or r["obj_id"] in wanted:
                    per_obj.setdefault(r["obj_id"], []).append(r)
            picked = []
            for obj_id, rows in per_obj.items():
                top = n_top if n_top > 0 else None
                if wanted is not None:
                    top = min(n_top, wanted[obj_id]) if n_top > 0 else wanted[obj_id] if n_top == -1 else None
                picked.append((obj_id, sorted(rows, key=lambda r: r["score"], reverse=True)[:top]))
            yield sid, iid, gts, np.asarray(cameras[sid][iid], np.float64), picked


def _recall_tables(sets, vsd_sets, do_vsd):
    rec_s = [_recall_at(sets["mssd"], th) for th in MSSD_THRESHOLDS]
    rec_p = [_recall_at(sets["mspd"], th) for th in MSPD_THRESHOLDS]
    ar_s, ar_p = float(np.mean(rec_s)), float(np.mean(rec_p))
    out = dict(AR_MSSD=ar_s, AR_MSPD=ar_p, AR_MSSD_MSPD=0.5 * (ar_s + ar_p), recalls_mssd=rec_s, recalls_mspd=rec_p, AR_VSD=None, AR=None,
               recalls_vsd=None)
    if do_vsd:
        rec_v = [[_recall_at(vsd_sets[ti], th) for th in VSD_THRESHOLDS] for ti in range(len(VSD_TAUS))]
        ar_v = float(np.mean(rec_v))
        out.update(recalls_vsd=rec_v, AR_VSD=ar_v, AR=float(np.mean([ar_v, ar_s, ar_p])))
    return out


def scored_pairs(walk):
    """The (estimate, ground truth) pairs of a `_walk`, grouped as the device route renders them: one unit per (image, object) with
    estimates AND ground truths -> [(scene_id, im_id, K, obj_id, estimates, [(gid, ground truth)])].  A pair's key is
    (scene_id, im_id, obj_id, rank of the estimate among the object's picked ones, gid)."""
    units = []
    for sid, iid, gts, K, picked in walk:
        for obj_id, rows in picked:
            mine = [(gid, g) for gid, g in enumerate(gts) if g["obj_id"] == obj_id]
            if rows and mine:
                units.append((sid, iid, K, obj_id, rows, mine))
    return units


def _cuda_device(device):
    import torch

    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"bop_eval: the device route needs a CUDA device, not {device!r} (leave `device` unset for the host route)")
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def device_pose_errors(units, models, device):
    """`mssd` and `mspd` of every pair of `units` in model units / pixels: one `ops.pose_errors` launch per object.  -> {key: (mssd, mspd)}."""
    from .ops.score import pose_errors

    dev = _cuda_device(device)
    by_obj = {}
    for sid, iid, K, obj_id, rows, mine in units:
        for rank, r in enumerate(rows):
            for gid, g in mine:
                by_obj.setdefault(obj_id, []).append(((sid, iid, obj_id, rank, gid), r, g, K))
    out, pending = {}, []
    for obj_id, pairs in by_obj.items():
        m = models[obj_id]
        pending.append((pairs, pose_errors(m["pts"], m["symmetries"], [p[1]["R"] for p in pairs], [p[1]["t"] for p in pairs], [p[2]["R"] for p in pairs],
                                           [p[2]["t"] for p in pairs], [p[3] for p in pairs], dev)))
    for pairs, (e_s, e_p) in pending:  # read back after everything is queued
        for p, a, b in zip(pairs, e_s.cpu().numpy(), e_p.cpu().numpy()):
            out[p[0]] = (float(a), float(b))
    return out


def device_vsd_counts(units, models, renderer, depth_images, vsd_delta, device, chunk_bytes=DEVICE_CHUNK_BYTES):
    """The integer counts of `vsd` for every pair of `units`, from maps that never leave the device.  Every estimate is rendered once and
    every (image, ground truth) once, each image's test depth is uploaded once, and pairs are processed in chunks whose rendered and
    test maps fit `chunk_bytes`: a chunk is a run of whole (image, object) units, rendered with one `render_batch` per object and side
    and counted with one `ops.vsd_counts` launch per object.  Only a unit that exceeds the budget on its own is split, its ground
    truths rendered again per piece.  -> ({key: int64 array (2 + len(VSD_TAUS),) = n_union, n_inter, count per tau}, number of chunks)."""
    import torch

    from .ops.score import vsd_counts
    from .render import HipDepthRenderer

    dev = _cuda_device(device)
    if not isinstance(renderer, HipDepthRenderer) or _cuda_device(renderer.device) != dev:
        raise RuntimeError(f"bop_eval: VSD on the device route needs a render.HipDepthRenderer on {dev}, not {type(renderer).__name__}"
                           f"{' on ' + str(renderer.device) if isinstance(renderer, HipDepthRenderer) else ''}; there is no fallback to the host route")
    H, W = renderer.H, renderer.W
    budget = min(max(3, int(chunk_bytes) // (4 * H * W)), 65535)  # maps alive at a time: one test image, one ground truth and one estimate at least
    pieces = []
    for unit in units:
        rows, mine = unit[4], unit[5]
        step = len(rows) if 1 + len(mine) + len(rows) <= budget else max(1, budget - 1 - len(mine))
        pieces += [(unit, first, min(first + step, len(rows))) for first in range(0, len(rows), step)]
    chunks, used, images = [], budget + 1, set()
    for piece in pieces:
        (sid, iid, _, _, _, mine), first, last = piece
        need = len(mine) + last - first
        if used + need + ((sid, iid) not in images) > budget:
            chunks.append([])
            used, images = 0, set()
        used += need + ((sid, iid) not in images)
        images.add((sid, iid))
        chunks[-1].append(piece)
    out, on_dev = {}, {}
    for chunk in chunks:
        order = list(dict.fromkeys((p[0][0], p[0][1]) for p in chunk))
        on_dev = {k: v for k, v in on_dev.items() if k in order}  # an image shared with the previous chunk is not uploaded again
        for sid, iid in order:
            if (sid, iid) not in on_dev:
                d = np.ascontiguousarray(np.asarray(depth_images[sid][iid], dtype=np.float32))
                if d.shape != (H, W):
                    raise RuntimeError(f"bop_eval: depth image {sid}/{iid} is {d.shape}, the renderer {(H, W)}")
                on_dev[(sid, iid)] = torch.from_numpy(d).to(dev)
        test = on_dev[order[0]][None] if len(order) == 1 else torch.stack([on_dev[k] for k in order])
        by_obj = {}
        for piece in chunk:
            by_obj.setdefault(piece[0][3], []).append(piece)
        pending = []
        for obj_id, group in by_obj.items():
            est, gt, gt_at, keys, index, K4, diam = [], [], {}, [], [], [], models[obj_id]["diameter"]
            for (sid, iid, K, _, rows, mine), first, last in group:
                k4 = [K[0, 0], K[1, 1], K[0, 2], K[1, 2]]
                for gid, g in mine:
                    if (sid, iid, gid) not in gt_at:
                        gt_at[(sid, iid, gid)] = len(gt)
                        gt.append((g["R"], g["t"], k4))
                for rank in range(first, last):
                    est.append((rows[rank]["R"], rows[rank]["t"], k4))
                    for gid, _ in mine:
                        keys.append((sid, iid, obj_id, rank, gid))
                        index.append((order.index((sid, iid)), gt_at[(sid, iid, gid)], len(est) - 1))
                        K4.append(k4)
            d_gt = renderer.render_batch(obj_id, np.stack([p[0] for p in gt]), np.stack([p[1] for p in gt]), np.asarray([p[2] for p in gt]))
            d_est = renderer.render_batch(obj_id, np.stack([p[0] for p in est]), np.stack([p[1] for p in est]), np.asarray([p[2] for p in est]))
            index, K4 = np.asarray(index), np.asarray(K4)
            for a in range(0, len(keys), 65535):  # the launch limit of pairs
                b = slice(a, a + 65535)
                pending.append((keys[b], vsd_counts(test, d_gt, d_est, K4[b], vsd_delta, diam, VSD_TAUS, index[b, 0], index[b, 1], index[b, 2])))
        for keys, counts in pending:  # one read-back per chunk, after its launches are queued; the maps are released with the chunk
            out.update(zip(keys, counts.cpu().numpy()))
    return out, len(chunks)


def _host_errors(walk, models, im_width, renderer, depth_images, vsd_delta):
    """The host route: errors of every scored pair with numpy, one estimate at a time -> {key: (mssd / diameter, mspd at 640 px width, VSD
    error per tau or None)}, keys as `scored_pairs` documents them.  Every estimate is rendered once, every (image, ground truth) once."""
    out, gt_depth = {}, {}
    for sid, iid, gts, K, picked in walk:
        for obj_id, rows in picked:
            m = models[obj_id]
            for rank, r in enumerate(rows):
                d_est = renderer.render_object(obj_id, r["R"], r["t"], K[0, 0], K[1, 1], K[0, 2], K[1, 2])["depth"] if renderer is not None else None
                for gid, g in enumerate(gts):
                    if g["obj_id"] != obj_id:
                        continue
                    Rg, tg = np.asarray(g["R"], np.float64), np.asarray(g["t"], np.float64)
                    e1 = mssd(r["R"], r["t"], Rg, tg, m["pts"], m["symmetries"]) / m["diameter"]
                    e2 = mspd(r["R"], r["t"], Rg, tg, K, m["pts"], m["symmetries"]) * (640.0 / im_width)
                    e3 = None
                    if renderer is not None:
                        key = (sid, iid, gid)
                        if key not in gt_depth:
                            gt_depth[key] = renderer.render_object(obj_id, Rg, tg, K[0, 0], K[1, 1], K[0, 2], K[1, 2])["depth"]
                        e3 = vsd(d_est, gt_depth[key], depth_images[sid][iid], K, vsd_delta, VSD_TAUS, m["diameter"])
                    out[(sid, iid, obj_id, rank, gid)] = (e1, e2, e3)
    return out


def _device_errors(walk, models, im_width, renderer, depth_images, vsd_delta, device, chunk_bytes):
    """Errors of every scored pair as the host loop forms them: {key: (mssd / diameter, mspd at 640 px width, VSD error per tau or None)}.
    The VSD error comes from the integer counts exactly as in `vsd`: (count + n_union - n_inter) / n_union, 1.0 for an empty union."""
    units = scored_pairs(walk)
    if not units:
        return {}
    dist = device_pose_errors(units, models, device)
    counts = device_vsd_counts(units, models, renderer, depth_images, vsd_delta, device, chunk_bytes)[0] if renderer is not None else None
    out = {}
    for key, (e_s, e_p) in dist.items():
        e_v = None
        if counts is not None:
            n_union, n_inter, *per_tau = (int(c) for c in counts[key])
            e_v = [1.0] * len(per_tau) if n_union == 0 else [float((c + (n_union - n_inter)) / float(n_union)) for c in per_tau]
        out[key] = (e_s / models[key[2]]["diameter"], e_p * (640.0 / im_width), e_v)
    return out


def further_errors(walk, models, types, symmetric_obj_ids, n_top, device, targets, legacy):
    """The `out["errors"]` blocks of `average_recall` for `types`.  `legacy` {"mssd" / "mspd": per-image sets, "vsd": one per tau or None}:
    the BOP'19 errors already computed, tabulated per object too when `types` names them."""
    symmetric = set(symmetric_obj_ids)
    obj_ids = sorted(models)
    pairs = metric_pairs(walk, models, types, symmetric)
    values = host_pose_metrics(pairs, models) if device is None else device_pose_metrics(pairs, models, device)
    apart = {p["key"]: p["apart"] for p in pairs}
    if targets is not None:
        weights = {}
        for objs in targets.values():
            for o, c in objs.items():
                weights[o] = weights.get(o, 0) + c
    else:
        weights = {}
        for _, _, gts, _, _ in walk:
            for g in gts:
                weights[g["obj_id"]] = weights.get(g["obj_id"], 0) + bool(g["valid"])

    def listed(per_image):
        return [(gts, [dict(score=e["score"], errors={gid: [v] for gid, v in e["errors"].items()}) for e in ests]) for gts, ests in per_image]

    out = {}
    for T in types:
        if T == "vsd":
            if legacy["vsd"] is None:
                continue
            tabs = [[localization_scores(listed(per_tau), [th], obj_ids, n_top) for th in VSD_THRESHOLDS] for per_tau in legacy["vsd"]]
            flat = _error_block(None, [t for row in tabs for t in row], weights)
            nt = len(VSD_THRESHOLDS)
            out[T] = dict(flat, thresholds=dict(taus=[float(t) for t in VSD_TAUS], correct_th=[[float(t)] for t in VSD_THRESHOLDS]),
                          recalls=[[t[0] for t in row] for row in tabs],
                          obj_recalls={o: [v[i * nt:(i + 1) * nt] for i in range(len(tabs))] for o, v in flat["obj_recalls"].items()})
        elif T in ("mssd", "mspd"):
            ths = MSSD_THRESHOLDS if T == "mssd" else MSPD_THRESHOLDS
            out[T] = _error_block([[float(t)] for t in ths], [localization_scores(listed(legacy[T]), [th], obj_ids, n_top) for th in ths], weights)
        else:
            per_image = []
            for sid, iid, gts, K, picked in walk:
                ests = []
                for obj_id, rows in picked:
                    for rank, r in enumerate(rows):
                        errs = {}
                        for gid, g in enumerate(gts):
                            key = (sid, iid, obj_id, rank, gid)
                            if g["obj_id"] == obj_id:
                                errs[gid] = pair_error(T, values[key], models[obj_id]["diameter"], obj_id in symmetric, apart[key])
                        ests.append(dict(score=r["score"], errors=errs))
                per_image.append((gts, ests))
            ths = ERROR_TYPES[T]["thresholds"]
            out[T] = _error_block([list(th) for th in ths], [localization_scores(per_image, th, obj_ids, n_top) for th in ths], None)
    return out


def average_recall(results, scene_gt, models, cameras, im_width, n_top=1, renderer=None, depth_images=None, vsd_delta=VSD_DELTA, device=None,
                   targets=None, chunk_bytes=DEVICE_CHUNK_BYTES, error_types=DEFAULT_ERROR_TYPES, symmetric_obj_ids=None, gt_info=None,
                   visib_gt_min=-1):
    """results: `read_results` rows; scene_gt[scene_id][im_id] = list of {"obj_id", "R" (3,3), "t" (3,) mm, optional "valid"};
    models[obj_id] = {"pts" (n,3) mm, "diameter", "symmetries": [{"R","t"}] incl. identity}; cameras[scene_id][im_id] = K.
    Only the `n_top` best-scored estimates per (image, object) take part (BOP: the instance count of the target; `targets`: see `_walk`).
    With `renderer` (render_object(obj_id, R, t, fx, fy, cx, cy) -> {"depth"}) and depth_images[scene_id][im_id] (mm, (H,W)) the VSD
    errors are computed too and "AR" = mean(AR_VSD, AR_MSSD, AR_MSPD) is the BOP'19 average recall; else AR_VSD = AR = None.
    Without `device` the errors come from `_host_errors` (numpy); a CUDA `device` selects `_device_errors`: same walk, same matching, the errors from csrc/bopscore.hip; VSD
    then needs a `render.HipDepthRenderer` of the image size on that device, and at most `chunk_bytes` of rendered maps exist at a time.
    The device route reads the test depth as float32, which is what `load_dataset` and the toolkit's `load_depth` return.
    -> {"AR_VSD", "AR_MSSD", "AR_MSPD", "AR", "AR_MSSD_MSPD", "recalls_vsd" [tau][threshold], "recalls_mssd", "recalls_mspd"}.
    `error_types` (`parse_error_types`: names of KNOWN_ERROR_TYPES, a list or a comma-separated string): with the default the result is the
    dictionary above.  Otherwise nothing is rendered unless "vsd" is named (AR_VSD = AR = None), and every named type T adds the block
    below.  MSSD and MSPD are computed whatever `error_types` names, on purpose: they need no renderer, cost one launch per object beside
    the further errors' (tens of microseconds per call), and with them "AR_MSSD", "AR_MSPD", "recalls_mssd" and "recalls_mspd" mean the
    same in every scores file and on `--eval`'s AR line; VSD is the expensive one, and the only one left out.  The block:
    out["errors"][T] = {"thresholds", "recalls" (per threshold, what `score.calc_localization_scores` calls "recall"), "mean_recall" (the
    script's "average recall"), "obj_recalls" {obj_id: [per threshold]}, "mean_obj_recall" (mean over the objects of their mean recall;
    for vsd / mssd / mspd weighted by the targets' instance counts)}; for "vsd" the lists are [tau][threshold].  The host route computes
    them with this module's functions, the device route with `ops.pose_metrics` / `ops.adi`.  `symmetric_obj_ids`: the objects that take
    ADI under ad / ABSad / AUCad (default `default_symmetric_obj_ids(models)`); the ids used are returned as out["symmetric_obj_ids"].
    `gt_info` / `visib_gt_min`: which ground truths count follows the toolkit's visibility rule (`_walk`, `_valid_by_visibility`) instead of
    "every ground truth of a targeted object"; the matching, the recalls and every block of out["errors"] see the same flags."""
    types = parse_error_types(error_types)
    do_vsd = renderer is not None and depth_images is not None and "vsd" in types
    if device is not None:
        _cuda_device(device)
    walk = list(_walk(results, scene_gt, cameras, n_top, targets, gt_info, visib_gt_min))
    if device is None:
        errors = _host_errors(walk, models, im_width, renderer if do_vsd else None, depth_images, vsd_delta)
    else:
        errors = _device_errors(walk, models, im_width, renderer if do_vsd else None, depth_images, vsd_delta, device, chunk_bytes)
    sets = {"mssd": [], "mspd": []}
    vsd_sets = [[] for _ in VSD_TAUS]
    for sid, iid, gts, K, picked in walk:
        ests = {"mssd": [], "mspd": []}
        vests = [[] for _ in VSD_TAUS]
        for obj_id, rows in picked:
            for rank, r in enumerate(rows):
                mine = {gid: errors[(sid, iid, obj_id, rank, gid)] for gid, g in enumerate(gts) if g["obj_id"] == obj_id}
                ests["mssd"].append(dict(score=r["score"], errors={gid: e[0] for gid, e in mine.items()}))
                ests["mspd"].append(dict(score=r["score"], errors={gid: e[1] for gid, e in mine.items()}))
                for ti in range(len(VSD_TAUS)):
                    vests[ti].append(dict(score=r["score"], errors={gid: e[2][ti] for gid, e in mine.items()} if do_vsd else {}))
        for k in sets:
            sets[k].append((gts, ests[k]))
        for ti in range(len(VSD_TAUS)):
            vsd_sets[ti].append((gts, vests[ti]))
    out = _recall_tables(sets, vsd_sets, do_vsd)
    if types != DEFAULT_ERROR_TYPES:
        sym_ids = default_symmetric_obj_ids(models) if symmetric_obj_ids is None else sorted(int(o) for o in symmetric_obj_ids)
        out["errors"] = further_errors(walk, models, types, sym_ids, n_top, device, targets, dict(sets, vsd=vsd_sets if do_vsd else None))
        out["symmetric_obj_ids"] = sym_ids
    return out


# ---- reading a BOP dataset folder for scoring ----------------------------------------------------------------------------------
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def read_ply(path):
    """A PLY mesh, ASCII or binary_little_endian, with scalar vertex properties (x, y, z among them) and triangular faces (one list
    property, `vertex_indices` / `vertex_index`) -> {"pts" (V,3) float64, "faces" (F,3) int32}.  Elements other than vertex and face may
    follow them and are not read; anything else in the file is an error, not a guess."""
    return _read_ply(path, False)


def read_ply_colors(path):
    """`read_ply` plus "colors": the vertex properties `red`, `green`, `blue` as (V,3) float64 in [0, 1] -- an integer property divided by
    its type's largest value (uchar: 255, as the toolkit's renderers do), a floating-point one clipped to [0, 1] -- or None where the
    file has no such properties (BOP's models_eval meshes carry none)."""
    return _read_ply(path, True)


def read_ply_model(path):
    """`read_ply_colors` plus what a renderer of the model needs: "normals" (V,3) float64 from the vertex properties `nx, ny, nz`,
    "texture_uv" (V,2) float64 from `texture_u, texture_v` (None without them) and "texture_file", the NAME of the header's
    `comment TextureFile NAME` line (None without one; the image lies beside the PLY).  Texture coordinates per FACE (a `texcoord` list
    property of the face element) are an error: a vertex would need one pair per face it belongs to, and nothing here guesses one.
    A file without normals gets `vertex_normals(pts, faces)`.  That is this project's rule -- the toolkit's renderers refuse to shade
    such a model smoothly -- and "normals_computed" says which of the two happened."""
    out = _read_ply(path, True, True)
    out["normals_computed"] = out["normals"] is None
    if out["normals_computed"]:
        out["normals"] = vertex_normals(out["pts"], out["faces"])
    return out


def vertex_normals(pts, faces):
    """Area-weighted vertex normals (V,3) float64: every face adds the cross product of its edges (its normal times twice its area) to its
    three vertices, and the sums are brought to unit length.  A vertex that no face with an area touches keeps the zero vector."""
    pts, faces = np.asarray(pts, np.float64), np.asarray(faces).reshape(-1, 3)
    n = np.zeros_like(pts)
    cross = np.cross(pts[faces[:, 1]] - pts[faces[:, 0]], pts[faces[:, 2]] - pts[faces[:, 0]])
    for k in range(3):
        np.add.at(n, faces[:, k], cross)
    length = np.linalg.norm(n, axis=1, keepdims=True)
    return np.divide(n, length, out=np.zeros_like(n), where=length > 0)


def _read_ply(path, with_colors, with_model=False):
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    body = data.find(b"\n", end) + 1
    fmt, elements, texture_file = None, [], None
    for line in data[:end].decode("latin-1").splitlines():
        w = line.split()
        if len(w) >= 3 and w[:2] == ["comment", "TextureFile"]:
            texture_file = w[-1]
        if not w or w[0] in ("ply", "comment", "obj_info"):
            continue
        if w[0] == "format":
            fmt = w[1]
        elif w[0] == "element":
            elements.append((w[1], int(w[2]), []))
        elif w[0] == "property" and elements:
            elements[-1][2].append(tuple(w[1:]))
        else:
            raise ValueError(f"{path}: header line {line!r}")
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"{path}: PLY format {fmt!r} (ascii and binary_little_endian are read)")
    out = {"faces": np.zeros((0, 3), np.int32)}
    tokens, at = (data[body:].split(), 0) if fmt == "ascii" else (None, body)
    for name, count, props in elements:
        if name not in ("vertex", "face"):
            if "pts" not in out:
                raise ValueError(f"{path}: element {name!r} before the vertices")
            break
        lists = [p for p in props if p[0] == "list"]
        unknown = [t for p in props for t in (p[1:3] if p[0] == "list" else p[:1]) if t not in _PLY_TYPES]
        if unknown or any(len(p) != (4 if p[0] == "list" else 2) for p in props):
            raise ValueError(f"{path}: {name} properties {props}")
        if name == "vertex":
            if lists or not {"x", "y", "z"} <= {p[1] for p in props}:
                raise ValueError(f"{path}: vertex properties {props}")
            dtype = np.dtype([(p[1], "<" + _PLY_TYPES[p[0]]) for p in props])
        else:
            if with_model and any(p[0] == "list" and p[3] == "texcoord" for p in props):
                raise ValueError(f"{path}: texture coordinates per face (the `texcoord` list property) are not read: "
                                 "save the model with per-vertex `texture_u`, `texture_v`")
            if len(props) != 1 or not lists or props[0][3] not in ("vertex_indices", "vertex_index"):
                raise ValueError(f"{path}: face properties {props} (one list of vertex indices is read)")
            dtype = np.dtype([("n", "<" + _PLY_TYPES[props[0][1]]), ("v", "<" + _PLY_TYPES[props[0][2]], (3,))])
        if fmt == "ascii":
            width = len(props) if name == "vertex" else 4
            rows = np.array(tokens[at:at + count * width], dtype=np.float64).reshape(count, width)
            if name == "face" and count and (rows[:, 0] != 3).any():
                raise ValueError(f"{path}: a face that is not a triangle")  # rows of another length also misalign the reshape above
            at += count * width
            rec = {p[1]: rows[:, i] for i, p in enumerate(props)} if name == "vertex" else {"v": rows[:, 1:]}
        else:
            if at + count * dtype.itemsize > len(data):
                raise ValueError(f"{path}: truncated {name} data")
            rec = np.frombuffer(data, dtype=dtype, count=count, offset=at)
            at += count * dtype.itemsize
            if name == "face" and count and (rec["n"] != 3).any():
                raise ValueError(f"{path}: a face that is not a triangle")
        if name == "vertex":
            out["pts"] = np.stack([np.asarray(rec[k], np.float64) for k in "xyz"], axis=1)
            if with_colors:
                kinds = {p[1]: np.dtype(_PLY_TYPES[p[0]]) for p in props}
                out["colors"] = None
                if {"red", "green", "blue"} <= set(kinds):
                    chans = [np.asarray(rec[k], np.float64) / (np.iinfo(kinds[k]).max if kinds[k].kind in "iu" else 1.0) for k in ("red", "green", "blue")]
                    out["colors"] = np.clip(np.stack(chans, axis=1), 0.0, 1.0)
            if with_model:
                names = {p[1] for p in props}
                for key, wanted in (("normals", ("nx", "ny", "nz")), ("texture_uv", ("texture_u", "texture_v"))):
                    out[key] = np.stack([np.asarray(rec[k], np.float64) for k in wanted], axis=1) if set(wanted) <= names else None
                out["texture_file"] = texture_file
        else:
            out["faces"] = np.asarray(rec["v"]).astype(np.int32).reshape(count, 3)
    if "pts" not in out:
        raise ValueError(f"{path}: no vertex element")
    if len(out["faces"]) and (out["faces"].min() < 0 or out["faces"].max() >= len(out["pts"])):
        raise ValueError(f"{path}: face index outside the {len(out['pts'])} vertices")
    return out


def _axis_rotation(angle, axis):
    d = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    skew = np.array([[0.0, -d[2], d[1]], [d[2], 0.0, -d[0]], [-d[1], d[0], 0.0]])
    return np.cos(angle) * np.eye(3) + (1.0 - np.cos(angle)) * np.outer(d, d) + np.sin(angle) * skew


def symmetry_transformations(model_info, max_sym_disc_step=MAX_SYM_DISC_STEP):
    """The toolkit's `misc.get_symmetry_transformations` (misc.py:44-91): the identity and `symmetries_discrete`, each combined with
    every step of every `symmetries_continuous` axis discretised into ceil(pi / max_sym_disc_step) rotations -> [{"R" (3,3), "t" (3,)}],
    identity first."""
    disc = [dict(R=np.eye(3), t=np.zeros(3))]
    for sym in model_info.get("symmetries_discrete", []):
        m = np.reshape(np.asarray(sym, np.float64), (4, 4))
        disc.append(dict(R=m[:3, :3], t=m[:3, 3]))
    cont = []
    for sym in model_info.get("symmetries_continuous", []):
        offset = np.asarray(sym["offset"], np.float64).reshape(3)
        steps = int(np.ceil(np.pi / max_sym_disc_step))
        for i in range(steps):
            R = _axis_rotation(i * (2.0 * np.pi / steps), sym["axis"])
            cont.append(dict(R=R, t=-R.dot(offset) + offset))
    if not cont:
        return disc
    return [dict(R=c["R"].dot(d["R"]), t=c["R"].dot(d["t"]) + c["t"]) for d in disc for c in cont]


class _SceneDepth:
    def __init__(self, owner, scene_id):
        self.owner, self.scene_id = owner, scene_id

    def __getitem__(self, im_id):
        return self.owner.image(self.scene_id, im_id)


class DepthImages:
    """depth_images[scene_id][im_id] -> the test depth in mm (float32, file value x depth_scale as the toolkit's `load_depth` then
    `*= depth_scale`), read when asked for and kept behind `provider.SceneFiles`' LRU rule."""

    def __init__(self, folder, depth_scales, max_images=16):
        from collections import OrderedDict

        self.folder, self.depth_scales, self.max_images, self._store = folder, depth_scales, max_images, OrderedDict()

    def __getitem__(self, scene_id):
        return _SceneDepth(self, scene_id)

    def image(self, scene_id, im_id):
        from .provider import SceneFiles, read_image

        def make():
            base = osp.join(self.folder, f"{scene_id:06d}", "depth", f"{im_id:06d}")
            d = read_image(base + ".png" if osp.exists(base + ".png") else base + ".tif").astype(np.float32)
            d *= self.depth_scales[scene_id][im_id]
            return d

        return SceneFiles._lru(self._store, (scene_id, im_id), self.max_images, make)


def dataset_paths(root, name, split, targets_filename="test_targets_bop19.json"):
    """The files and folders `load_dataset` reads."""
    base = osp.join(root, name)
    return dict(targets=osp.join(base, targets_filename), models_info=osp.join(base, "models_eval", "models_info.json"),
                models=osp.join(base, "models_eval"), split=osp.join(base, split))


MODELS_INFO_MODES = ("file", "compute")


def _models_info_mode(mode):
    if mode not in MODELS_INFO_MODES:
        raise ValueError(f"bop_eval: models_info {mode!r} (file or compute)")
    return mode


def load_dataset(root, name, split, targets_filename="test_targets_bop19.json", gt_info=False, models_info="file", device=None):
    """What `average_recall` needs of the BOP dataset `<root>/<name>`, for the images and objects of the targets file:
    models[obj_id] = {"pts", "verts", "faces", "diameter", "symmetries"} from models_eval/obj_XXXXXX.ply + models_info.json;
    scene_gt / cameras / depth_scales[scene_id][im_id] from <split>/<scene>/scene_gt.json and scene_camera.json; depth_images: a lazy
    `DepthImages`; targets[(scene_id, im_id)] = {obj_id: inst_count}; im_size = (W, H) of the first target's depth image.
    gt_info=True adds "gt_info"[scene_id][im_id] from <split>/<scene>/scene_gt_info.json; a scene without the file is an error.
    models_info="compute": the diameters are not read but computed from the targeted objects' vertices (`model_info.compute_models_info`: on
    the CUDA `device`, on the host without one -- equal bits), so a dataset without models_info.json can be scored; the symmetries still come
    from the file where it exists (they are annotations), else every object has the identity only."""
    from .provider import SceneFiles, load_json

    _models_info_mode(models_info)
    paths = dataset_paths(root, name, split, targets_filename)
    targets = {}
    for t in load_json(paths["targets"]):
        targets.setdefault((int(t["scene_id"]), int(t["im_id"])), {})[int(t["obj_id"])] = int(t.get("inst_count", 1))
    info = load_json(paths["models_info"]) if models_info == "file" or osp.exists(paths["models_info"]) else {}
    meshes = {obj_id: read_ply(osp.join(paths["models"], f"obj_{obj_id:06d}.ply")) for obj_id in sorted({o for objs in targets.values() for o in objs})}
    if models_info == "compute":
        from .model_info import compute_models_info

        diameters = {o: e["diameter"] for o, e in compute_models_info({o: m["pts"] for o, m in meshes.items()}, device=device).items()}
    else:
        diameters = {o: float(info[str(o)]["diameter"]) for o in meshes}
    models = {}
    for obj_id, mesh in meshes.items():
        models[obj_id] = dict(pts=mesh["pts"], verts=mesh["pts"], faces=mesh["faces"], diameter=diameters[obj_id],
                              symmetries=symmetry_transformations(info.get(str(obj_id), {})))
    files = SceneFiles()
    scene_gt, cameras, depth_scales = {}, {}, {}
    for sid, iid in targets:
        gts = files.scene_json(paths["split"], sid, "scene_gt.json")[str(iid)]
        scene_gt.setdefault(sid, {})[iid] = [dict(obj_id=int(g["obj_id"]), R=np.asarray(g["cam_R_m2c"], np.float64).reshape(3, 3),
                                                  t=np.asarray(g["cam_t_m2c"], np.float64).reshape(3)) for g in gts]
        K, scale = files.camera(paths["split"], sid, iid)
        cameras.setdefault(sid, {})[iid] = np.asarray(K, np.float64)
        depth_scales.setdefault(sid, {})[iid] = float(scale)
    depth_images = DepthImages(paths["split"], depth_scales)
    im_size = None
    if targets:
        sid, iid = next(iter(targets))
        im_size = depth_images[sid][iid].shape[::-1]
    out = dict(models=models, scene_gt=scene_gt, cameras=cameras, depth_scales=depth_scales, depth_images=depth_images, targets=targets,
               im_size=im_size)
    if gt_info:
        from .gt_info import load_gt_info

        out["gt_info"] = load_gt_info(root, name, split, sorted(scene_gt))
    return out


def _computed_gt_info(data, delta, dev, on_device, chunk_bytes):
    """`score_csv(gt_visibility="compute")`: `gt_info.compute_gt_info` for the ground truths of the targeted objects in the scored images (the
    others are never valid and `load_dataset` holds no model of theirs: their entries are None) -> gt_info[scene_id][im_id]."""
    from .gt_info import compute_gt_info
    from .render import HipDepthRenderer

    W, H = data["im_size"]
    canvas = HipDepthRenderer(3 * W, 3 * H, device=dev)
    for obj_id, m in data["models"].items():
        canvas.add_object(obj_id, m["verts"], m["faces"])
    keep = {sid: {iid: [gid for gid, g in enumerate(gts) if g["obj_id"] in data["targets"][(sid, iid)]] for iid, gts in ims.items()}
            for sid, ims in data["scene_gt"].items()}
    part = {sid: {iid: [data["scene_gt"][sid][iid][gid] for gid in gids] for iid, gids in ims.items()} for sid, ims in keep.items()}
    info = compute_gt_info(part, data["cameras"], data["depth_images"], canvas, delta, device=dev if on_device else None, chunk_bytes=chunk_bytes)
    out = {}
    for sid, ims in keep.items():
        for iid, gids in ims.items():
            row = [None] * len(data["scene_gt"][sid][iid])
            for gid, entry in zip(gids, info[sid][iid]):
                row[gid] = entry
            out.setdefault(sid, {})[iid] = row
    return out


def score_csv(csv_path, root, name, split, device="cuda", device_scoring=True, n_top=-1, vsd_delta=None,
              targets_filename="test_targets_bop19.json", renderer=None, chunk_bytes=DEVICE_CHUNK_BYTES, error_types=None, symmetric_obj_ids=None,
              gt_visibility="off", visib_gt_min=-1, gt_delta=None, models_info=None):
    """Score the result file `csv_path` against the BOP dataset `<root>/<name>` and write `scores_bop19.json` beside it: the AR values
    and recall tables of `average_recall`, the number of scored targets ((image, object) entries of the targets file) and estimates,
    and the settings.  `device`: the GPU that renders (`render.HipDepthRenderer`, unless a `renderer` is handed in) and, with
    `device_scoring`, computes the errors; device_scoring=False is the host scorer on the same renders.  n_top as in `_walk` (-1: the
    targets' instance counts); vsd_delta defaults to the dataset's (15 mm, ITODD 5 mm).  `error_types` / `symmetric_obj_ids` as in
    `average_recall` (None: the BOP'19 three): the file then also holds "errors", "error_types" and "symmetric_obj_ids", and no renderer
    is built unless "vsd" is among the types.
    `gt_visibility`: "off" -- every ground truth of a targeted object counts; "file" -- the toolkit's rule (`_valid_by_visibility` with
    `visib_gt_min`) on the dataset's `scene_gt_info.json`, an error where the file is missing; "compute" -- the same rule on
    `gt_info.compute_gt_info` for the targeted objects' ground truths in the scored images on the scoring device (on the host from HIP
    renders with device_scoring=False), with the visibility tolerance `gt_delta` in mm: by default the dataset's (15, ITODD 5), which is what
    `write_gt_info` and BOP's own files use -- NOT `vsd_delta`, which belongs to the VSD error; pass the `delta` a dataset's files were written
    with to compute what they hold.  `visib_gt_min` under "off" and `gt_delta` without "compute" are errors.  The file then holds
    "gt_visibility" and "visib_gt_min", under "compute" also "gt_delta".
    `models_info`: None or "file" -- the diameters of models_eval/models_info.json; "compute" -- the diameters computed from the models_eval
    vertices of the targeted objects (`load_dataset`), on the scoring device or, with device_scoring=False, on the host: a dataset without the
    file can be scored.  The file holds "models_info" only when the option is given.
    -> the dictionary written."""
    types = parse_error_types(error_types)
    if models_info is not None:
        _models_info_mode(models_info)
    if gt_visibility not in ("off", "file", "compute"):
        raise ValueError(f"bop_eval: gt_visibility {gt_visibility!r} (off, file or compute)")
    if gt_visibility == "off" and visib_gt_min != -1:
        raise ValueError("bop_eval: visib_gt_min has no effect with gt_visibility=\"off\" (file or compute)")
    if gt_delta is not None and gt_visibility != "compute":
        raise ValueError("bop_eval: gt_delta is the visibility tolerance of gt_visibility=\"compute\"")
    gt_delta = VSD_DELTAS.get(name, VSD_DELTA) if gt_delta is None else gt_delta
    data = load_dataset(root, name, split, targets_filename, gt_info=gt_visibility == "file", models_info=models_info or "file",
                        device=_cuda_device(device) if device_scoring and models_info == "compute" else None)
    results = read_results(csv_path)
    vsd_delta = VSD_DELTAS.get(name, VSD_DELTA) if vsd_delta is None else vsd_delta
    W, H = data["im_size"]
    if renderer is None and "vsd" in types:
        from .render import HipDepthRenderer

        renderer = HipDepthRenderer(W, H, device=_cuda_device(device))
    if renderer is not None:
        for obj_id, m in data["models"].items():
            renderer.add_object(obj_id, m["verts"], m["faces"])
    gt_info = data.get("gt_info")
    if gt_visibility == "compute":
        gt_info = _computed_gt_info(data, gt_delta, _cuda_device(device), device_scoring, chunk_bytes)
    out = average_recall(results, data["scene_gt"], data["models"], data["cameras"], W, n_top=n_top, renderer=renderer,
                         depth_images=data["depth_images"], vsd_delta=vsd_delta, device=device if device_scoring else None,
                         targets=data["targets"], chunk_bytes=chunk_bytes, error_types=types, symmetric_obj_ids=symmetric_obj_ids,
                         gt_info=gt_info, visib_gt_min=visib_gt_min)
    if gt_visibility != "off":
        out.update(gt_visibility=gt_visibility, visib_gt_min=visib_gt_min, **(dict(gt_delta=float(gt_delta)) if gt_visibility == "compute" else {}))
    if models_info is not None:
        out.update(models_info=models_info)
    if "errors" in out:
        out["error_types"] = list(types)
    scored = sum(len(rows) for *_, picked in _walk(results, data["scene_gt"], data["cameras"], n_top, data["targets"]) for _, rows in picked)  # not a matter of validity
    out.update(n_targets=sum(len(objs) for objs in data["targets"].values()), n_estimates=len(results), n_scored_estimates=scored, dataset=name,
               split=split, n_top=n_top, vsd_delta=float(vsd_delta), scorer="device" if device_scoring else "host")
    with open(osp.join(osp.dirname(osp.abspath(csv_path)), "scores_bop19.json"), "w") as f:
        json.dump(out, f, indent=1)
    return out
