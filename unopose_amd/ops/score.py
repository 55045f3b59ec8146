"""Pose errors of the BOP'19 scorer on the device (csrc/bopscore.hip): the integer counts inside `bop_eval.vsd` and the
`bop_eval.mssd` / `mspd` errors, for many (estimate, ground truth) pairs per launch, and the further errors of csrc/posemetrics.hip:
`pose_metrics` (add, proj, re, te and the symmetry-aware projS, reS, teS) and `adi`; `gt_visibility` (csrc/gtinfo.hip) is the
ground-truth side, the integers behind `scene_gt_info.json` and the two masks; `pts_extent` (csrc/modelinfo.hip) the model side, the box
and the diameter behind `models_info.json`; `ref_select` (csrc/reftargets.hip) the reference-view search behind the one-reference target list
(`ref_targets.select_host`, equal bits); `sym_deviation` (csrc/symmetry.hip) the Hausdorff deviation of a model under candidate
symmetries (`model_sym.sym_deviation_host`, equal bits).  `bop_eval`'s and `gt_info`'s host functions are the
specification: the counts equal numpy's, the distances and means agree with the BLAS-backed host code to rounding.

The kernels trust the map indices they are given: the wrappers check every index against the map stacks on the host BEFORE
anything is launched.  Depth maps are CUDA tensors; the small per-pair tables are host arrays; there is no CPU path."""
import ctypes
import functools

import numpy as np
import torch

from .._lib import call, lib, on_device, ptr, stream_ptr

MAX_TAUS = 16


@functools.lru_cache(maxsize=None)
def _count_ints():
    return int(lib().unopose_vsd_count_ints())


def _maps(x, name, hw=None):
    if not torch.is_tensor(x) or not x.is_cuda:
        raise RuntimeError(f"{name}: CPU not supported")
    if x.dtype != torch.float32 or not x.is_contiguous() or x.dim() != 3 or x.shape[0] < 1:
        raise RuntimeError(f"{name} must be a contiguous float32 tensor (maps, H, W), not {x.dtype} {tuple(x.shape)}")
    if hw is not None and tuple(x.shape[1:]) != tuple(hw):
        raise RuntimeError(f"{name}: maps of {tuple(x.shape[1:])}, expected {tuple(hw)}")
    return x


def _index(idx, P, limit, name, op="vsd_counts"):
    idx = np.arange(P, dtype=np.int64) if idx is None else np.asarray(idx, dtype=np.int64).reshape(-1)
    if idx.shape[0] != P or idx.min() < 0 or idx.max() >= limit:
        raise ValueError(f"{op}: {name} must hold {P} indices inside [0, {limit})")
    return idx


def vsd_delta_as_compared(delta):
    """`_visib_mask` compares a float32 difference with `delta`: numpy does that in float32 for a Python number and in float64 for
    a float64 array scalar.  The kernel compares in float64, with `delta` rounded the way numpy would have."""
    return float(np.result_type(np.float32, delta).type(delta))


def vsd_counts(depth_test, depth_gt, depth_est, K4, delta, diameter, taus, image_index=None, gt_index=None, est_index=None):
    """The counts of `bop_eval.vsd` for P pairs over one image size.  depth_test (n_test, H, W), depth_gt (n_gt, H, W), depth_est
    (n_est, H, W): float32 CUDA maps in mm, the rendered ones straight from `HipDepthRenderer.render_batch`; pair p scores
    depth_est[est_index[p]] against depth_gt[gt_index[p]] in front of depth_test[image_index[p]] (each index defaults to p).  K4 (P, 4) or
    (4,) = fx, fy, cx, cy; delta, diameter: scalars or (P,); taus: T <= 16 tolerances.
    -> int64 CUDA tensor (P, 2 + T): n_union, n_inter, then per tau the intersection pixels with |dist_gt - dist_est| / diameter >= tau."""
    _maps(depth_test, "vsd_counts: depth_test")
    hw = tuple(depth_test.shape[1:])
    _maps(depth_gt, "vsd_counts: depth_gt", hw), _maps(depth_est, "vsd_counts: depth_est", hw)
    dev = depth_test.device
    if depth_gt.device != dev or depth_est.device != dev:
        raise RuntimeError("vsd_counts: the maps live on different devices")
    taus = np.ascontiguousarray(np.asarray(taus, dtype=np.float64).reshape(-1))
    T = taus.shape[0]
    if not 1 <= T <= MAX_TAUS:
        raise ValueError(f"vsd_counts: {T} taus (1 .. {MAX_TAUS})")
    P = len(est_index) if est_index is not None else len(gt_index) if gt_index is not None else int(depth_est.shape[0])
    if not 1 <= P <= 65535:
        raise ValueError(f"vsd_counts: {P} pairs per call (1 .. 65535)")
    index = np.stack([_index(image_index, P, depth_test.shape[0], "image_index"), _index(gt_index, P, depth_gt.shape[0], "gt_index"),
                      _index(est_index, P, depth_est.shape[0], "est_index")], axis=1).astype(np.int32)
    pairs = np.empty((P, 6), dtype=np.float64)
    pairs[:, :4] = np.asarray(K4, dtype=np.float64).reshape(-1, 4)
    pairs[:, 4] = [vsd_delta_as_compared(d) for d in delta] if np.ndim(delta) else vsd_delta_as_compared(delta)
    pairs[:, 5] = np.asarray(diameter, dtype=np.float64)
    index_d, pairs_d = torch.from_numpy(index).to(dev), torch.from_numpy(pairs).to(dev)
    n = _count_ints()
    counts = torch.empty(P, n, dtype=torch.int32, device=dev)
    with on_device(dev):
        call("unopose_vsd_counts", ptr(depth_test), int(depth_test.shape[0]), ptr(depth_gt), int(depth_gt.shape[0]), ptr(depth_est),
             int(depth_est.shape[0]), ptr(index_d), ptr(pairs_d), ctypes.c_void_p(taus.ctypes.data), T, P, hw[0], hw[1], ptr(counts), stream_ptr(dev))
    return counts[:, :2 + T].to(torch.int64)


GT_COLUMNS = ("px_count_all", "px_count_valid", "px_count_visib", "obj_xmin", "obj_ymin", "obj_xmax", "obj_ymax", "visib_xmin", "visib_ymin",
              "visib_xmax", "visib_ymax")  # the row unopose_gt_visibility writes per ground truth


def gt_visibility(depth_test, canvas, K4, delta, image_index=None, canvas_index=None, masks=False):
    """The integers of `gt_info.gt_counts_host` for G ground truths over one image size (csrc/gtinfo.hip).  depth_test (n_test, H, W):
    float32 CUDA depth in mm; canvas (n_canvas, 3H, 3W): the objects rendered on the toolkit's enlarged canvas with the principal point at
    (cx + W, cy + H), straight from a `HipDepthRenderer(3W, 3H).render_batch`; ground truth g is canvas[canvas_index[g]] in front of
    depth_test[image_index[g]] (each index defaults to g).  K4 (G, 4) or (4,) = fx, fy, cx, cy of the image; delta: scalar or (G,).
    -> int64 CUDA tensor (G, 11), columns `GT_COLUMNS`: the three pixel counts, then min x, min y, max x, max y of the silhouette on the
    canvas in image coordinates (negative where the object leaves the image) and of the visible mask; the minimum / maximum of an empty
    set is the largest / smallest int32.  With masks=True also two uint8 CUDA tensors (G, H, W), 0 / 255: `dist_gt > 0` and the visible mask."""
    _maps(depth_test, "gt_visibility: depth_test")
    H, W = (int(v) for v in depth_test.shape[1:])
    _maps(canvas, "gt_visibility: canvas", (3 * H, 3 * W))
    dev = depth_test.device
    if canvas.device != dev:
        raise RuntimeError("gt_visibility: the maps live on different devices")
    G = len(canvas_index) if canvas_index is not None else len(image_index) if image_index is not None else int(canvas.shape[0])
    if not 1 <= G <= 65535:
        raise ValueError(f"gt_visibility: {G} ground truths per call (1 .. 65535)")
    if 9 * H * W > 1 << 30:
        raise ValueError(f"gt_visibility: a canvas of {3 * H} x {3 * W} pixels (at most 2^30)")
    idx = np.stack([_index(canvas_index, G, canvas.shape[0], "canvas_index", "gt_visibility"),
                    _index(image_index, G, depth_test.shape[0], "image_index", "gt_visibility")], axis=1).astype(np.int32)
    params = np.empty((G, 5), dtype=np.float64)
    params[:, :4] = np.asarray(K4, dtype=np.float64).reshape(-1, 4)
    params[:, 4] = [vsd_delta_as_compared(d) for d in delta] if np.ndim(delta) else vsd_delta_as_compared(delta)
    idx_d, params_d = torch.from_numpy(idx).to(dev), torch.from_numpy(params).to(dev)
    n = int(lib().unopose_gt_visibility_ints())
    out = torch.empty(G, n, dtype=torch.int32, device=dev)
    m = torch.empty(2, G, H, W, dtype=torch.uint8, device=dev) if masks else None
    null = ctypes.c_void_p(None)
    with on_device(dev):
        call("unopose_gt_visibility", ptr(canvas), int(canvas.shape[0]), ptr(depth_test), int(depth_test.shape[0]), ptr(idx_d), ptr(params_d), G, H, W,
             ptr(out), ptr(m[0]) if masks else null, ptr(m[1]) if masks else null, stream_ptr(dev))
    out = out.to(torch.int64)
    return (out, m[0], m[1]) if masks else out


def pose_errors(pts, symmetries, R_est, t_est, R_gt, t_gt, K, device):
    """`bop_eval.mssd` and `bop_eval.mspd` for P pairs of one object.  pts (n, 3) model points; symmetries: list of {"R", "t"} with the
    identity; R_est, R_gt (P, 3, 3), t_est, t_gt (P, 3); K (P, 3, 3) or (3, 3) -- host arrays, float64 on the device.
    -> (mssd (P,), mspd (P,)) float64 CUDA tensors, in model units and pixels."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("pose_errors: CPU not supported")
    pts = np.ascontiguousarray(np.asarray(pts, dtype=np.float64).reshape(-1, 3))
    syms = np.stack([np.concatenate([np.asarray(s["R"], np.float64).reshape(9), np.asarray(s["t"], np.float64).reshape(3)]) for s in symmetries])
    R_est, R_gt = np.asarray(R_est, np.float64).reshape(-1, 9), np.asarray(R_gt, np.float64).reshape(-1, 9)
    P = R_est.shape[0]
    if P < 1 or R_gt.shape[0] != P or pts.shape[0] < 1:
        raise ValueError(f"pose_errors: {P} estimates, {R_gt.shape[0]} ground truths, {pts.shape[0]} points")
    poses = np.concatenate([R_est, np.asarray(t_est, np.float64).reshape(P, 3), R_gt, np.asarray(t_gt, np.float64).reshape(P, 3)], axis=1)
    K = np.broadcast_to(np.asarray(K, np.float64).reshape(-1, 9), (P, 9))
    host = np.concatenate([pts.reshape(-1), syms.reshape(-1), poses[:, :12].reshape(-1), poses[:, 12:].reshape(-1), K.reshape(-1)])
    buf = torch.from_numpy(host).to(dev)  # one upload
    o = np.cumsum([0, pts.size, syms.size, 12 * P, 12 * P, 9 * P])
    part = [buf[o[i]:o[i + 1]] for i in range(5)]
    out = torch.empty(2, P, dtype=torch.float64, device=dev)
    with on_device(dev):
        call("unopose_pose_errors", ptr(part[0]), pts.shape[0], ptr(part[1]), syms.shape[0], ptr(part[2]), ptr(part[3]), ptr(part[4]), P,
             ptr(out[0]), ptr(out[1]), stream_ptr(dev))
    return out[0], out[1]


METRIC_NAMES = ("add", "proj", "re", "te", "projS", "reS", "teS")  # the rows unopose_pose_metrics writes


@functools.lru_cache(maxsize=None)
def adi_sizes():
    """(points per LDS tile, query points per workgroup) of the ADI kernel."""
    return int(lib().unopose_adi_tile_points()), int(lib().unopose_adi_slab_points())


def _pair_table(name, device, pts, R_est, t_est, R_gt, t_gt):
    """The host-side checks `pose_metrics` and `adi` share -> (device, pts (n,3), est (P,12), gt (P,12), finite (P,) bool)."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"{name}: CPU not supported")
    pts = np.ascontiguousarray(np.asarray(pts, dtype=np.float64).reshape(-1, 3))
    R_est, R_gt = np.asarray(R_est, np.float64).reshape(-1, 9), np.asarray(R_gt, np.float64).reshape(-1, 9)
    t_est, t_gt = np.asarray(t_est, np.float64).reshape(-1, 3), np.asarray(t_gt, np.float64).reshape(-1, 3)
    P = R_est.shape[0]
    if P < 1 or pts.shape[0] < 1 or not (R_gt.shape[0] == t_est.shape[0] == t_gt.shape[0] == P):
        raise ValueError(f"{name}: {P} / {t_est.shape[0]} estimates (R / t), {R_gt.shape[0]} / {t_gt.shape[0]} ground truths, {pts.shape[0]} points")
    if pts.shape[0] > 1 << 24 or not np.isfinite(pts).all():
        raise ValueError(f"{name}: {pts.shape[0]} points (at most 2^24, all finite)")
    est, gt = np.concatenate([R_est, t_est], axis=1), np.concatenate([R_gt, t_gt], axis=1)
    finite = np.isfinite(est).all(axis=1) & np.isfinite(gt).all(axis=1)
    return dev, pts, est, gt, finite


def _with_nan_rows(out, finite, dev):
    """A pair with a non-finite pose gets NaN in every output, decided on the host (the kernel saw an identity pose in its place)."""
    if not finite.all():
        out[..., torch.from_numpy(~finite).to(dev)] = float("nan")
    return out


def pose_metrics(pts, symmetries, R_est, t_est, R_gt, t_gt, K, device, proj_sym=True):
    """`bop_eval.add`, `proj`, `re`, `te`, `proj_sym`, `re_sym`, `te_sym` for P pairs of one object in one launch.  pts (n, 3) model points;
    symmetries: list of {"R", "t"} with the identity; R_est, R_gt (P, 3, 3), t_est, t_gt (P, 3); K (P, 3, 3) or (3, 3) -- host arrays,
    float64 on the device, one upload.  -> {"add", "proj", "re", "te", "projS", "reS", "teS"}: float64 CUDA tensors (P,) in model units,
    pixels and degrees; NaN for a pair with a non-finite pose.  Calling it twice gives the same bits.
    projS is the only output whose work is points x symmetries: proj_sym=False leaves that pass out and the dictionary then has no "projS"
    (reS / teS over a continuous symmetry's 315 poses cost a few hundred small products per pair)."""
    dev, pts, est, gt, finite = _pair_table("pose_metrics", device, pts, R_est, t_est, R_gt, t_gt)
    P = est.shape[0]
    if len(symmetries) < 1:
        raise ValueError("pose_metrics: no symmetries (the identity is one)")
    syms = np.stack([np.concatenate([np.asarray(s["R"], np.float64).reshape(9), np.asarray(s["t"], np.float64).reshape(3)]) for s in symmetries])
    K = np.asarray(K, np.float64).reshape(-1, 9)
    if K.shape[0] not in (1, P) or not np.isfinite(K).all() or not np.isfinite(syms).all():
        raise ValueError(f"pose_metrics: {K.shape[0]} intrinsics for {P} pairs, or a non-finite entry in K or the symmetries")
    K = np.broadcast_to(K, (P, 9))
    identity = np.concatenate([np.eye(3).reshape(9), [0.0, 0.0, 1.0]])
    est, gt = np.where(finite[:, None], est, identity), np.where(finite[:, None], gt, identity)
    host = np.concatenate([pts.reshape(-1), syms.reshape(-1), est.reshape(-1), gt.reshape(-1), K.reshape(-1)])
    buf = torch.from_numpy(host).to(dev)  # one upload
    o = np.cumsum([0, pts.size, syms.size, 12 * P, 12 * P, 9 * P])
    part = [buf[o[i]:o[i + 1]] for i in range(5)]
    out = torch.empty(len(METRIC_NAMES), P, dtype=torch.float64, device=dev)
    with on_device(dev):
        call("unopose_pose_metrics", ptr(part[0]), pts.shape[0], ptr(part[1]), syms.shape[0], ptr(part[2]), ptr(part[3]), ptr(part[4]), P, int(bool(proj_sym)),
             ptr(out), stream_ptr(dev))
    out = _with_nan_rows(out, finite, dev)
    return {k: out[i] for i, k in enumerate(METRIC_NAMES) if proj_sym or k != "projS"}


def adi(pts, R_est, t_est, R_gt, t_gt, device):
    """`bop_eval.adi` for P <= 65535 pairs of one object: the mean distance from each model point in the ground-truth pose to the nearest
    model point in the estimated pose, by a tiled brute force (n^2 distances per pair).  Host arrays in, one upload.
    -> float64 CUDA tensor (P,), NaN for a pair with a non-finite pose.  Calling it twice gives the same bits."""
    dev, pts, est, gt, finite = _pair_table("adi", device, pts, R_est, t_est, R_gt, t_gt)
    P, n = est.shape[0], pts.shape[0]
    if P > 65535:
        raise ValueError(f"adi: {P} pairs per call (1 .. 65535)")
    identity = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])
    est, gt = np.where(finite[:, None], est, identity), np.where(finite[:, None], gt, identity)
    buf = torch.from_numpy(np.concatenate([pts.reshape(-1), est.reshape(-1), gt.reshape(-1)])).to(dev)  # one upload
    o = np.cumsum([0, pts.size, 12 * P, 12 * P])
    part = [buf[o[i]:o[i + 1]] for i in range(3)]
    slabs = -(-n // adi_sizes()[1])
    work = torch.empty(P * slabs, dtype=torch.float64, device=dev)
    out = torch.empty(P, dtype=torch.float64, device=dev)
    with on_device(dev):
        call("unopose_adi", ptr(part[0]), n, ptr(part[1]), ptr(part[2]), P, ptr(work), ptr(out), stream_ptr(dev))
    return _with_nan_rows(out, finite, dev)


PTS_EXTENT_OBJECTS = 65535      # objects per launch sequence (the library's limit)
PTS_EXTENT_POINTS = 1 << 26     # points per upload: 1.5 GiB of float64 coordinates, as much again for the pruned copy
PTS_EXTENT_LIMIT = 1e150        # |coordinate| up to which a squared distance cannot overflow


@functools.lru_cache(maxsize=None)
def pts_extent_tile():
    """Points per LDS tile of the all-pairs kernel."""
    return int(lib().unopose_pts_extent_tile_points())


def pts_extent(points, device, prune=True):
    """`model_info.extent_host` for M objects (csrc/modelinfo.hip).  points: list of (V_k, 3) host arrays, 1 <= V_k <= 2^24, every
    coordinate finite and at most 1e150 in magnitude -- checked here, before anything is launched.  -> (min (M, 3), size (M, 3) = max - min,
    diameter (M,)), float64 host arrays; the diameter is the square root, taken on the host, of the largest (dx*dx + dy*dy) + dz*dz the
    kernel finds, pair (i, i) included: the bits of the host route and of the toolkit's `misc.calc_pts_diameter`.  prune=True lets only the
    points that can belong to a farthest pair into the all-pairs pass; it changes the time, not a bit of the result.  The objects go up in
    one upload with their offsets table and are scored by one launch sequence; more than 65535 objects or 2^26 points are split into
    several such calls.  Calling it twice gives the same bits."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("pts_extent: CPU not supported")
    clouds = []
    for k, p in enumerate(points):
        p = np.asarray(p, dtype=np.float64)
        if p.ndim != 2 or p.shape[1] != 3 or not 1 <= p.shape[0] <= 1 << 24:
            raise ValueError(f"pts_extent: object {k} is {p.shape}: (V, 3) with 1 <= V <= 2^24")
        if not (np.abs(p) <= PTS_EXTENT_LIMIT).all():  # False for NaN too
            raise ValueError(f"pts_extent: object {k} holds a coordinate that is not finite or beyond {PTS_EXTENT_LIMIT:g}")
        clouds.append(p)
    if not clouds:
        raise ValueError("pts_extent: no objects")
    doubles = int(lib().unopose_pts_extent_doubles())
    chunks, rows = [[]], 0
    for p in clouds:
        if chunks[-1] and (len(chunks[-1]) == PTS_EXTENT_OBJECTS or rows + len(p) > PTS_EXTENT_POINTS):
            chunks.append([])
            rows = 0
        chunks[-1].append(p)
        rows += len(p)
    pending = []
    for chunk in chunks:
        M = len(chunk)
        offsets = np.zeros(M + 1, dtype=np.int64)
        np.cumsum([len(p) for p in chunk], out=offsets[1:])
        N = int(offsets[-1])
        host = np.empty(3 * N + M + 1, dtype=np.float64)
        host[:3 * N] = np.concatenate([p.reshape(-1) for p in chunk])
        host[3 * N:] = offsets.view(np.float64)
        buf = torch.from_numpy(host).to(dev)  # one upload: the points, then the table the kernels read
        kept = torch.empty(3 * N, dtype=torch.float64, device=dev) if prune else None
        kept_count = torch.empty(M, dtype=torch.int64, device=dev) if prune else None
        out = torch.empty(M, doubles, dtype=torch.float64, device=dev)
        null = ctypes.c_void_p(None)
        with on_device(dev):
            call("unopose_pts_extent", ptr(buf), ctypes.c_void_p(offsets.ctypes.data), ptr(buf[3 * N:]), M, int(bool(prune)),
                 ptr(kept) if prune else null, ptr(kept_count) if prune else null, ptr(out), stream_ptr(dev))
        pending.append((out, buf, kept, kept_count))  # the buffers live until the read-back below
    res = np.concatenate([p[0].cpu().numpy() for p in pending])  # read back after everything is queued
    return res[:, :3].copy(), res[:, 3:6] - res[:, :3], np.sqrt(res[:, 6])


@functools.lru_cache(maxsize=None)
def ref_select_sizes():
    """(queries per workgroup, (candidate, symmetry) entries per LDS tile) of the reference-selection kernel."""
    return int(lib().unopose_ref_select_query_tile()), int(lib().unopose_ref_select_entry_tile())


def ref_select_slab(Q, C, S):
    """Candidates per workgroup that `ref_select` takes when `slab` is left to it."""
    slab = int(lib().unopose_ref_select_slab(int(Q), int(C), int(S)))
    if slab < 1:
        raise ValueError(f"ref_select: {lib().unopose_last_error().decode()}")
    return slab


def ref_select(Rq, q_scene, q_key, Rc, c_scene, c_key, syms, trace_min, seed=0, cross_scene=True, device="cuda", slab=None):
    """`ref_targets.select_host` for one object (csrc/reftargets.hip).  Rq (Q, 3, 3), Rc (C, 3, 3), syms (S >= 1, 3, 3) rotations; q_scene, c_scene
    int64 scene identities; q_key, c_key uint64 view keys; trace_min = 1 + 2 cos(max rotation); seed: a 64-bit unsigned number -- host arrays,
    checked by `ref_targets.check_inputs`, the host rule's own validator, before anything is launched (finite, |entry| <= 1e100), one upload.
    -> (pick (Q,) int64, n_eligible (Q,) int64, nearest (Q,) int64, nearest_trace (Q,) float64), host arrays with the host rule's bits.
    Q or C of zero returns empty or all -1 results without a launch.  `slab`: candidates per workgroup (default: what fills the device); the
    result does not depend on it.  Calling it twice gives the same bits."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("ref_select: CPU not supported")
    from ..ref_targets import check_inputs  # one validator for both routes

    Rq, q_scene, q_key, Rc, c_scene, c_key, syms, trace_min, seed = check_inputs(Rq, q_scene, q_key, Rc, c_scene, c_key, syms, trace_min, seed)
    Q, C, S = len(Rq), len(Rc), len(syms)
    if Q == 0 or C == 0:
        return np.full(Q, -1, np.int64), np.zeros(Q, np.int64), np.full(Q, -1, np.int64), np.full(Q, -np.inf)
    slab = ref_select_slab(Q, C, S) if slab is None else int(slab)
    if not 1 <= slab <= C:
        raise ValueError(f"ref_select: {slab} candidates per slab (1 .. C = {C})")
    host = np.concatenate([Rq.reshape(-1), Rc.reshape(-1), syms.reshape(-1), q_scene.view(np.float64), q_key.view(np.float64), c_scene.view(np.float64),
                           c_key.view(np.float64)])
    buf = torch.from_numpy(host).to(dev)  # one upload
    o = np.cumsum([0, 9 * Q, 9 * C, 9 * S, Q, Q, C, C])
    part = [buf[o[i]:o[i + 1]] for i in range(7)]
    work = torch.empty(5 * Q * -(-C // slab), dtype=torch.int64, device=dev)
    out = torch.empty(4, Q, dtype=torch.int64, device=dev)
    with on_device(dev):
        call("unopose_ref_select", ptr(part[0]), ptr(part[3]), ptr(part[4]), Q, ptr(part[1]), ptr(part[5]), ptr(part[6]), C, ptr(part[2]), S, trace_min,
             seed, int(bool(cross_scene)), slab, ptr(work), ptr(out), stream_ptr(dev))
    res = out.cpu().numpy()
    return res[0].copy(), res[1].copy(), res[2].copy(), res[3].copy().view(np.float64)


@functools.lru_cache(maxsize=None)
def sym_deviation_sizes():
    """(query points per workgroup pass = points per LDS tile, candidates per launch) of the symmetry kernel."""
    return int(lib().unopose_sym_deviation_tile()), int(lib().unopose_sym_deviation_launch_candidates())


def sym_deviation(pts, transforms, bound=None, device="cuda"):
    """`model_sym.sym_deviation_host` on the device (csrc/symmetry.hip).  pts (N, 3), 1 <= N <= 2^22; transforms (C, 4, 4) or (C, 3, 4) matrices
    [R | t], 1 <= C <= 2^19; bound: a distance, None or inf for none -- host arrays, checked by `model_sym.check_inputs`, the host route's own
    validator, before anything is launched (finite, |entry| <= 1e100).  The candidates and their inverses (`model_sym.inverse_transforms`, formed
    on the host) go up with the points in one upload and through the kernel in one call.  -> (C,) float64 host array: sqrt(max(directed,
    directed of the inverse)), +inf where either direction has a point further than `bound` from the cloud: the host route's bits.  Calling it
    twice gives the same bits."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("sym_deviation: CPU not supported")
    from ..model_sym import both_directions, check_inputs, two_sided  # one validator and one combination for both routes

    p, R, t, bound2 = check_inputs(pts, transforms, bound)
    table = both_directions(R, t)
    N, C2 = len(p), len(table)
    buf = torch.from_numpy(np.concatenate([p.reshape(-1), table.reshape(-1)])).to(dev)  # one upload
    out = torch.empty(C2, dtype=torch.float64, device=dev)
    with on_device(dev):
        call("unopose_sym_deviation", ptr(buf), N, ptr(buf[3 * N:]), C2, bound2, ptr(out), stream_ptr(dev))
    return two_sided(out.cpu().numpy())
