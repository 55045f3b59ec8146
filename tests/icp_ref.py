"""The rule of `ops.icp_refine` (csrc/icp.hip), stated once in numpy.  A helper module, not a test.

For one pair: query cloud P (N1, 3), reference cloud Q (N2, 3), optional mask m (N1) (non-zero: the point takes part), pose (R, t) with
p ~ R q + t (the convention of `fine_pose`: (p - t) @ R maps P into Q's frame), threshold tau > 0, iters >= 0.

    prev = 0
    for k in range(iters):
        x_i  = ((p_i0 - t0) R[0][c] + (p_i1 - t1) R[1][c]) + (p_i2 - t2) R[2][c]        c = 0, 1, 2
        j_i  = argmin_j ((x_i0 - q_j0)^2 + (x_i1 - q_j1)^2) + (x_i2 - q_j2)^2           lowest j on ties;  d_i = sqrt(minimum)
        in_i = m_i != 0 and d_i < tau ;  c_k = sum in_i ;  trace[k] = c_k
        if c_k <= prev or c_k < 3: break            (entries of trace after the break are -1; the pose stays as it is)
        prev = c_k
        w_i  = in_i / (1 + (d_i / tau)^2)
        (R, t) = weighted_procrustes(src = q_{j_i}, ref = p_i, w, weight_thresh = 0, eps = 1e-5)

This is the reference's `post_refinement` (utils/model_utils.py:649-664) per pair with the correspondences found anew in every iteration;
the Procrustes step is the project's (model_utils.py:667-743), whose centroid normalisation differs from `rigid_transform_3d`'s by eps only.
The argmin is a scan in ascending j with a strict <, starting from (infinity, j = 0): a distance that is NaN or infinite is never taken.

`icp(..., dtype=np.float64)` is the restatement every test compares with.  `dtype=np.float32` evaluates the same expressions in float32
with sequential sums (np.cumsum): the same rule at the kernel's precision and another summation order, used to find the inputs on which
float32 rounding does not change an inlier decision (the condition under which a float64 comparison of the kernel means anything) and to
measure the float32 noise floor of the final pose.  `corr`: fixed correspondences j_i instead of the search (what `post_refinement` has).
"""
import functools

import numpy as np


def _sum0(a):
    """Sum over axis 0: pairwise in float64 (numpy's), one element after the other in float32."""
    if a.dtype == np.float32:
        return np.cumsum(a, axis=0, dtype=np.float32)[-1]
    return a.sum(0)


def weighted_procrustes(src, ref, w, eps=1e-5):
    """model_utils.py:667-743 with weight_thresh = 0 for one problem, in the dtype of its inputs: R, t with ref ~ R src + t."""
    dt = src.dtype
    w = w / (_sum0(w) + dt.type(eps))
    cs, cr = _sum0(src * w[:, None]), _sum0(ref * w[:, None])
    a, b = src - cs, w[:, None] * (ref - cr)
    H = _sum0(a[:, :, None] * b[:, None, :])
    U, _, Vt = np.linalg.svd(H)
    V = Vt.T
    D = np.eye(3, dtype=dt)
    D[2, 2] = np.sign(np.linalg.det(V @ U.T))
    R = (V @ D @ U.T).astype(dt)
    return R, (cr - R @ cs).astype(dt)


def transform(P, R, t):
    a = P - t
    return (a[:, 0:1] * R[0] + a[:, 1:2] * R[1]) + a[:, 2:3] * R[2]


def search(x, Q, chunk=512):
    """(j, d): index of the nearest row of Q (lowest on ties) and the distance to it, in x's dtype."""
    j = np.empty(len(x), np.int64)
    m = np.empty(len(x), x.dtype)
    for s in range(0, len(x), chunk):
        e = x[s:s + chunk, None, :] - Q[None, :, :]
        d2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
        d2 = np.where(d2 < np.inf, d2, np.inf)   # the strict-< scan from (inf, 0) takes neither a NaN nor an infinity
        j[s:s + chunk] = np.argmin(d2, 1)
        m[s:s + chunk] = d2[np.arange(d2.shape[0]), j[s:s + chunk]]
    return j, np.sqrt(m)


def icp(P, Q, mask, R, t, tau, iters, dtype=np.float64, corr=None):
    """-> dict(R, t, trace (iters,) int, idx, dist (of the last search that ran; None when iters == 0), solved (Procrustes steps taken))."""
    P, Q, R, t = (np.asarray(v, dtype) for v in (P, Q, R, t))
    live = np.ones(len(P), bool) if mask is None else np.asarray(mask) != 0
    tau = dtype(tau)
    trace = np.full(iters, -1, np.int64)
    prev, solved, j, d = 0, 0, None, None
    for k in range(iters):
        x = transform(P, R, t)
        if corr is None:
            j, d = search(x, Q)
        else:
            j = np.asarray(corr)
            e = x - Q[j]
            d = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
        inl = live & (d < tau)
        c = int(inl.sum())
        trace[k] = c
        if c <= prev or c < 3:
            break
        prev = c
        r = d / tau
        w = np.where(inl, dtype(1) / (dtype(1) + r * r), dtype(0)).astype(dtype)
        R, t = weighted_procrustes(Q[j], P, w)
        solved += 1
    return dict(R=R, t=t, trace=trace, idx=j, dist=d, solved=solved)


def icp_batch(P, Q, mask, R, t, tau, iters, dtype=np.float64):
    outs = [icp(P[b], Q[b], None if mask is None else mask[b], R[b], t[b], tau, iters, dtype) for b in range(len(P))]
    return {k: (np.stack([o[k] for o in outs]) if outs[0][k] is not None else None) for k in outs[0]}


# ------------------------------------------------------------------------------------------------ synthetic problems -----
def rot(axis, angle):
    """Rodrigues rotation (float64)."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def surface(n, rng):
    """n points on a surface without a symmetry: an ellipsoid with semi-axes (0.5, 0.35, 0.22), bumped by low harmonics.  Returns the points
    and their outward direction (the unbumped ellipsoid's normal, enough for a visibility test)."""
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    th, ph = np.arccos(u[:, 2]), np.arctan2(u[:, 1], u[:, 0])
    r = 1 + 0.18 * np.sin(2 * ph + 0.4) * np.sin(th) ** 2 + 0.12 * np.cos(3 * th + 1.1) + 0.1 * np.sin(ph - 0.7) * np.sin(th)
    ax = np.array([0.5, 0.35, 0.22])
    nrm = u / ax
    return u * r[:, None] * ax, nrm / np.linalg.norm(nrm, axis=1, keepdims=True)


def rot_err_deg(Ra, Rb):
    return float(np.degrees(np.arccos(np.clip((np.trace(np.asarray(Ra, np.float64).T @ np.asarray(Rb, np.float64)) - 1) / 2, -1, 1))))


def problem(seed, n1=384, n2=1024, angle_deg=8.0, shift=0.04, noise=0.002):
    """A partial-view pair: Q = n2 surface points; P = n1 OTHER points of the same surface that face a view direction (a half-space-visible
    subset), under the pose (R_gt, t_gt) (p = R_gt q + t_gt) with `noise`; the start is that pose perturbed by `angle_deg` and `shift`.
    float32 arrays (what the kernel is given) and the float64 truth."""
    rng = np.random.default_rng(seed)
    Q, _ = surface(n2, rng)
    S, nrm = surface(4 * n1, rng)
    view = rng.normal(size=3)
    view /= np.linalg.norm(view)
    vis = np.flatnonzero(nrm @ view > 0.1)[:n1]
    assert len(vis) == n1
    R_gt = rot(rng.normal(size=3), rng.uniform(0, np.pi))
    t_gt = rng.uniform(-0.3, 0.3, 3)
    P = S[vis] @ R_gt.T + t_gt + noise * rng.normal(size=(n1, 3))
    R0 = R_gt @ rot(rng.normal(size=3), np.radians(angle_deg))
    d = rng.normal(size=3)
    t0 = t_gt + shift * d / np.linalg.norm(d)
    f = np.float32
    return dict(P=P.astype(f), Q=Q.astype(f), R0=R0.astype(f), t0=t0.astype(f), R_gt=R_gt, t_gt=t_gt)


def pose_dist(Ra, ta, Rb, tb):
    """max |dR| and max |dt|: the distance between two poses the tests bound."""
    return max(float(np.abs(np.asarray(Ra, np.float64) - np.asarray(Rb, np.float64)).max()),
               float(np.abs(np.asarray(ta, np.float64) - np.asarray(tb, np.float64)).max()))


# The seeds of `problem` the GPU multi-iteration tests use, with a threshold below the start's displacement (about 0.05) so that the inlier
# count grows over several iterations.  tests/test_icp_ref_cpu.py checks that on each of them the float64 and the float32 restatement give
# identical traces (no inlier decision hangs on float32 rounding); the distance of their final poses is the float32 noise floor.
GPU_SEEDS = (1, 2, 3, 4)
GPU_TAU = 0.03
GPU_ITERS = 16


@functools.lru_cache(maxsize=None)
def screened():
    """-> (problems, float64 results, float32 results, noise floor) for GPU_SEEDS, computed once per process.  The noise floor is the
    largest distance over the seeds between the final poses of the two restatements."""
    zs = [problem(s) for s in GPU_SEEDS]
    r64 = [icp(z["P"], z["Q"], None, z["R0"], z["t0"], GPU_TAU, GPU_ITERS) for z in zs]
    r32 = [icp(z["P"], z["Q"], None, z["R0"], z["t0"], GPU_TAU, GPU_ITERS, dtype=np.float32) for z in zs]
    floor = max(pose_dist(a["R"], a["t"], b["R"], b["t"]) for a, b in zip(r64, r32))
    return zs, r64, r32, floor
