"""GPU: `ops.icp_refine` (csrc/icp.hip) against the rule of tests/icp_ref.py.

One iteration: the search (idx, trace) equals the float32 numpy search exactly and dist to the last bit of the square root (1 ulp); the
new pose is compared with float64 Procrustes on those same correspondences at the tolerance tests/test_geom_gpu.py applies to
`weighted_procrustes` (1e-4).  Many iterations, on the seeds tests/test_icp_ref_cpu.py screens: the trace is the float64 restatement's
and the final pose within 4 x the float32 noise floor of it (`icp_ref.screened`: the distance between the float64 and the float32
restatement's final poses, 2.2e-7 -> bound 8.8e-7)."""
import numpy as np
import pytest
import torch

import icp_ref as I

pytestmark = pytest.mark.gpu
PROCRUSTES_TOL = 1e-4  # tests/test_geom_gpu.py: test_weighted_procrustes_stress_256_hypotheses
TILE = 4096            # csrc/icp.hip: ICP_TILE, reference points per LDS tile


def _cuda(*arrs):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _pairs(B, N1, N2, seed, masked):
    """B different pairs of one shape: surface samples under different poses and perturbations.  Duplicated reference points (every
    point of the first eighth again in the second half, and the eight before the tile boundary again right after it), query points that
    are images of duplicated points (exact ties: the lowest index has to win, across the tile boundary too), a mask with dead points."""
    rng = np.random.default_rng(seed)
    P, Q, R0, t0, M = [], [], [], [], []
    for b in range(B):
        q, _ = I.surface(N2, rng)
        k = N2 // 8
        if k:
            q[N2 // 2:N2 // 2 + k] = q[:k]
        if N2 > TILE:
            m = min(8, N2 - TILE)
            q[TILE:TILE + m] = q[TILE - 8:TILE - 8 + m]
        q = q.astype(np.float32)
        R = I.rot(rng.normal(size=3), rng.uniform(0, np.pi))
        t = rng.uniform(-0.3, 0.3, 3)
        s, _ = I.surface(N1, rng)
        p = s @ R.T + t + 0.002 * rng.normal(size=(N1, 3))
        src = np.r_[np.arange(min(k, N1 // 4)), np.arange(max(N2 - 3, 0), N2)]  # duplicated points, and the last ones of the last tile
        if N2 > TILE:
            src = np.r_[src, np.arange(TILE - 8, TILE - 8 + min(8, N2 - TILE))]
        src = src[:max(N1 // 2, 1)]
        p[:len(src)] = q[src].astype(np.float64) @ R.T + t
        P.append(p.astype(np.float32))
        Q.append(q)
        R0.append((R @ I.rot(rng.normal(size=3), np.radians(3.0 + b))).astype(np.float32))
        t0.append((t + 0.01 * rng.normal(size=3)).astype(np.float32))
        M.append((rng.uniform(size=N1) > 0.3).astype(np.float32) * rng.choice([1.0, -2.0, 0.5], N1).astype(np.float32))
    return np.stack(P), np.stack(Q), np.stack(R0), np.stack(t0), (np.stack(M) if masked else None)


SHAPES = [(1, 1, 5000, False), (3, 63, 1, True), (1, 65, 255, True), (3, 1000, 257, True), (1, 2048, 4097, False), (3, 2048, 5000, True),
          (3, 65, 4097, True), (1, 1000, 1, False)]


@pytest.mark.parametrize("B,N1,N2,masked", SHAPES, ids=[f"B{b}-N1_{n1}-N2_{n2}" + ("-mask" if m else "") for b, n1, n2, m in SHAPES])
def test_one_iteration(B, N1, N2, masked):
    from unopose_amd import ops

    tau = 0.05
    P, Q, R0, t0, M = _pairs(B, N1, N2, seed=100 + N1 + N2, masked=masked)
    R, t, trace, idx, dist = (v.cpu().numpy() for v in ops.icp_refine(*_cuda(P, Q, R0, t0, M), iters=1, inlier_thres=tau, return_trace=True))
    assert trace.shape == (B, 1) and idx.shape == (B, N1) and dist.shape == (B, N1)
    ties = 0
    for b in range(B):
        j, d = I.search(I.transform(P[b], R0[b], t0[b]), Q[b])  # float32, the kernel's expressions
        assert j.dtype == np.int64 and d.dtype == np.float32
        assert np.array_equal(idx[b], j), (b, np.flatnonzero(idx[b] != j)[:8])
        ulp = np.abs(dist[b].view(np.int32).astype(np.int64) - d.view(np.int32).astype(np.int64)).max()
        print(f"pair {b}: dist differs from numpy's sqrt by at most {ulp} ulp")
        assert ulp <= 1
        live = np.ones(N1, bool) if M is None else M[b] != 0
        inl = live & (dist[b] < np.float32(tau))
        assert trace[b, 0] == int(inl.sum()) == int((live & (d < np.float32(tau))).sum())
        ties += int((Q[b][j] == Q[b][np.minimum(j + max(N2 // 2, 1), N2 - 1)]).all(1).sum()) if N2 > 8 else 0
        if trace[b, 0] < 3:
            assert np.array_equal(R[b], R0[b]) and np.array_equal(t[b], t0[b])
            continue
        r = dist[b].astype(np.float64) / np.float64(np.float32(tau))
        w = np.where(inl, 1.0 / (1.0 + r * r), 0.0)
        Rr, tr = I.weighted_procrustes(Q[b][j].astype(np.float64), P[b].astype(np.float64), w)
        if len(np.unique(j[inl])) < 3:
            # every inlier matched to one or two reference points (N2 = 1): H has rank <= 1 and the rotation is not defined by the rule
            # (tests/test_geom_gpu.py: "a deterministic valid rotation").  What is defined: a proper rotation, and t = c_ref - R c_src.
            Rk = R[b].astype(np.float64)
            wn = w / (w.sum() + 1e-5)
            cs, cr = (Q[b][j] * wn[:, None]).sum(0), (P[b] * wn[:, None]).sum(0)
            assert np.abs(Rk @ Rk.T - np.eye(3)).max() < PROCRUSTES_TOL and abs(np.linalg.det(Rk) - 1) < PROCRUSTES_TOL
            assert np.abs(t[b] - (cr - Rk @ cs)).max() < PROCRUSTES_TOL
            continue
        e = I.pose_dist(R[b], t[b], Rr, tr)
        print(f"pair {b}: {trace[b, 0]} inliers, |pose - float64 Procrustes| = {e:.2e}")
        assert e < PROCRUSTES_TOL, (b, e)
    if N2 > 8 and N1 >= 63:
        assert ties > 0  # (the case holds query points whose nearest reference point exists twice)
    if B > 1:
        assert not np.array_equal(R[0], R[1])


def test_tile_boundary_and_ties_pick_the_lowest_index():
    """Reference points on both sides of the tile boundary and exact duplicates: index 4095 / 4096 / the last one are found, and of two
    equal points the lower index, also when the duplicate lies in the next tile."""
    from unopose_amd import ops

    N2 = TILE + 5
    rng = np.random.default_rng(7)
    Q = rng.uniform(-1, 1, (1, N2, 3)).astype(np.float32)
    Q[0, TILE] = Q[0, 17]            # a duplicate in the second tile of a point in the first
    Q[0, TILE + 1] = Q[0, TILE - 1]  # ... of the last point of the first tile
    Q[0, 300] = Q[0, 200]
    want = np.array([17, TILE - 1, 200, TILE + 2, TILE + 4, 0, TILE - 2])
    P = Q[:, want].copy()
    R0, t0 = np.eye(3, dtype=np.float32)[None], np.zeros((1, 3), np.float32)
    _, _, trace, idx, dist = ops.icp_refine(*_cuda(P, Q, R0, t0), iters=1, inlier_thres=0.01, return_trace=True)
    assert idx.cpu().numpy()[0].tolist() == want.tolist()
    assert (dist == 0).all() and trace.item() == len(want)


def _degenerate_batch():
    z = [I.problem(s) for s in (1, 2, 3, 4, 5)]
    P, Q = np.stack([v["P"] for v in z]), np.stack([v["Q"] for v in z])
    R0, t0 = np.stack([v["R0"] for v in z]), np.stack([v["t0"] for v in z])
    N1 = P.shape[1]
    M = np.ones((5, N1), np.float32)
    M[0] = 0                                             # pair 0: nobody takes part
    _, d = I.search(I.transform(P[1], R0[1], t0[1]), Q[1])
    two = np.flatnonzero(d < np.float32(I.GPU_TAU) * np.float32(0.5))[:2]
    M[1] = 0
    M[1, two] = 1                                        # pair 1: two inliers
    P[2] = Q[2, 100:100 + N1]                            # pair 2: every point an inlier at once, so the count cannot grow at k = 1
    R0[2], t0[2] = I.rot([1, 2, 3], 0.002).astype(np.float32), np.float32([1e-3, -1e-3, 5e-4])
    return P, Q, R0, t0, M                               # pairs 3, 4: normal


def test_degenerate_pairs_keep_their_pose_beside_normal_ones():
    from unopose_amd import ops

    P, Q, R0, t0, M = _degenerate_batch()
    dev = _cuda(P, Q, R0, t0, M)
    iters = 6
    R, t, trace, idx, dist = (v.cpu().numpy() for v in ops.icp_refine(*dev, iters=iters, inlier_thres=I.GPU_TAU, return_trace=True))
    assert trace[0].tolist() == [0] + [-1] * (iters - 1) and trace[1].tolist() == [2] + [-1] * (iters - 1)
    for b in (0, 1):
        assert np.array_equal(R[b], R0[b]) and np.array_equal(t[b], t0[b])
    N1 = P.shape[1]
    assert trace[2].tolist() == [N1, N1] + [-1] * (iters - 2)
    one = [v.cpu().numpy() for v in ops.icp_refine(*dev, iters=1, inlier_thres=I.GPU_TAU)]
    assert np.array_equal(R[2], one[0][2]) and np.array_equal(t[2], one[1][2]) and not np.array_equal(R[2], R0[2])
    # iters = 0: every pair keeps its pose, nothing was searched
    R_, t_, trace_, idx_, dist_ = (v.cpu().numpy() for v in ops.icp_refine(*dev, iters=0, inlier_thres=I.GPU_TAU, return_trace=True))
    assert np.array_equal(R_, R0) and np.array_equal(t_, t0) and trace_.shape == (5, 0) and (idx_ == -1).all() and np.isinf(dist_).all()
    # the normal pairs: as when run alone, and really refined
    for b in (3, 4):
        alone = [v.cpu().numpy() for v in ops.icp_refine(*_cuda(P[b:b + 1], Q[b:b + 1], R0[b:b + 1], t0[b:b + 1], M[b:b + 1]), iters=iters,
                                                         inlier_thres=I.GPU_TAU, return_trace=True)]
        for got, want in zip((R, t, trace, idx, dist), alone):
            assert np.array_equal(got[b], want[0])
        k = int((trace[b] >= 0).sum())
        assert k >= 3 and (np.diff(trace[b][:k - 1]) > 0).all() and (trace[b][k:] == -1).all()


@pytest.fixture(scope="module")
def screened():
    zs, r64, r32, floor = I.screened()
    stack = lambda k: np.stack([z[k] for z in zs])  # noqa: E731
    return zs, r64, floor, _cuda(stack("P"), stack("Q"), stack("R0"), stack("t0"))


def test_many_iterations_on_the_screened_seeds(screened):
    from unopose_amd import ops

    zs, r64, floor, dev = screened
    R, t, trace, idx, dist = (v.cpu().numpy() for v in ops.icp_refine(*dev, iters=I.GPU_ITERS, inlier_thres=I.GPU_TAU, return_trace=True))
    margin = 4 * floor
    for b, (z, r) in enumerate(zip(zs, r64)):
        assert np.array_equal(trace[b], r["trace"]), (b, trace[b], r["trace"])
        e =I.pose_dist(R[b], t[b], r["R"], r["t"])
        err, err_ref = I.pose_dist(R[b], t[b], z["R_gt"], z["t_gt"]), I.pose_dist(r["R"], r["t"], z["R_gt"], z["t_gt"])
        print(f"seed {I.GPU_SEEDS[b]}: |kernel - float64 restatement| = {e:.3e} (bound {margin:.3e}); pose error {err:.6f} vs {err_ref:.6f}")
    for b, (z, r) in enumerate(zip(zs, r64)):
        assert I.pose_dist(R[b], t[b], r["R"], r["t"]) <= margin, b
        assert I.pose_dist(R[b], t[b], z["R_gt"], z["t_gt"]) <= I.pose_dist(r["R"], r["t"], z["R_gt"], z["t_gt"]) + margin, b


def test_two_calls_are_bit_equal(screened):
    from unopose_amd import ops

    dev = screened[3]
    a = ops.icp_refine(*dev, iters=I.GPU_ITERS, inlier_thres=I.GPU_TAU, return_trace=True)
    b = ops.icp_refine(*dev, iters=I.GPU_ITERS, inlier_thres=I.GPU_TAU, return_trace=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    R, t = ops.icp_refine(*dev, iters=I.GPU_ITERS, inlier_thres=I.GPU_TAU)
    assert torch.equal(R, a[0]) and torch.equal(t, a[1])


def test_composite_agrees_in_trace(screened):
    from unopose_amd import ops

    zs, r64, floor, dev = screened
    a = ops.icp_refine(*dev, iters=I.GPU_ITERS, inlier_thres=I.GPU_TAU, return_trace=True)
    b = ops.icp_refine_torch(*dev, iters=I.GPU_ITERS, inlier_thres=I.GPU_TAU, return_trace=True)
    assert torch.equal(a[2], b[2])
    assert torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])  # the last search: the same expressions, bit for bit
    assert (a[0] - b[0]).abs().max().item() < PROCRUSTES_TOL and (a[1] - b[1]).abs().max().item() < PROCRUSTES_TOL


def test_autocast_does_not_change_the_result(screened):
    from unopose_amd import ops

    dev = screened[3]
    want = ops.icp_refine(*dev, iters=3, inlier_thres=I.GPU_TAU)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        got = ops.icp_refine(*dev, iters=3, inlier_thres=I.GPU_TAU)
    assert got[0].dtype == torch.float32 and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_errors():
    from unopose_amd import ops
    from unopose_amd._lib import call, ptr, stream_ptr

    f = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    eye = torch.eye(3, device="cuda")[None]
    for n1, n2 in ((4097, 8), (8, 16385)):
        with pytest.raises(ValueError, match="exceed the limits"):
            ops.icp_refine(f(1, n1, 3), f(1, n2, 3), eye, f(1, 3))
    with pytest.raises(ValueError, match="exceed the limits"):
        ops.icp_refine(f(65536, 1, 3), f(65536, 1, 3), eye.expand(65536, 3, 3), f(65536, 3))
    with pytest.raises(ValueError, match="inlier_thres > 0"):
        ops.icp_refine(f(1, 8, 3), f(1, 8, 3), eye, f(1, 3), inlier_thres=0.0)
    with pytest.raises(ValueError, match="mask"):
        ops.icp_refine(f(1, 8, 3), f(1, 8, 3), eye, f(1, 3), mask=f(1, 7))
    p, q, R, t, Ro, to = f(1, 8, 3), f(1, 8, 3), eye.contiguous(), f(1, 3), f(1, 3, 3), f(1, 3)
    ok = [ptr(p), ptr(q), None, 1, 8, 8, ptr(R), ptr(t), 0.1, 2, ptr(Ro), ptr(to), None, None, None, stream_ptr()]
    call("unopose_icp_refine", *ok)
    for i in (0, 1, 6, 7, 10, 11):
        bad = list(ok)
        bad[i] = None
        with pytest.raises(RuntimeError, match="icp_refine: null pointer"):
            call("unopose_icp_refine", *bad)
    for i, v in ((3, -1), (4, 0), (5, 0), (9, -1), (8, 0.0), (8, float("nan"))):
        bad = list(ok)
        bad[i] = v
        with pytest.raises(RuntimeError, match="icp_refine: bad sizes"):
            call("unopose_icp_refine", *bad)
    for i, v in ((3, 65536), (4, 4097), (5, 16385)):
        bad = list(ok)
        bad[i] = v
        with pytest.raises(RuntimeError, match="icp_refine: .*exceed the limits"):  # (nothing is launched)
            call("unopose_icp_refine", *bad)
    torch.cuda.synchronize()
