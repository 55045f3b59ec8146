"""CPU: the rule of `ops.icp_refine` as tests/icp_ref.py states it -- against the reference's `post_refinement`, on a synthetic partial-view
pair, and the screening of the inputs the GPU tests use.

Tolerance against the reference (test_restatement_reproduces_post_refinement): 2.32e-6 on every entry of R and t.  Measured, not chosen:
the largest |restatement - reference| over the cases of tests/golden/icp_post_refinement.npz is 5.80e-7 (case 0; the others 1.8e-7 to
5.3e-7), times 4.  Its origin: the reference computes in float32 (transform, norms, weights, the 3x3 SVD), the restatement in float64,
and `rigid_transform_3d` divides its centroids by sum(w) + 1e-6 where the project's Procrustes normalises the weights by sum(w) + 1e-5
(a relative 1e-5 / sum(w), about 1e-7 here, on the centroids only)."""
import os

import numpy as np

import icp_ref as I

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "icp_post_refinement.npz")
REF_TOL = 4 * 5.80e-7


def test_restatement_reproduces_post_refinement():
    """With its search replaced by the fixture's fixed correspondences the restatement takes the reference's number of steps and ends at
    the reference's pose."""
    z = np.load(GOLD)
    n = int(z["n_cases"])
    assert n >= 4
    worst, steps = 0.0, []
    for c in range(n):
        g = lambda k: z[f"c{c}_{k}"]  # noqa: E731
        r = I.icp(g("P"), g("Q"), None, g("R0"), g("t0"), float(g("tau")), int(g("iters")), corr=g("corr"))
        assert r["solved"] == int(g("steps")), (c, r["solved"], int(g("steps")))
        e = I.pose_dist(r["R"], r["t"], g("R"), g("t"))
        print(f"case {c}: {r['solved']} steps, |restatement - reference| = {e:.3e}")
        worst = max(worst, e)
        steps.append(r["solved"])
    assert max(steps) >= 3 and min(steps) >= 1  # (the fixture exercises the loop, not only its first step)
    assert worst <= REF_TOL, worst


def test_convergence_on_a_partial_view():
    """A surface without a symmetry, the query a half-space-visible subset of other samples of it under a known pose, the start 8 degrees
    and 0.04 off: the restatement ends closer to the truth than it started, in rotation and in translation, and its inlier count grows
    strictly until the iteration that stops it."""
    for seed in I.GPU_SEEDS:
        z = I.problem(seed)
        r = I.icp(z["P"], z["Q"], None, z["R0"], z["t0"], I.GPU_TAU, I.GPU_ITERS)
        r0, r1 = I.rot_err_deg(z["R0"], z["R_gt"]), I.rot_err_deg(r["R"], z["R_gt"])
        t0, t1 = np.linalg.norm(z["t0"] - z["t_gt"]), np.linalg.norm(r["t"] - z["t_gt"])
        print(f"seed {seed}: rotation {r0:.2f} -> {r1:.2f} deg, translation {t0:.4f} -> {t1:.4f}, trace {r['trace'].tolist()}")
        assert r1 < r0 and t1 < t0, (seed, r0, r1, t0, t1)
        tr = r["trace"]
        k = int((tr >= 0).sum())  # entries written
        assert 3 <= k < I.GPU_ITERS and (tr[k:] == -1).all()  # stopped by the rule, not by the iteration limit
        assert (np.diff(tr[:k - 1]) > 0).all() and tr[k - 1] <= tr[k - 2]
        assert r["solved"] == k - 1


def test_gpu_seeds_are_screened():
    """The float32 restatement (the kernel's precision, another summation order) takes the float64 restatement's inlier decisions on every
    seed the GPU multi-iteration tests use: identical traces.  The distance of the two final poses is the float32 noise floor those tests
    scale their bound by; it has to be float32-sized for that to mean anything."""
    zs, r64, r32, floor = I.screened()
    for s, a, b in zip(I.GPU_SEEDS, r64, r32):
        assert np.array_equal(a["trace"], b["trace"]), (s, a["trace"], b["trace"])
        assert np.array_equal(a["idx"], b["idx"]), s
    print(f"float32 noise floor of the final pose over seeds {I.GPU_SEEDS}: {floor:.3e}")
    assert 1e-8 < floor < 1e-6, floor


def test_degenerate_pairs_keep_their_pose():
    z = I.problem(1)
    for mask, iters, tau in ((np.zeros(len(z["P"])), 5, 0.03), (None, 0, 0.03), (None, 5, 1e-6)):
        for dt in (np.float64, np.float32):
            r = I.icp(z["P"], z["Q"], mask, z["R0"], z["t0"], tau, iters, dtype=dt)
            assert np.array_equal(r["R"], z["R0"].astype(dt)) and np.array_equal(r["t"], z["t0"].astype(dt)) and r["solved"] == 0
            assert r["trace"].tolist() == ([0] + [-1] * (iters - 1) if iters else [])


def test_ties_go_to_the_lowest_index():
    Q = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [0, 0, 0]], np.float32)
    x = np.array([[0.9, 0, 0], [0.1, 0, 0], [np.nan, 0, 0]], np.float32)
    j, d = I.search(x, Q)
    assert j.tolist() == [1, 0, 0] and d[2] == np.inf
