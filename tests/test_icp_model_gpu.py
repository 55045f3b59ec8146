"""GPU: the opt-in pose refinement inside the model (`fine_point_matching.icp_iters`, `ops.icp_refine` between the fine head's Procrustes
and its verification).  Inputs and weights: the builders of tests/test_model_gpu.py (the `forward_cfg1` fixture, trained-like weights)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ("init_R", "init_t", "init_pose_score", "pred_R", "pred_t", "pred_pose_score")


def load(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    return {k: torch.from_numpy(z[k]).cuda() if z[k].ndim else z[k].item() for k in z.files}


@pytest.fixture(scope="module")
def models():
    """(a model built WITHOUT the two keys, one built with them at their defaults) on the same trained-like weights."""
    from oracle.unopose_ref import default_cfg, random_state_dict  # weights only (test infrastructure)
    from unopose_amd.model import UNOPose, default_model_cfg

    sd = random_state_dict(default_cfg(), seed=0, tame=0.1)
    with_keys = default_model_cfg(fine_npoint=1024)
    assert with_keys["fine_point_matching"]["icp_iters"] == 0 and with_keys["fine_point_matching"]["icp_inlier_thres"] == 0.1
    without = default_model_cfg(fine_npoint=1024)
    for k in ("icp_iters", "icp_inlier_thres"):
        del without["fine_point_matching"][k]
    out = []
    for cfg in (without, with_keys):
        m = UNOPose(cfg)
        m.load_state_dict(sd, strict=True)
        out.append(m.cuda().eval())
    return out


@pytest.fixture(scope="module")
def inputs():
    z = load("forward_cfg1")
    ep = {k: z[k] for k in ("pts", "tem1_pts", "rgb", "tem1_rgb", "rgb_choose", "tem1_choose")}
    ep["coarse_rand"] = z["rand"]
    return ep


def _run(model, ep, amp, iters=None, fine_taps=False):
    """One forward; with `iters` the key is set for this call.  -> (outputs, the refinement's record, the model's own taps)."""
    fine = model.fine_point_matching
    old = dict(fine.cfg)
    rec = {}
    model.taps = {}
    if fine_taps:
        fine.taps = rec
    else:
        fine.icp_taps = rec
    try:
        if iters is not None:
            fine.cfg["icp_iters"] = iters
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            out = model(dict(ep))
        return {k: out[k].clone() for k in KEYS}, rec, model.taps
    finally:
        fine.cfg.clear()
        fine.cfg.update(old)
        model.taps = fine.taps = fine.icp_taps = None


@torch.no_grad()
@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "bf16"])
def test_off_by_default_bit_for_bit(models, inputs, amp):
    without, with_keys = models
    a, rec_a, _ = _run(without, inputs, amp)
    b, rec_b, _ = _run(with_keys, inputs, amp)
    c, rec_c, _ = _run(with_keys, inputs, amp, iters=0)
    assert rec_a == {} and rec_b == {} and rec_c == {}
    for k in KEYS:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k


def _check_refined(out, rec, taps, iters, thres):
    from unopose_amd import ops
    from unopose_amd._lib import call, ptr, stream_ptr

    assert set(rec) >= {"icp_R0", "icp_t0", "icp_w1", "icp_p1", "icp_p2", "icp_trace"}
    p1, p2, w1 = rec["icp_p1"], rec["icp_p2"], rec["icp_w1"]
    B, N1, N2 = p1.shape[0], p1.shape[1], p2.shape[1]
    assert rec["icp_trace"].shape == (B, iters) and rec["icp_trace"].dtype == torch.int32 and (rec["icp_trace"][:, 0] >= 0).all()
    assert torch.equal(w1, (w1 > 0).float()) and 0 < w1.sum().item()
    R, t, trace, _, _ = ops.icp_refine(p1, p2, rec["icp_R0"], rec["icp_t0"], w1, iters, thres, return_trace=True)
    assert torch.equal(trace, rec["icp_trace"])
    assert torch.equal(out["pred_R"], R)
    assert torch.equal(out["pred_t"], ops.scale_by_radius(t, taps["radius"], multiply=True))
    dis = torch.empty(B, N1, dtype=torch.float32, device=p1.device)
    call("unopose_min_dist", ptr(p1), ptr(p2), B, N1, N2, ptr(R), ptr(t), 1, ptr(dis), stream_ptr())
    assert torch.equal(out["pred_pose_score"], ops.pose_score(dis, w1, 0.15))
    return trace


@torch.no_grad()
@pytest.mark.parametrize("route", ["stacked-fp32", "fused-bf16", "taps-fp32", "taps-bf16", "unstacked-fp32", "unstacked-fused-bf16"])
def test_refined_pose_is_icp_refine_of_the_tapped_pose(models, inputs, route):
    """pred_R / pred_t are `ops.icp_refine` of the pose the fine head's Procrustes gave, over its own clouds and mask (w1 = label1 > 0), and
    pred_pose_score is the existing kernels' score of that refined pose -- on the stacked and the unstacked forward, with the pose head
    on the stored similarity (`fine_pose`: fp32, and whenever `taps` is set) and on the recomputed one (`fine_pose_from_features`: bf16)."""
    import unopose_amd.model.unopose as U

    model = models[1]
    amp = route.endswith("bf16")
    stacked = U.STACKED_FINE
    try:
        if route.startswith("unstacked"):
            U.STACKED_FINE = False
        plain, _, _ = _run(model, inputs, amp, iters=0, fine_taps=route.startswith("taps"))
        out, rec, taps = _run(model, inputs, amp, iters=5, fine_taps=route.startswith("taps"))
    finally:
        U.STACKED_FINE = stacked
    if route.startswith("taps"):
        assert "atten" in rec  # (the probe of the unfused pose head shares the dict)
    trace = _check_refined(out, rec, taps, 5, 0.1)
    for k in ("init_R", "init_t", "init_pose_score"):
        assert torch.equal(out[k], plain[k]), k
    print(route, "trace", trace.tolist(), "|pred_R - unrefined|", (out["pred_R"] - plain["pred_R"]).abs().max().item(),
          "score", plain["pred_pose_score"].tolist(), "->", out["pred_pose_score"].tolist())
    assert not torch.equal(out["pred_R"], plain["pred_R"])  # the refinement took at least one step on this pair


@torch.no_grad()
def test_coarse_only_ignores_the_keys(models, inputs):
    """(Training never reaches the pose head's eval branch: `forward` hands over to `forward_train` first.)"""
    model = models[1]
    fine = model.fine_point_matching
    assert fine._icp() == {}
    fine.cfg["icp_iters"] = 5
    try:
        assert fine._icp()["icp_iters"] == 5 and fine._icp()["icp_inlier_thres"] == 0.1
        model.test_coarse_only = True
        out = model(dict(inputs))
        assert torch.equal(out["pred_R"], out["init_R"])
    finally:
        model.test_coarse_only = False
        fine.cfg["icp_iters"] = 0


@torch.no_grad()
def test_graphed_forward_replays_the_refinement(models, inputs):
    from unopose_amd.graph import GraphedForward

    model = models[1]
    model.fine_point_matching.cfg["icp_iters"] = 5
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            eager = {k: v.clone() for k, v in model(dict(inputs)).items() if k in KEYS}
        g = GraphedForward(model, inputs)
        out = g(dict(inputs))
        torch.cuda.synchronize()
        for k in KEYS:
            assert torch.equal(out[k], eager[k]), k
    finally:
        model.fine_point_matching.cfg["icp_iters"] = 0
