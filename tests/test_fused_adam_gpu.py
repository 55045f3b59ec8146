"""GPU: optim.FusedAdam's fused route (csrc/optim.hip: prepare / finalise / update) on a parameter set built to hit the table logic -- sizes
around the 64-lane wave, the 256-thread workgroup, the 16-byte quad and the chunk length, a 0-element parameter and one whose gradient is None
-- with NaN / +inf / -inf planted at first, last and chunk-boundary positions, over 5 steps with changing gradients.

Parameters start at magnitudes in [0.5, 2) and lr is 1e-3, so no value comes near zero in 5 steps: "ulps of the parameter" is then one scale
per element for the whole run, and the update (~1e-3, known to ~1e-7 relative) carries its error far below it.  What is left is the rounding of
the parameter itself, once per step, for the kernel and for torch alike."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, BETAS, EPS, STEPS = 1e-3, (0.5, 0.999), 1e-6, 5
INF_STEPS = (0, 3)  # the steps whose gradients carry +-inf (their norm is ~1e5 sqrt(count)); NaN is planted in every step
MAX_NORMS = (1.0, 1e3, 1e12, None)  # below every step's norm; above the norm of the steps without inf (~150) only; far above all; no clipping


@pytest.fixture(scope="module")
def case():
    from unopose_amd.optim import table_ints

    chunk = table_ints()[0]
    sizes = [1, 3, 63, 64, 65, 255, 257, chunk - 1, chunk, chunk + 1, 2 * chunk + 5, 0]
    g = torch.Generator().manual_seed(20)
    params = [(torch.rand(n, generator=g) * 1.5 + 0.5) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1).float() for n in sizes]
    params.append(torch.rand(7, generator=g) + 0.5)  # the parameter whose gradient stays None
    grads = []
    for k in range(STEPS):
        gs = []
        for n in sizes:
            t = torch.randn(n, generator=g)
            spots = [i for i in (0, n - 1, chunk - 1, chunk, 2 * chunk - 1, 2 * chunk) if 0 <= i < n]
            for j, i in enumerate(dict.fromkeys(spots)):
                t[i] = (float("nan"), float("inf"), -float("inf"))[(j + k) % 3] if k in INF_STEPS else float("nan")
            gs.append(t)
        grads.append(gs)
    clean = [[torch.nan_to_num(t, nan=0.0, posinf=1e5, neginf=-1e5) for t in gs] for gs in grads]
    norms = [float(torch.cat(gs).double().pow(2).sum().sqrt()) for gs in clean]
    assert all(MAX_NORMS[0] < n for n in norms) and all((MAX_NORMS[1] < n) == (k in INF_STEPS) for k, n in enumerate(norms)) and max(norms) < MAX_NORMS[2]
    return dict(chunk=chunk, sizes=sizes, params=params, grads=grads, clean=clean, norms=norms)


def _params(case):
    return [torch.nn.Parameter(p.clone().cuda()) for p in case["params"]]


def _set_grads(ps, gs):
    for p, g in zip(ps, gs):  # the last parameter gets none
        p.grad = g.cuda() if not g.is_cuda else g.clone()  # (a new tensor every step; from device copies nothing waits for the device)
    ps[-1].grad = None


def _same_tree(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same_tree(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same_tree(x, y) for x, y in zip(a, b))
    return a == b


def _fused(case, steps=STEPS, max_norm=None, finite=None, grads="grads", sync=False):
    from unopose_amd.optim import FusedAdam

    ps = _params(case)
    opt = FusedAdam(ps, lr=LR, betas=BETAS, eps=EPS)
    norms = []
    resident = [[g.cuda() for g in gs] for gs in case[grads]]
    torch.cuda.synchronize()
    for k in range(steps):
        _set_grads(ps, resident[k % STEPS])
        norms.append(opt.step(finite, max_norm))
        assert opt.launches == 3
        if sync:
            torch.cuda.synchronize()
    return ps, opt, norms


def _torch_route(case, max_norm, steps=STEPS):
    """The parent route on the same device: nan_to_num per gradient, clip_grad_norm_, torch.optim.Adam(foreach=False)."""
    ps = _params(case)
    opt = torch.optim.Adam(ps, lr=LR, betas=BETAS, eps=EPS, foreach=False)
    norms = []
    for k in range(steps):
        _set_grads(ps, case["grads"][k])
        with_grad = [p for p in ps if p.grad is not None]
        for p in with_grad:
            torch.nan_to_num(p.grad, nan=0.0, posinf=1e5, neginf=-1e5, out=p.grad)
        norms.append(torch.nn.utils.clip_grad_norm_(with_grad, max_norm if max_norm is not None else float("inf"), foreach=False))
        opt.step()
    return ps, opt, norms


def _adam64(case, max_norm, steps=STEPS):
    """Adam's rule in float64 on the cleaned fp32 gradients, clipped by the float64 coefficient."""
    ps = [p.double() for p in case["params"][:-1]]
    ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    for k in range(steps):
        coef = 1.0 if max_norm is None else min(max_norm / (case["norms"][k] + 1e-6), 1.0)
        t = k + 1
        for i, g in enumerate(case["clean"][k]):
            g = g.double() * coef
            ms[i] = ms[i] + (1 - BETAS[0]) * (g - ms[i])
            vs[i] = BETAS[1] * vs[i] + (1 - BETAS[1]) * g * g
            denom = vs[i].sqrt() / (1 - BETAS[1] ** t) ** 0.5 + EPS
            ps[i] = ps[i] - (LR / (1 - BETAS[0] ** t)) * ms[i] / denom
    return ps


def _worst_ulps(ps, ref):
    """Largest |p - ref| over all elements in units of the fp32 spacing at ref."""
    worst = 0.0
    for p, r in zip(ps, ref):
        if r.numel():
            ulp = np.spacing(np.abs(r.numpy()).astype(np.float32)).astype(np.float64)
            worst = max(worst, float(np.max(np.abs(p.detach().cpu().double().numpy() - r.numpy()) / ulp)))
    return worst


def _norm_ulps(norms, case):
    return max(abs(float(n) - r) / float(np.spacing(np.float32(r))) for n, r in zip(norms, case["norms"]))


def _bits(ps, opt):
    out = [p.detach().clone() for p in ps]
    for p in ps:
        st = opt.state.get(p) or {}
        out += [st[k].clone() for k in ("step", "exp_avg", "exp_avg_sq") if k in st]
    return out


def _equal(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))


def test_hygiene_cleans_the_gradients_in_place_and_leaves_them_unclipped(case):
    """The kernels write back the CLEANED gradient only: the clip coefficient is applied inside the update and never stored, so with
    max_norm far below the norm the gradients after the step still equal nan_to_num's, bit for bit."""
    ps, opt, _ = _fused(case, steps=1, max_norm=1.0)
    for p, want in zip(ps[:-1], case["clean"][0]):
        assert torch.equal(p.grad.cpu(), want)
    ps, opt, _ = _fused(case, steps=4, max_norm=None)
    for p, want in zip(ps[:-1], case["clean"][3]):
        assert torch.equal(p.grad.cpu(), want)


def test_gate_closed_changes_nothing_and_open_advances_every_count(case):
    from unopose_amd.optim import FusedAdam

    ps, opt, _ = _fused(case, steps=2, max_norm=1e3)
    before, sd = _bits(ps, opt), opt.state_dict()
    _set_grads(ps, case["grads"][2])
    norm = opt.step(torch.zeros(1, dtype=torch.bool, device="cuda"), 1e3)
    assert opt.launches == 3 and _equal(_bits(ps, opt), before)
    after = opt.state_dict()
    assert _same_tree(after, sd)
    assert all(float(v["step"]) == 2 for v in after["state"].values()) and len(after["state"]) == len(ps) - 1
    assert abs(float(norm) - case["norms"][2]) < 1e-6 * case["norms"][2]  # the norm is produced whatever the gate says
    for p, want in zip(ps[:-1], case["clean"][2]):
        assert torch.equal(p.grad.cpu(), want)  # ... and the gradients have been cleaned
    for flag, count in ((torch.ones(1, dtype=torch.bool, device="cuda"), 3), (torch.ones(1, dtype=torch.uint8, device="cuda"), 4), (None, 5)):
        moving = [p for p in ps[:-1] if p.numel() >= 3]  # (the 1-element gradient is the planted NaN in every step: cleaned to 0, nothing moves)
        prev = _bits(moving, opt)
        _set_grads(ps, case["grads"][count - 1])
        opt.step(flag, 1e3)
        now = _bits(moving, opt)
        assert opt.launches == 3 and len(now) == 4 * len(moving) and all(not torch.equal(x, y) for x, y in zip(now, prev))
        assert all(int(opt.state[p]["step"]) == count for p in ps[:-1])  # the 0-element parameter's count advances too (torch's rule)
    assert not opt.state.get(ps[-1]) and torch.equal(ps[-1].detach().cpu(), case["params"][-1])  # no gradient: no state, no count, no change
    assert isinstance(opt, FusedAdam) and opt.state[ps[0]]["step"].dtype == torch.int32 and opt.state[ps[0]]["step"].is_cuda


@pytest.mark.parametrize("max_norm", MAX_NORMS)
def test_norm_clip_and_update_against_float64(case, max_norm):
    """After 5 steps: worst error per element in ulps of the parameter, and worst error of the returned norm in ulps of the norm, both against
    float64, for the kernels and for nan_to_num + clip_grad_norm_ + torch.optim.Adam(foreach=False) on the same device.  Both round a different
    association of the same fp32 expression; the kernels pass at no more than twice torch's error or 1 ulp, whichever is larger."""
    ref = _adam64(case, max_norm)
    ps, opt, norms = _fused(case, max_norm=max_norm)
    tps, topt, tnorms = _torch_route(case, max_norm)
    mine, theirs = _worst_ulps(ps[:-1], ref), _worst_ulps(tps[:-1], ref)
    mine_n, theirs_n = _norm_ulps(norms, case), _norm_ulps(tnorms, case)
    line = "max_norm %s: parameter error after %d steps, ulps: fused %.3f torch %.3f; norm error, ulps: fused %.3f torch %.3f" % (
        max_norm, STEPS, mine, theirs, mine_n, theirs_n)
    print(line)
    if max_norm == MAX_NORMS[0]:
        with open(os.path.join(ROOT, "profiles", "fused_adam_parity.txt"), "w") as f:
            f.write("tests/test_fused_adam_gpu.py::test_norm_clip_and_update_against_float64, worst errors against float64 (fp32 ulps)\n" + line + "\n")
    assert mine <= max(2 * theirs, 1.0), line
    assert mine_n <= max(2 * theirs_n, 1.0), line
    assert torch.equal(ps[-1].detach().cpu(), case["params"][-1])
    # the moments follow the same rule (a looser check: the bound above is about the parameters; a wrong formula is off by far more than this)
    for p, tp in zip(ps[:-1], tps[:-1]):
        for k in ("exp_avg", "exp_avg_sq"):
            a, b = opt.state[p][k], topt.state[tp][k]
            assert a.shape == b.shape and (a.numel() == 0 or torch.allclose(a, b, rtol=1e-4, atol=1e-4 * float(b.abs().max()))), k


def test_two_runs_from_equal_state_give_equal_bits(case):
    a_ps, a_opt, a_norms = _fused(case, max_norm=1e3)
    b_ps, b_opt, b_norms = _fused(case, max_norm=1e3)
    assert _equal(_bits(a_ps, a_opt), _bits(b_ps, b_opt)) and _equal(a_norms, b_norms)


def test_state_interchange_with_torch_adam(case):
    """3 fused steps -> state_dict() -> torch.optim.Adam -> 2 torch steps, and 3 torch steps -> FusedAdam -> 2 fused steps, on the cleaned
    gradients without clipping: both chains stay within the bound of the update test (twice the error of 5 torch steps, or 1 ulp)."""
    from unopose_amd.optim import FusedAdam

    ref = _adam64(case, None)
    tps, _, _ = _torch_route(case, None)
    bound = max(2 * _worst_ulps(tps[:-1], ref), 1.0)

    def chain(first, second):
        ps = _params(case)
        a = first(ps, lr=LR, betas=BETAS, eps=EPS)
        for k in range(3):
            _set_grads(ps, case["clean"][k])
            a.step()
        b = second(ps, lr=LR, betas=BETAS, eps=EPS)
        b.load_state_dict(a.state_dict())
        for k in range(3, STEPS):
            _set_grads(ps, case["clean"][k])
            b.step()
        steps = [float(st["step"]) for st in b.state_dict()["state"].values()]
        assert steps == [float(STEPS)] * (len(ps) - 1)
        return _worst_ulps(ps[:-1], ref)

    plain = lambda ps, **kw: torch.optim.Adam(ps, foreach=False, **kw)  # noqa: E731
    fused_then_torch, torch_then_fused = chain(FusedAdam, plain), chain(plain, FusedAdam)
    print("interchange, ulps: fused->torch %.3f torch->fused %.3f (bound %.3f)" % (fused_then_torch, torch_then_fused, bound))
    assert fused_then_torch <= bound and torch_then_fused <= bound


def test_twenty_steps_without_a_host_wait_equal_a_synchronised_loop(case):
    """New gradient tensors every step and nothing that waits for the device in between: the pointer tables go through the pinned ring, whose
    slots are reused five times each here; every slot's own event keeps a table from being overwritten before its copy has run."""
    a_ps, a_opt, a_norms = _fused(case, steps=20, max_norm=1e3, sync=False)
    b_ps, b_opt, b_norms = _fused(case, steps=20, max_norm=1e3, sync=True)
    assert _equal(_bits(a_ps, a_opt), _bits(b_ps, b_opt)) and _equal(a_norms, b_norms)
    assert all(int(a_opt.state[p]["step"]) == 20 for p in a_ps[:-1])
