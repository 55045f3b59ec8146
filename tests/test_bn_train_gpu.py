"""GPU: the training-mode BatchNorm2d + ReLU (+ max-pool) kernels of csrc/bn_train.hip against the float64 reference of
tests/bn_train_ref.py on its off-centre data, under its a-priori per-channel tolerances (derived there; test_bn_train_ref_cpu.py
shows that a correct fp32 kernel stays under a quarter of each and that the E[x^2] - E[x]^2 statistics do not pass).  Every element
of every tensor is compared: the builder guarantees that no pre-activation is within rounding of the ReLU threshold and that
every positive row maximum is unique.

Measured on an MI355X with the kernels as they were before the statistics were centred (fp32 sum x, sum x^2; the shift
beta - mean a folded): all 14 cases of this module fail.  Largest error / tolerance per family over the cases, y | dx | running_var:
(16, 1) 0.97 | 1.02 | 1.4;  (64, 1) 24 | 22 | 79;  (-64, 1) 26 | 23 | 49;  (-300, 3) 79 | 81 | 198;  (1000, 1) 481 | 464 | 298;
(1000, 1/2) 394 | 373 | 1170;  (256, 1/16) 2.1e4 | 1.2e6 | 5.1e3;  the constant 1000.0 channel's y 9.4e3 (its statistics are exact:
the rounding of mean * a in the folded shift);  the centred families, (0, 1e-3) and the constant 5.0: at most 0.08.
With the centred statistics every ratio is below 0.12, running_mean (one rounding of the stored value is up to 0.5) below 0.8."""
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_train_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _module(c, eps=1e-5, momentum=0.1, track=True):
    bn = torch.nn.BatchNorm2d(c.x.shape[1], eps=eps, momentum=momentum, track_running_stats=track).cuda().train()
    with torch.no_grad():
        bn.weight.copy_(c.gamma)
        bn.bias.copy_(c.beta)
        if track:
            bn.running_mean.copy_(c.running_mean)
            bn.running_var.copy_(c.running_var)
    return bn


def _run(c, bn):
    """One fused forward + backward of the case on the module -> what the kernels wrote (the saved batch mean included)."""
    from unopose_amd import ops

    x = c.x.cuda().requires_grad_(True)
    y = (ops.bn_relu_maxpool if c.pool else ops.bn_relu)(x, bn)
    assert ("BNReLUMaxPoolTrain" if c.pool else "BNReLUTrain") in type(y.grad_fn).__name__  # the fused path was taken
    mean = y.grad_fn.saved_tensors[3].clone()
    bn.zero_grad()
    y.backward(c.dy.cuda())
    return SimpleNamespace(y=y.detach(), dx=x.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad, mean=mean,
                           running_mean=bn.running_mean, running_var=bn.running_var)


def _check(c, r, tol, got):
    """Everything `got` carries within its tolerance, on every channel; the constant channels and the ReLU mask on their own."""
    ratio = R.ratios(got, r, tol)
    print({k: [round(float(v), 3) for v in t] for k, t in ratio.items()})
    for k, t in ratio.items():
        assert float(t.max()) <= 1.0, (k, [(ch, R.family(ch)[:2], round(float(v), 2)) for ch, v in enumerate(t) if v > 1.0])
    # constant channels: the saved mean is the constant, bit for bit (y and dx: the tighter of their two tolerances, in `tol`)
    const = [ch for ch in range(c.x.shape[1]) if R.is_const(ch)]
    assert torch.equal(got.mean.cpu()[const].double(), r.mean[const]), (got.mean.cpu()[const], r.mean[const])
    # mask agreement: the forward's zeros are the reference's (the guard band leaves no excuse), and wherever the kernel's y is 0
    # its dx is the reference's: fails if forward, backward and pool ever evaluate the pre-activation by different expressions
    dead = got.y.cpu() == 0
    assert torch.equal(dead, r.y == 0)
    dead = (dead[..., None] if c.pool else dead).expand_as(r.dx)
    e = ((got.dx.cpu().double() - r.dx).abs() * dead).amax((0, 2, 3))
    assert bool((e <= tol.dx).all()), e / tol.dx


@pytest.mark.parametrize("shape,seed", R.CASES_BN)
def test_bn_relu_train_on_off_centre_channels(shape, seed):
    """relu(batch_norm(x)): two chunks with a ragged second one, two whole chunks, one ragged chunk with most lanes idle."""
    c, r, tol = R.case_and_reference(shape, seed, False)
    bn = _module(c)
    _check(c, r, tol, _run(c, bn))
    assert int(bn.num_batches_tracked) == 1


@pytest.mark.parametrize("shape,seed", R.CASES_POOL)
def test_bn_relu_maxpool_train_on_off_centre_channels(shape, seed):
    """max_s relu(batch_norm(x)) from the pooled gradient: every row width S, N not a multiple of the rows per wave, and 134400
    rows, past the 8192-workgroup grid cap (the row loop takes a second trip)."""
    c, r, tol = R.case_and_reference(shape, seed, True)
    bn = _module(c)
    _check(c, r, tol, _run(c, bn))
    assert int(bn.num_batches_tracked) == 1


@pytest.mark.parametrize("pool", [False, True])
def test_cumulative_average_over_two_calls_and_fresh_data_on_one_module(pool):
    """momentum=None: the first call updates the running statistics with momentum 1, the second, on fresh data, with 1/2.  The
    second call's outputs and gradients are those of its own data: saved statistics and workspace carry nothing over."""
    first, fresh = R.STATE_SEEDS[pool][:2]
    ca, cb = R.make_case(R.STATE_SHAPE, first, pool), R.make_case(R.STATE_SHAPE, fresh, pool)
    bn = _module(ca, momentum=None)
    ra = R.reference(ca.x, ca.gamma, ca.beta, ca.dy, 1e-5, 1.0, ca.running_mean, ca.running_var, pool)
    _check(ca, ra, R.tolerances(ca, ra), _run(ca, bn))
    with torch.no_grad():
        bn.weight.copy_(cb.gamma)
        bn.bias.copy_(cb.beta)
    rb = R.reference(cb.x, cb.gamma, cb.beta, cb.dy, 1e-5, 0.5, ra.running_mean, ra.running_var, pool)
    _check(cb, rb, R.tolerances(cb, rb), _run(cb, bn))
    assert int(bn.num_batches_tracked) == 2


@pytest.mark.parametrize("pool", [False, True])
def test_without_running_statistics(pool):
    """track_running_stats=False: the buffers are None, a null pointer goes into the kernel."""
    c = R.make_case(R.STATE_SHAPE, R.STATE_SEEDS[pool][0], pool)
    bn = _module(c, track=False)
    r = R.reference(c.x, c.gamma, c.beta, c.dy, 1e-5, pool=pool)
    got = _run(c, bn)
    assert bn.running_mean is None and bn.running_var is None and bn.num_batches_tracked is None
    got.running_mean = got.running_var = None
    _check(c, r, R.tolerances(c, r), got)


@pytest.mark.parametrize("pool", [False, True])
def test_non_default_eps_and_momentum(pool):
    """eps = 1e-3 (data and beta built for it: the tiny-scale and constant channels are all eps) and momentum = 0.3."""
    c = R.make_case(R.STATE_SHAPE, R.STATE_SEEDS[pool][2], pool, eps=1e-3)
    bn = _module(c, eps=1e-3, momentum=0.3)
    r = R.reference(c.x, c.gamma, c.beta, c.dy, 1e-3, 0.3, c.running_mean, c.running_var, pool)
    _check(c, r, R.tolerances(c, r), _run(c, bn))
    assert int(bn.num_batches_tracked) == 1
