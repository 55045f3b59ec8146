"""CPU: the float64 reference of the match head (tests/match_head_ref.py) pinned against the code it stands for, before any kernel is
judged by it: losses.overlap_losses for the loss values, the saliency_pair fallback expression, max(2)[1], and torch autograd for its G."""
import torch
import torch.nn.functional as F

import match_head_ref as ref
from train_case import random_block_outputs


def _case():
    """(3, 60, 50) from random_block_outputs: its points give the labels; unit features, logits and upstream gradients are drawn here."""
    from unopose_amd.losses import match_targets

    g = torch.Generator().manual_seed(7)
    case = random_block_outputs(g)
    B, n1, n2 = 3, 60, 50
    a = F.normalize(torch.randn(B, n1 + 1, 256, generator=g, dtype=torch.float64), dim=2)
    b = F.normalize(torch.randn(B, n2 + 1, 256, generator=g, dtype=torch.float64), dim=2)
    s1 = torch.randn(B, n1, 1, generator=g, dtype=torch.float64)
    s2 = torch.randn(B, n2, 1, generator=g, dtype=torch.float64)
    tg = match_targets(case["p1"].double(), case["p2"].double(), case["R"].double(), case["t"].double(), 0.15, 0.15, torch.float64)
    gs = [torch.randn(B, generator=g, dtype=torch.float64), torch.randn(B, n1, generator=g, dtype=torch.float64),
          torch.randn(B, n2, generator=g, dtype=torch.float64)]
    return case, a, b, s1, s2, tg, gs


def test_reference_equals_overlap_losses_saliency_pair_and_argmax():
    from unopose_amd import ops
    from unopose_amd.losses import overlap_losses

    case, a, b, s1, s2, tg, _ = _case()
    tau = 10.0
    l1, l2 = tg["l1"], tg["l2"]
    assert (l1 == 0).any() and (l1 > 0).any() and (l2 == 0).any() and (l2 > 0).any()
    f = ref.forward(a, b, s1, s2, l1, l2, tau)
    S = f["S"]
    # the loss values: overlap_losses on the materialised similarity (float64 in, its fp32 island out)
    ep = overlap_losses({}, [S], [case["score"][0].double()], [case["sal"][0].double()], case["p1"].double(), case["p2"].double(),
                        case["R"].double(), case["t"].double(), prefix="x")
    assert torch.allclose(ep["x_atten_loss0"].double(), f["loss"], rtol=2e-6, atol=0)
    assert torch.allclose(ops.infonce_two_way(S, l1, l2).double(), f["loss"], rtol=2e-6, atol=0)
    # and in float64 exactly the two cross entropies
    ce = 0.5 * (F.cross_entropy(S.transpose(1, 2)[:, :, 1:], l1, reduction="none").mean(1) + F.cross_entropy(S[:, :, 1:], l2, reduction="none").mean(1))
    assert torch.allclose(ce, f["loss"], rtol=1e-13, atol=0)
    # the saliency pair: the fallback expression of ops.saliency_pair
    inner = S[:, 1:, 1:]
    m1 = torch.matmul(F.softmax(inner, dim=2), s2).squeeze(2)
    m2 = torch.matmul(F.softmax(inner.transpose(1, 2), dim=2), s1).squeeze(2)
    assert torch.allclose(m1, f["m1"], rtol=1e-12, atol=1e-14) and torch.allclose(m2, f["m2"], rtol=1e-12, atol=1e-14)
    p1, p2 = ops.saliency_pair(S, s1, s2)
    assert torch.equal(p1.squeeze(2), m1) and torch.equal(p2.squeeze(2), m2)
    # the arg max and the monitoring scalars it feeds
    assert torch.equal(f["pred"], S[:, 1:, :].max(2)[1])
    assert torch.equal(ep["x_acc"], (f["pred"] == l1).float().mean(1))


def test_reference_gradient_formula_equals_autograd():
    _, a, b, s1, s2, tg, (gL, g1, g2) = _case()
    tau = 10.0
    l1, l2 = tg["l1"], tg["l2"]
    leaves = [t.clone().requires_grad_(True) for t in (a, b, s1, s2)]
    f = ref.forward(*leaves, l1, l2, tau)
    ((f["loss"] * gL).sum() + (f["m1"] * g1).sum() + (f["m2"] * g2).sum()).backward()
    f0 = ref.forward(a, b, s1, s2, l1, l2, tau)
    got = ref.backward(a, b, s1, s2, l1, l2, tau, f0, gL, g1, g2)
    for name, leaf in zip(("da", "db", "ds1", "ds2"), leaves):
        want = leaf.grad.reshape(got[name].shape)
        assert torch.allclose(got[name], want, rtol=1e-10, atol=1e-13 * want.abs().max().item() + 1e-15), name
    # G itself: autograd through the materialised matrix
    S = f0["S"].clone().requires_grad_(True)
    B, n1, n2 = 3, 60, 50
    Lr, Lc = torch.logsumexp(S[:, 1:, :], 2), torch.logsumexp(S[:, :, 1:], 1)
    pr = torch.gather(S[:, 1:, :], 2, l1.unsqueeze(2)).squeeze(2)
    pc = torch.gather(S[:, :, 1:], 1, l2.unsqueeze(1)).squeeze(1)
    loss = 0.5 * ((Lr - pr).mean(1) + (Lc - pc).mean(1))
    m1 = torch.matmul(F.softmax(S[:, 1:, 1:], 2), s2).squeeze(2)
    m2 = torch.matmul(F.softmax(S[:, 1:, 1:].transpose(1, 2), 2), s1).squeeze(2)
    ((loss * gL).sum() + (m1 * g1).sum() + (m2 * g2).sum()).backward()
    G = ref.grad_S(f0, s1, s2, l1, l2, gL, g1, g2)
    assert torch.allclose(G, S.grad, rtol=1e-10, atol=1e-15)
