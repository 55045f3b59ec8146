"""The float64 reference of the match head (ops.match_head / csrc/match_train.hip), written with the materialised similarity.

For unit rows a (B, R, 256), b (B, C, 256) (row / column 0 = the background token), S = tau a b^T, overlap logits s1 (B, n1, 1),
s2 (B, n2, 1) and labels l1 (B, n1) in [0, n2], l2 (B, n2) in [0, n1] (0 = background):
    rows i >= 1:     Lr_i = lse_{j >= 0} S_ij, Fr_i = lse_{j >= 1} S_ij, m1_i = sum_{j >= 1} exp(S_ij - Fr_i) s2_j, pred_i = argmax_{j >= 0} S_ij
    columns j >= 1:  Lc_j, Fc_j the same over i, m2_j = sum_{i >= 1} exp(S_ij - Fc_j) s1_i
    loss_b = 0.5 (mean_{i >= 1} (Lr_i - S_{i, l1_i}) + mean_{j >= 1} (Lc_j - S_{l2_j, j}))
and the backward through G = dS (`backward`).  tests/test_match_head_ref_cpu.py pins this module against losses.overlap_losses, the
saliency_pair expression, max(2)[1] and torch autograd before any kernel is judged by it."""
import torch


def similarity(a, b, tau):
    return tau * (a.double() @ b.double().transpose(1, 2))


def forward(a, b, s1, s2, l1, l2, tau):
    """-> dict(S, Lr, Fr, m1, pred, Lc, Fc, m2, loss), float64 (pred int64)."""
    S = similarity(a, b, tau)
    B, n1, n2 = S.shape[0], S.shape[1] - 1, S.shape[2] - 1
    v1, v2 = s1.double().reshape(B, n1), s2.double().reshape(B, n2)
    Lr = torch.logsumexp(S[:, 1:, :], dim=2)
    Fr = torch.logsumexp(S[:, 1:, 1:], dim=2)
    m1 = (torch.exp(S[:, 1:, 1:] - Fr.unsqueeze(2)) * v2.unsqueeze(1)).sum(2)
    Lc = torch.logsumexp(S[:, :, 1:], dim=1)
    Fc = torch.logsumexp(S[:, 1:, 1:], dim=1)
    m2 = (torch.exp(S[:, 1:, 1:] - Fc.unsqueeze(1)) * v1.unsqueeze(2)).sum(1)
    pr = torch.gather(S[:, 1:, :], 2, l1.unsqueeze(2)).squeeze(2)
    pc = torch.gather(S[:, :, 1:], 1, l2.unsqueeze(1)).squeeze(1)
    loss = 0.5 * ((Lr - pr).mean(1) + (Lc - pc).mean(1))
    return dict(S=S, Lr=Lr, Fr=Fr, m1=m1, pred=S[:, 1:, :].max(2)[1], Lc=Lc, Fc=Fc, m2=m2, loss=loss)


def grad_S(f, s1, s2, l1, l2, gL, g1, g2):
    """G = d(sum_b gL_b loss_b + sum g1 m1 + sum g2 m2) / dS from the forward's statistics `f` (the issue's formula), float64."""
    S = f["S"]
    B, n1, n2 = S.shape[0], S.shape[1] - 1, S.shape[2] - 1
    v1, v2 = s1.double().reshape(B, n1), s2.double().reshape(B, n2)
    gL, g1, g2 = gL.double().reshape(B, 1, 1), g1.double().reshape(B, n1, 1), g2.double().reshape(B, 1, n2)
    G = torch.zeros_like(S)
    d1 = torch.zeros(B, n1, n2 + 1, dtype=torch.float64, device=S.device).scatter_(2, l1.unsqueeze(2), 1.0)
    d2 = torch.zeros(B, n1 + 1, n2, dtype=torch.float64, device=S.device).scatter_(1, l2.unsqueeze(1), 1.0)
    G[:, 1:, :] += gL / (2 * n1) * (torch.exp(S[:, 1:, :] - f["Lr"].unsqueeze(2)) - d1)
    G[:, :, 1:] += gL / (2 * n2) * (torch.exp(S[:, :, 1:] - f["Lc"].unsqueeze(1)) - d2)
    inner = S[:, 1:, 1:]
    G[:, 1:, 1:] += g1 * torch.exp(inner - f["Fr"].unsqueeze(2)) * (v2.unsqueeze(1) - f["m1"].unsqueeze(2))
    G[:, 1:, 1:] += g2 * torch.exp(inner - f["Fc"].unsqueeze(1)) * (v1.unsqueeze(2) - f["m2"].unsqueeze(1))
    return G


def backward(a, b, s1, s2, l1, l2, tau, f, gL, g1, g2):
    """-> dict(da, db, ds1, ds2), float64, from G."""
    S = f["S"]
    B, n1, n2 = S.shape[0], S.shape[1] - 1, S.shape[2] - 1
    G = grad_S(f, s1, s2, l1, l2, gL, g1, g2)
    inner = S[:, 1:, 1:]
    ds2 = (g1.double().reshape(B, n1, 1) * torch.exp(inner - f["Fr"].unsqueeze(2))).sum(1)
    ds1 = (g2.double().reshape(B, 1, n2) * torch.exp(inner - f["Fc"].unsqueeze(1))).sum(2)
    return dict(da=tau * (G @ b.double()), db=tau * (G.transpose(1, 2) @ a.double()), ds1=ds1, ds2=ds2)


def reference(a, b, s1, s2, l1, l2, tau, gL, g1, g2):
    f = forward(a, b, s1, s2, l1, l2, tau)
    f.update(backward(a, b, s1, s2, l1, l2, tau, f, gL, g1, g2))
    return f
