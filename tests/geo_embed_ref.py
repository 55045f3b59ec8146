"""Float64 reference, with a derived error bound, of the geometric structure embedding (csrc/embed.hip: geo_knn_kernel, geo_embed_kernel,
geo_embed_table_kernel and its backward), GeometricStructureEmbedding.forward (transformer.py:303-350):

    E[b,i,j,:] = proj_d(sinus(|p_i - p_j| / sigma_d)) + reduce_k proj_a(sinus(angle(p_knn(i,k) - p_i, p_j - p_i) * factor_a)) + biases

Everything is torch float64 computed from the fp32 inputs with direct differences (the diagonal is exactly distance 0, angle 0), in chunks
of rows, on whatever device the inputs are on.  The neighbour list is an argument: the GPU tests validate the kernel's own list
(`knn_valid`) and hand it in, so that a legitimate near-tie never shows up as an embedding error.

The bound is carried next to the values; every constant is derived here or taken from the project, none is fitted to a kernel's output.
u = 2^-24 (one correctly rounded fp32 operation, relative).

  distance index x_d = sqrt(dx^2 + dy^2 + dz^2) / sigma_d: three subtractions (u each, relative, per component: 2 u on d^2), three
    products and two additions of positive terms (3 u), the square root halves that (2.5 u) and adds its own 1 ulp (2 u), the division
    2.5 ulp (5 u), sigma_d as a float (u), the product with the frequency (u): 11.5 u, taken as E_DIST = 14 u, relative to x_d.  x_d = 0
    (diagonal, duplicated points) is exact.
  angle = atan2(|r x a|, r.a): the components of r and a carry u each; a cross-product component is two products and a subtraction,
    (2 u + u + u)(|r_y a_z| + |r_z a_y|), as a vector <= 4 sqrt(3) u |r||a|; its norm adds 4.5 u |r||a|; the dot product
    (2 u + u + 2 u) |r||a|.  s^2 + c^2 = |r|^2 |a|^2, so the angle moves by at most sqrt(11.5^2 + 5^2) u = 12.5 u rad -- atan2 is
    well-conditioned except at r = 0 or a = 0, where kernels and reference all give exactly 0.  atan2f itself 2 ulp of <= pi (12.6 u),
    the product with factor_a, factor_a as a float and the product with the frequency 3 u pi: 34.5 u, taken as E_ANGLE = 36 u rad.
  Both propagate through the per-channel Lipschitz constant L[c] = sum_f div_f (|W[c,2f]| + |W[c,2f+1]|).

  arithmetic, with A[c] = sum_f (|W[c,2f]| + |W[c,2f+1]|) >= sum |W||s|:
    split   U_BF16X3 = 3 * 2^-17 of A (the budget of test_linear_f32x3_vs_fp64_reference: hi + lo of each operand exact to 2^-18, the
            dropped lo * lo term 2^-18, the rest for the 48 accumulator roundings of the 16 k-steps x 3 MFMAs and the sums inside them),
            plus the sin / cos error embed.hip states: 1e-7 (sincos_cw; frequencies 0-63, and 64-127 at an index >= 32), 1e-8 (sincos_small)
    bf16    operand rounding 2^-9 on each side ((2 * 2^-9 + 2^-18) A), the hardware sin / cos 1e-6, U_BF16X3 for the accumulation
    table   the interpolation bounds embed.hip states, 0.0234 h^4 max|f''''| resp. 0.0235 h^6 max|f''''''| at h = 1/4 with
            max|f^(p)| <= sum_f div_f^p (|W_sin| + |W_cos|); the fp32 rounding of a table entry (u M, M[c] = max |f[c]| over the table's
            range, evaluated here from the weights), NP fma roundings and 2 NP roundings in every Lagrange weight, all times the
            weights' absolute sum LEBESGUE[NP]: (3 NP + 1) u LEBESGUE M.  A distance index past the table takes the defining sum:
            fp32 sinf / cosf (2 ulp: 4 u absolute) and 256 + 128 accumulation roundings, 388 u A.
  the epilogue d + reduce(a) + (b_d + b_a): 5 u (M_d + M_a + |b_d| + |b_a|).  Max over k is 1-Lipschitz, mean divides by three what it
  summed: both keep the per-term bound.  A bf16 result adds half a bf16 ulp of the value: 2^(floor(log2 v) - 8) at v = |ref| + bound.

Nothing here is used by the package.  The test clouds (`make_cloud`), the case list of test_geo_embedding_gpu.py (`CASES`), the float32
restatement of each route (`emulate`) and the mutants the tests must be able to tell from the truth are here too, so that
test_geo_embed_ref_cpu.py can check the teeth of the GPU tests without a GPU."""
import math
from types import SimpleNamespace

import numpy as np
import torch

F64 = torch.float64
U = 2.0 ** -24
U_BF16X3 = 3 * 2.0 ** -17
U_BF16 = 2.0 ** -9
SLACK = 8 * U          # knn_valid: three products and two additions per distance^2, <= 3 ulp on each side of a comparison
E_DIST = 14 * U        # relative error of a distance index
E_ANGLE = 36 * U       # absolute error of an angle, rad
HINV = 4               # table nodes per unit index (csrc/embed.hip GT_HINV)
D_LDS, D_TABLE = 16.0, 64.0   # distance indices: LDS rows below 16, global rows up to 64, the defining sum past it
INTERP_C = {4: 0.0234, 6: 0.0235}   # embed.hip: error <= C h^NP max|d^NP f / dx^NP|
SIGMA_D, SIGMA_A = 0.2, 15.0
MIN_GAP = 1e-5         # smallest relative gap of neighbour distances^2 at which exact equality of the lists is demanded
MAX_BWD_INDEX = 60.0   # the backward refuses (device assert) indices past 64: its clouds stay below this
ROWS_PER_CHUNK = 1 << 15

MUTANTS = ("tie_second", "self_included", "hi_only", "four_for_six", "diag_pi", "drop_tail", "shift_j", "mean_for_max", "lds_row_for_global")


# ------------------------------------------------------------------------------------------------------------ module and clouds
def make_module(regime="default", reduction="max", seed=3):
    """GeometricStructureEmbedding as test_geo_table_cpu.py builds it; `trained`: weights x 4, well above the 1/16 of the default init."""
    from unopose_amd.model.modules import GeometricStructureEmbedding

    torch.manual_seed(seed)
    m = GeometricStructureEmbedding(SimpleNamespace(hidden_dim=256, sigma_d=SIGMA_D, sigma_a=SIGMA_A, angle_k=3, reduction_a=reduction))
    if regime == "trained":
        with torch.no_grad():
            m.proj_d.weight.mul_(4.0)
            m.proj_a.weight.mul_(4.0)
    return m


RING_RADII = (16.0, 64.0, 80.0, 15.99, 64.3, 16.01, 63.9)      # distance indices from point 0 (the steps first: small n keeps them)
RING_RADII_BWD = (16.0, 55.0, 47.9, 15.99, 30.0, 16.01)


def _unit(v):
    return v / v.norm(dim=-1).max()


def make_cloud(kind, n, seed):
    """One test cloud (n,3) fp32 on the CPU."""
    g = torch.Generator().manual_seed(seed)

    def rand(*s):
        return torch.rand(*s, generator=g, dtype=F64)

    if kind == "random":
        p = _unit(rand(n, 3) - 0.5)
    elif kind == "bg":       # what the model feeds: the background token in front of a radius-normalised cloud
        p = torch.cat([torch.ones(1, 3, dtype=F64), _unit(rand(n - 1, 3) - 0.5)])
    elif kind == "object":   # a noisy ellipsoid surface
        v = torch.randn(n, 3, generator=g, dtype=F64)
        v = v / v.norm(dim=1, keepdim=True) * torch.tensor([1.0, 0.6, 0.35], dtype=F64) + 0.01 * torch.randn(n, 3, generator=g, dtype=F64)
        p = _unit(v - v.mean(0))
    elif kind == "lattice":  # integer coordinates x 2^-4: every fp32 operation on them is exact; duplicates and many ties
        p = torch.randint(0, 6, (n, 3), generator=g).to(F64) / 16.0
        c = max(1, n // 8)
        p[n - c:] = p[:c]
    elif kind == "dup_heavy":
        p = _unit(rand(n, 3) - 0.5)
        h = n // 2
        p[n - h:] = p[:h]
    elif kind == "line":     # exactly collinear in fp32: cross products are exactly 0, the angles exactly 0 and pi
        k = torch.randperm(4 * n, generator=g)[:n].to(F64) - 2 * n
        p = k[:, None] * torch.tensor([1.0, 2.0, 2.0], dtype=F64) * 2.0 ** -10 + torch.tensor([0.25, -0.125, 0.5], dtype=F64)
    elif kind in ("rings", "rings_bwd"):
        radii = RING_RADII if kind == "rings" else RING_RADII_BWD
        m = min(len(radii), n - 1)
        # directions within 20 degrees of one axis: two ring points are never farther apart than the larger radius
        d = torch.full((m, 3), 3.0 ** -0.5, dtype=F64) + (rand(m, 3) - 0.5) * 0.4
        d = d / d.norm(dim=1, keepdim=True)
        ring = d * (torch.tensor(radii[:m], dtype=F64) * SIGMA_D)[:, None]
        fill = _unit(rand(n - 1 - m, 3) - 0.5) * 0.6 if n - 1 - m > 0 else torch.zeros(0, 3, dtype=F64)
        p = torch.cat([torch.zeros(1, 3, dtype=F64), ring, fill])
    elif kind == "wide":     # cube of side 6: distance indices up to ~52
        p = (rand(n, 3) - 0.5) * 6.0
    else:
        raise ValueError(kind)
    assert p.shape == (n, 3)
    return p.float()


SEED0 = 100


def make_batch(kind, B, n, seed=SEED0):
    """(B,n,3): clouds of seeds seed + 1000 b + n"""
    return torch.stack([make_cloud(kind, n, seed + 1000 * b + n) for b in range(B)])


# ------------------------------------------------------------------------------------------------------------ neighbours
def _d2(points):
    p = points.to(F64)
    return ((p[:, :, None, :] - p[:, None, :, :]) ** 2).sum(-1)


def knn_exact(points, ignore_ties=False):
    """The 3 nearest neighbours of every point of (B,n,3) in float64 from direct differences, self excluded by index, ordered by
    (distance^2, index): (knn (B,n,3) int32, the smallest relative gap between adjacent distances^2 among each row's first four
    candidates).  `ignore_ties`: exact ties (bit-identical points give bit-identical fp32 distances too) do not count as gaps."""
    d2 = _d2(points)
    n = d2.shape[1]
    d2 = d2.masked_fill(torch.eye(n, dtype=torch.bool, device=d2.device), float("inf"))
    val, idx = torch.sort(d2, dim=2, stable=True)
    v = val[:, :, :min(4, n - 1)]
    hi, lo = v[:, :, 1:], v[:, :, :-1]
    gap = torch.where(hi > 0, (hi - lo) / hi.clamp(min=1e-300), torch.zeros_like(hi))
    if ignore_ties:
        gap = gap.masked_fill(hi == lo, float("inf"))
    return idx[:, :, :3].to(torch.int32), float(gap.min())


def knn_valid(points, knn, slack=SLACK):
    """(B,n) bool: the three indices are distinct and not the row's own, in non-decreasing float64 distance within `slack` (relative), and no
    unlisted point is closer than the third by more than `slack`."""
    d2 = _d2(points)
    B, n, _ = d2.shape
    k = knn.long()
    own = torch.arange(n, device=d2.device)[None, :, None]
    ok = ((k >= 0) & (k < n) & (k != own)).all(-1) & (k[..., 0] != k[..., 1]) & (k[..., 0] != k[..., 2]) & (k[..., 1] != k[..., 2])
    kc = k.clamp(0, n - 1)
    dk = torch.gather(d2, 2, kc)
    ok &= (dk[..., 0] <= dk[..., 1] * (1 + slack)) & (dk[..., 1] <= dk[..., 2] * (1 + slack))
    listed = torch.zeros(B, n, n, dtype=torch.bool, device=d2.device).scatter_(2, kc, True) | torch.eye(n, dtype=torch.bool, device=d2.device)
    rest = d2.masked_fill(listed, float("inf")).amin(2)
    return ok & (rest * (1 + slack) >= dk[..., 2])


def knn_mutant(points, name):
    """tie_second: the larger index wins a tie; self_included: the point itself is its first neighbour."""
    d2 = _d2(points)
    n = d2.shape[1]
    if name == "self_included":
        d2 = d2.masked_fill(torch.eye(n, dtype=torch.bool, device=d2.device), -1.0)
        return torch.sort(d2, dim=2, stable=True)[1][:, :, :3].to(torch.int32)
    assert name == "tie_second"
    d2 = d2.masked_fill(torch.eye(n, dtype=torch.bool, device=d2.device), float("inf"))
    idx = torch.sort(d2.flip(2), dim=2, stable=True)[1]
    return (n - 1 - idx)[:, :, :3].to(torch.int32)


# ------------------------------------------------------------------------------------------------------------ float64 reference
def _params(module):
    return float(module.sigma_d), float(module.factor_a), module.embedding.div_term.detach().to(F64)


def _indices(p, knn, i0, i1, sigma_d, factor_a):
    """Rows i0..i1 of one cloud p (n,3), in p's dtype: x_d (r,n), x_a (r,n,3)"""
    pi = p[i0:i1]
    a = p[None, :, :] - pi[:, None, :]                       # anchor = p_j - p_i
    xd = a.pow(2).sum(-1).sqrt() / sigma_d
    rv = p[knn[i0:i1].long()] - pi[:, None, :]               # ref = p_knn - p_i  (r,3,3)
    r, n = a.shape[:2]
    re, ae = rv[:, None, :, :].expand(r, n, 3, 3), a[:, :, None, :].expand(r, n, 3, 3)
    s = torch.cross(re, ae, dim=-1).pow(2).sum(-1).sqrt()
    c = (re * ae).sum(-1) + 0.0                              # (+0: atan2(0, +0) = 0 where the anchor is 0)
    return xd, torch.atan2(s, c) * factor_a


def _sinus(x, div):
    om = x.unsqueeze(-1) * div
    return torch.stack([torch.sin(om), torch.cos(om)], dim=-1).reshape(*x.shape, -1)


def distance_index64(points, module):
    return _d2(points).sqrt() / float(module.sigma_d)


def embedding64(points, module, knn, reduction=None, terms=False):
    """(B,n,n,256) float64; with `terms` also the three angle terms (B,n,n,3,256) (small clouds only)."""
    sigma_d, factor_a, div = _params(module)
    div = div.to(points.device)
    reduction = reduction or module.reduction_a
    Wd, Wa = module.proj_d.weight.detach().to(points.device, F64), module.proj_a.weight.detach().to(points.device, F64)
    bias = (module.proj_d.bias.detach().to(F64) + module.proj_a.bias.detach().to(F64)).to(points.device)
    p = points.to(F64)
    B, n, _ = p.shape
    out = torch.empty(B, n, n, 256, dtype=F64, device=p.device)
    tm = torch.empty(B, n, n, 3, 256, dtype=F64, device=p.device) if terms else None
    step = max(1, ROWS_PER_CHUNK // n)
    for b in range(B):
        for i0 in range(0, n, step):
            i1 = min(n, i0 + step)
            xd, xa = _indices(p[b], knn[b], i0, i1, sigma_d, factor_a)
            a = _sinus(xa, div) @ Wa.t()
            if terms:
                tm[b, i0:i1] = a
            out[b, i0:i1] = _sinus(xd, div) @ Wd.t() + (a.amax(2) if reduction == "max" else a.mean(2)) + bias
    return (out, tm) if terms else out


def composite64(p64, knn, m64, reduction):
    """The op-by-op composite (ops.geo_embedding_torch, transformer.py:303-350) in float64 under autograd: p64 (B,n,3) float64, knn (B,n,3)
    int64, m64 the module in float64."""
    B, n, _ = p64.shape
    dist = torch.cdist(p64, p64)
    knn_pts = torch.gather(p64.unsqueeze(1).expand(B, n, n, 3), 2, knn.unsqueeze(3).expand(B, n, 3, 3))
    rv = (knn_pts - p64.unsqueeze(2)).unsqueeze(2).expand(B, n, n, 3, 3)
    av = (p64.unsqueeze(1) - p64.unsqueeze(2)).unsqueeze(3).expand(B, n, n, 3, 3)
    a_idx = torch.atan2(torch.linalg.norm(torch.cross(rv, av, dim=-1), dim=-1), (rv * av).sum(-1)) * m64.factor_a
    div = m64.embedding.div_term

    def sinus(idx):
        om = idx.unsqueeze(-1) * div
        return torch.stack([torch.sin(om), torch.cos(om)], dim=-1).reshape(*idx.shape, -1)

    a_emb = m64.proj_a(sinus(a_idx))
    return m64.proj_d(sinus(dist / m64.sigma_d)) + (a_emb.max(dim=3)[0] if reduction == "max" else a_emb.mean(dim=3))


# ------------------------------------------------------------------------------------------------------------ the table rule
def lagrange_weights(f, npoint):
    """Weights (len(f), npoint) of the nodes -(npoint / 2 - 1) .. npoint / 2 at f in [0, 1) (embed.hip gt_weights)."""
    nodes = np.arange(npoint) - (npoint // 2 - 1)
    w = np.ones((len(f), npoint))
    for j in range(npoint):
        for mth in range(npoint):
            if mth != j:
                w[:, j] *= (f - nodes[mth]) / (nodes[j] - nodes[mth])
    return w


def table_interp(tab, x, npoint, table_npoint=None, row_shift=0):
    """The kernel's interpolation rule: row r of `tab` holds x = (r - (NP / 2 - 1)) / 4, NP-point Lagrange on the nodes around x.
    `table_npoint` (mutants): the order the table was laid out for, when it is not the order of the weights; `row_shift`: rows read off by that."""
    shift = ((table_npoint or npoint) // 2 - 1) - (npoint // 2 - 1) + row_shift
    t = x * float(HINV)
    r0 = np.floor(t).astype(int)
    w = lagrange_weights(t - r0, npoint)
    out = np.zeros((len(x), tab.shape[1]))
    for j in range(npoint):
        out += w[:, j:j + 1] * tab[r0 + j + shift]
    return out


def _lebesgue(npoint):
    return float(np.abs(lagrange_weights(np.linspace(0.0, 1.0, 2001), npoint)).sum(1).max())


LEBESGUE = {4: _lebesgue(4), 6: _lebesgue(6)}


def tables64(module, npoint):
    """(table_d, table_a) float64 on the grid x = (r - (npoint / 2 - 1)) / 4, the layout of ops._geo_tables."""
    _, factor_a, div = _params(module)
    lo = npoint // 2 - 1
    rows_a = int(math.floor(math.pi * factor_a * HINV)) + npoint + 1
    rows_d = int(D_TABLE) * HINV + npoint

    def table(rows, lin):
        x = (torch.arange(rows, dtype=F64) - float(lo)) / HINV
        return _sinus(x, div.cpu()) @ lin.weight.detach().cpu().to(F64).t()

    return table(rows_d, module.proj_d), table(rows_a, module.proj_a)


# ------------------------------------------------------------------------------------------------------------ bound
def _channel_constants(module):
    _, factor_a, div = _params(module)
    div = div.cpu()
    c = {}
    for name, lin, top in (("d", module.proj_d, D_TABLE + 2.0), ("a", module.proj_a, math.pi * factor_a + 2.0)):
        W = lin.weight.detach().cpu().to(F64).abs()
        aw = W[:, 0::2] + W[:, 1::2]                      # (256 channels, 128 frequencies)
        c["A_" + name] = aw.sum(1)
        c["Alo_" + name], c["Ahi_" + name] = aw[:, :64].sum(1), aw[:, 64:].sum(1)
        c["L_" + name] = (aw * div).sum(1)
        c["D4_" + name], c["D6_" + name] = (aw * div ** 4).sum(1), (aw * div ** 6).sum(1)
        x = torch.arange(-1.0, top, 1.0 / 16, dtype=F64)
        f = _sinus(x, div) @ lin.weight.detach().cpu().to(F64).t()
        c["M_" + name] = f.abs().amax(0) + c["L_" + name] / 32   # max |f| over the range: the grid's maximum + L * half its spacing
        c["b_" + name] = lin.bias.detach().cpu().to(F64).abs()
    return c


def bound(points, module, knn, route, out_bf16=False, ref=None):
    """(B,n,n,256) float64: the error a correct kernel of `route` (split, bf16, table4, table6) may have against `embedding64`.  Only the
    distance index varies over the elements: the angle terms are bounded by their worst case (`knn` does not enter).  `ref` (the values):
    needed for a bf16 result."""
    assert math.pi * float(module.factor_a) < 32.0
    dev = points.device
    c = {k: v.to(dev) for k, v in _channel_constants(module).items()}
    xd = distance_index64(points, module).unsqueeze(-1)     # (B,n,n,1)
    total = c["L_d"] * (E_DIST * xd) + c["L_a"] * (E_ANGLE * float(module.factor_a))
    total = total + 5 * U * (c["M_d"] + c["M_a"] + c["b_d"] + c["b_a"])
    if route == "split":
        hi_err = torch.where(xd < 32.0, 1e-8, 1e-7)
        total = total + U_BF16X3 * (c["A_d"] + c["A_a"]) + 1e-7 * (c["Alo_d"] + c["Alo_a"]) + hi_err * c["Ahi_d"] + 1e-8 * c["Ahi_a"]
    elif route == "bf16":
        total = total + (2 * U_BF16 + U_BF16 ** 2 + 1e-6 + U_BF16X3) * (c["A_d"] + c["A_a"])
    else:
        NP = {"table4": 4, "table6": 6}[route]
        h = 1.0 / HINV
        rnd = (3 * NP + 1) * U * LEBESGUE[NP]
        tab_d = INTERP_C[NP] * h ** NP * c["D%d_d" % NP] + rnd * c["M_d"]
        sum_d = 388 * U * c["A_d"]
        eps = 1e-6 * D_TABLE
        arith_d = torch.where(xd < D_TABLE - eps, tab_d, torch.where(xd > D_TABLE + eps, sum_d, torch.maximum(tab_d, sum_d)))
        total = total + arith_d + INTERP_C[NP] * h ** NP * c["D%d_a" % NP] + rnd * c["M_a"]
    if out_bf16:
        total = total + bf16_half_ulp(ref.abs() + total)
    return total


def bf16_half_ulp(v):
    """Half the spacing of bf16 (8 significant bits) at |v|: 2^(floor(log2 |v|) - 8)"""
    return torch.ldexp(torch.ones_like(v), torch.frexp(v)[1] - 9)


# ------------------------------------------------------------------------------------------------------------ float32 emulation, mutants
def _bf(x):
    return x.float().bfloat16().to(F64)


def _split(x):
    x = x.float()
    hi = x.bfloat16().float()
    return hi.to(F64), (x - hi).bfloat16().to(F64)


def emulate(points, module, knn, route, out_bf16=False, mutant=None):
    """The float32 restatement of a route on the CPU: fp32 indices (phase A's formulas), then `split`: sinusoids and weights as bf16
    hi + lo, hh + hl + lh; `bf16`: the hi parts alone; `table4` / `table6`: fp32 tables and the interpolation rule, the defining sum past
    the table.  The result is rounded to fp32 (bf16) like the kernel's.  `mutant`: one of MUTANTS applied."""
    sigma_d, factor_a, div = _params(module)
    reduction = module.reduction_a
    if mutant == "mean_for_max":
        reduction = "mean" if reduction == "max" else "max"
    p = points.float().cpu()
    B, n, _ = p.shape
    Wd, Wa = module.proj_d.weight.detach().cpu(), module.proj_a.weight.detach().cpu()
    bias = (module.proj_d.bias.detach().cpu().float() + module.proj_a.bias.detach().cpu().float()).to(F64)
    if route in ("table4", "table6"):
        NP = {"table4": 4, "table6": 6}[route]
        used = 4 if mutant == "four_for_six" and NP == 6 else NP
        td, ta = (t.float().to(F64).numpy() for t in tables64(module, NP))

        def proj(x, tab, W, is_d):
            xf = x.reshape(-1).to(F64).numpy()
            inside = xf <= D_TABLE if is_d else np.ones_like(xf, dtype=bool)
            out = np.zeros((len(xf), 256))
            shift = np.zeros(len(xf), dtype=int)
            if is_d and mutant == "lds_row_for_global":
                shift = ((xf >= D_LDS) & (xf < D_TABLE - 0.5)).astype(int)
            for s in (0, 1):
                sel = inside & (shift == s)
                if sel.any():
                    out[sel] = table_interp(tab, xf[sel], used, table_npoint=NP, row_shift=s)
            if (~inside).any():
                out[~inside] = (_sinus(torch.from_numpy(xf[~inside]), div) @ W.to(F64).t()).numpy()
            return torch.from_numpy(out).float().to(F64).reshape(*x.shape, 256)
    else:
        def proj(x, tab, W, is_d):
            s = _sinus(x.to(F64), div).float()
            if route == "bf16" or mutant == "hi_only":
                return (_bf(s) @ _bf(W).t()).float().to(F64)
            (sh, sl), (wh, wl) = _split(s), _split(W)
            return (sh @ wh.t() + sl @ wh.t() + sh @ wl.t()).float().to(F64)
        td = ta = None
    out = torch.empty(B, n, n, 256, dtype=F64)
    for b in range(B):
        xd, xa = _indices(p[b], knn[b].cpu(), 0, n, np.float32(sigma_d).item(), np.float32(factor_a).item())
        if mutant == "diag_pi":
            xa[torch.arange(n), torch.arange(n)] = float(np.float32(math.pi) * np.float32(factor_a))
        a = proj(xa, ta, Wa, False)
        out[b] = proj(xd, td, Wd, True) + (a.amax(2) if reduction == "max" else a.mean(2)) + bias
    out = out.float()
    if mutant == "shift_j" and n > 64:   # the columns of the second 64-column step come from one column to the left
        out[:, :, 64:] = out[:, :, 63:-1].clone()
    if mutant == "drop_tail" and (n * n) % 32:
        out.view(B, n * n, 256)[:, n * n - (n * n) % 32:] = float("nan")
    return out.bfloat16() if out_bf16 else out


def within(got, ref, bnd):
    """The GPU test's check: every element written (no NaN left) and |got - ref| <= bound."""
    return bool(((got.to(F64) - ref).abs() <= bnd).all())


# ------------------------------------------------------------------------------------------------------------ the GPU test's cases
SIZES = ((3, 4), (1, 5), (2, 33), (3, 63), (2, 64), (3, 65), (2, 130))   # B n n is no multiple of 32 wherever n allows it
FULL = (3, 197)                                                          # the full coarse size: always the `bg` cloud
KINDS = ("random", "lattice", "dup_heavy", "line", "rings", "wide")
ROUTES = (("split", False), ("split", True), ("bf16", True), ("table4", False), ("table4", True), ("table6", False), ("table6", True),
          ("train", False))


def _cases():
    """(route, out_bf16, reduction, regime, kind, B, n): every route sees every cloud kind and every size."""
    out = []
    for r, (route, ob) in enumerate(ROUTES):
        for s, (B, n) in enumerate(SIZES):
            # (the first six sizes rotate through the six kinds; the seventh takes the rings again, with all their radii)
            kind = KINDS[(s + r) % len(KINDS)] if s < len(KINDS) else "rings"
            out.append((route, ob, "mean" if (s + r) % 3 == 0 else "max", "trained" if (s + r) % 2 else "default", kind, B, n))
    for route, ob in ROUTES:
        out.append((route, ob, "max", "trained", "bg", *FULL))
    return out


CASES = _cases()
BACKWARD_CASES = tuple((kind, red, B, n) for kind in ("wide", "rings_bwd") for red in ("max", "mean") for B, n in ((2, 65), (3, 33)))
KNN_CASES = tuple((kind, B, n) for kind in ("random", "bg", "object", "lattice", "dup_heavy", "line", "rings", "wide")
                  for B, n in ((3, 4), (1, 5), (3, 65), (3, 197)))
EXACT_KINDS = ("random", "bg", "object", "lattice", "dup_heavy")   # the kernel's list must EQUAL knn_exact
