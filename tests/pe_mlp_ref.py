"""Float64 reference, with a propagated error bound, of the MLP stage of the positional encoding (csrc/pe.hip
pe_group_mlp_max_bf16x3_kernel and pe_group_mlp_max_kernel): neighbour lists and frames in, max-pooled 128 channels out.

    d = p_k - c,   f = [d, F d / radius]   (F: the 3 x 3 frame, rows x, y, z; radius as the float32 value)
    x <- relu(W x + b) three times (6 -> 32 -> 64 -> 128),   out = max over ALL S list entries

Everything is torch float64 computed from the fp32 inputs, on whatever device the inputs are on (the large cases of
test_pe_mlp_gpu.py run it on the GPU), in chunks of centres.  The reference knows nothing about counts: a kernel that skips the tiles
of padding must give what the full list gives.

The bound is carried next to the values and every number in it is derived:

    e0 = 2^-24 |d|  (channels 0-2: one fp32 subtraction),   5 * 2^-24 (|F| |d|) / radius  (channels 3-5: the subtraction, the
         division, three products and two additions)
    per layer  e <- |W| e + u (|W| |x| + |b|);  ReLU and max are 1-Lipschitz, so bound = max over neighbours of e3

bf16x3 (U_BF16X3 = 3 * 2^-17, the budget of test_linear_f32x3_vs_fp64_reference): each operand's hi + lo is exact to 2^-18 of it,
the dropped lo * lo term is at most 2^-18 of the product, 3 K fp32 accumulations add at most 3 * 64 * 2^-24 -- a worst case for
K <= 64.  Exact fp32 (U_FP32): (K + 2) * 2^-24 per layer, K = 6, 32, 64.

Nothing here is used by the package.  The generator of the test problems (`make_case`) and the mutants the tests must be able to
tell from the truth (`hi_only`, `drop_last_tile`, `swap_in`, `swap_out`) are here too, so that test_pe_mlp_ref_cpu.py can check the
teeth of test_pe_mlp_gpu.py without a GPU."""
import math
from types import SimpleNamespace

import torch

F64 = torch.float64
U_BF16X3 = 3 * 2.0 ** -17
U_FP32 = tuple((k + 2) * 2.0 ** -24 for k in (6, 32, 64))
ROTATION = (1, 2, 31, 32, 33, 63, 64, 65, "S-1", "S", -1, 0)  # counts, by centre
DEAD_EVERY = 7      # every 7th output channel of layer 3 is dead
ROWS_PER_CHUNK = 1 << 18


# ------------------------------------------------------------------------------------------------------------ chain
def _chunks(B, N, S):
    step = max(1, ROWS_PER_CHUNK // S)
    return [(a, min(a + step, B * N)) for a in range(0, B * N, step)]


def features(pts, radius, lists, frames, a, b):
    """Features (n,S,6) and their rounding e0 of the centres a..b of the flattened (B * N) centre axis."""
    B, N, _ = pts.shape
    S = lists.shape[2]
    p = pts.to(F64).reshape(B * N, 3)
    idx = (lists.reshape(B * N, S)[a:b].to(torch.int64) & 0xFFFF)                 # 16-bit ids held in int16
    cloud = torch.arange(a, b, device=pts.device).div(N, rounding_mode="floor") * N
    d = p[idx + cloud[:, None]] - p[a:b, None]                                    # (n,S,3)
    Fm = frames.to(F64).reshape(B * N, 3, 3)[a:b]
    r = float(torch.tensor(radius, dtype=torch.float32))
    f = torch.cat([d, torch.einsum("nij,nsj->nsi", Fm, d) / r], 2)
    e0 = torch.cat([2.0 ** -24 * d.abs(), 5 * 2.0 ** -24 * torch.einsum("nij,nsj->nsi", Fm.abs(), d.abs()) / r], 2)
    return f, e0


def _split(x):
    """bf16 hi + lo of the fp32 value of x, as float64."""
    x = x.float()
    hi = x.bfloat16().float()
    lo = (x - hi).bfloat16()
    return hi.to(F64), lo.to(F64)


def _slot_limit(counts, S, a, b):
    """drop_last_tile: the slots [0, 32 * floor((cnt - 1) / 32)) stay (-1 = a full list)."""
    cnt = counts.reshape(-1)[a:b].to(torch.int64)
    cnt = torch.where(cnt < 0, torch.full_like(cnt, S), cnt).clamp(1, S)
    return (cnt - 1).div(32, rounding_mode="floor") * 32


def _run(pts, radius, lists, frames, folded, u=None, emulate=False, drop_counts=None):
    B, N, _ = pts.shape
    S = lists.shape[2]
    dev = pts.device
    Wb = [(w.to(dev, F64), b.to(dev, F64)) for w, b in folded]
    us = (u,) * 3 if not isinstance(u, (tuple, list)) else tuple(u)
    out = torch.empty(B * N, 128, dtype=F64, device=dev)
    bound = torch.empty(B * N, 128, dtype=F64, device=dev) if u is not None else None
    for a, b in _chunks(B, N, S):
        x, e = features(pts, radius, lists, frames, a, b)
        if emulate:
            x = x.float().to(F64)  # the kernel holds fp32 features
        for (w, bias), ul in zip(Wb, us):
            if u is not None:
                e = e @ w.abs().t() + ul * (x.abs() @ w.abs().t() + bias.abs())
            if emulate:
                (wh, wl), (xh, xl) = _split(w), _split(x)
                x = torch.relu(xh @ wh.t() + xl @ wh.t() + xh @ wl.t() + bias).float().to(F64)  # hh + hl + lh exactly, one fp32 rounding
            else:
                x = torch.relu(x @ w.t() + bias)
        if drop_counts is not None:
            keep = torch.arange(S, device=dev)[None, :] < _slot_limit(drop_counts, S, a, b)[:, None]
            x = x * keep[:, :, None]  # (post-ReLU values are >= 0: a dropped slot cannot win)
        out[a:b] = x.amax(1)
        if u is not None:
            bound[a:b] = e.amax(1)
    out = out.reshape(B, N, 128)
    return out if u is None else (out, bound.reshape(B, N, 128))


def pe_mlp_ref(pts, radius, lists, frames, folded, u=U_BF16X3):
    """(out, bound), both (B,N,128) float64.  `folded` = [(W, b)] * 3 (fp32, BatchNorm folded); `u` a number or one per layer."""
    return _run(pts, radius, lists, frames, folded, u=u)


def pe_mlp_values(pts, radius, lists, frames, folded):
    """The values of pe_mlp_ref alone (for mutants)."""
    return _run(pts, radius, lists, frames, folded)


def bf16x3_emulated(pts, radius, lists, frames, folded):
    """The same chain with both operands of every product split into bf16 hi + lo and hh + hl + lh summed exactly."""
    return _run(pts, radius, lists, frames, folded, emulate=True)


# ------------------------------------------------------------------------------------------------------------ mutants
def hi_only(folded, layer):
    """The weights of one layer rounded to bf16: that layer's lo terms dropped."""
    return [(w.float().bfloat16().float() if i == layer else w, b) for i, (w, b) in enumerate(folded)]


def drop_last_tile(pts, radius, lists, counts, frames, folded):
    """The max taken over slots [0, 32 * floor((cnt - 1) / 32)): a tile loop that stops one tile early."""
    return _run(pts, radius, lists, frames, folded, drop_counts=counts)


def dropped_centres(counts, S):
    """(B,N) bool: centres with cnt > 32 (-1 = S), whose last tile drop_last_tile drops."""
    cnt = torch.where(counts < 0, torch.full_like(counts, S), counts)
    return cnt > 32


def swap_in(folded, layer, i, j):
    """Input channels i and j of a layer swapped (the move pe_kperm makes)."""
    out = [(w.clone(), b) for w, b in folded]
    out[layer][0][:, [i, j]] = out[layer][0][:, [j, i]]
    return out


def swap_out(folded, layer, i, j):
    """Output rows i and j of a layer swapped, weights and bias (the move cd_row makes)."""
    out = [(w.clone(), b.clone()) for w, b in folded]
    for t in out[layer]:
        t[[i, j]] = t[[j, i]]
    return out


# ------------------------------------------------------------------------------------------------------------ modules
def fold64(mlp):
    """The BatchNorm fold of a _SharedMLP in float64, from its raw parameters: W' = W * s, b' = beta - mean * s, s = gamma / sqrt(var + eps)."""
    out = []
    for l in mlp.layers():
        bn = l.normlayer.bn
        s = bn.weight.detach().to(F64) / torch.sqrt(bn.running_var.to(F64) + bn.eps)
        w = l.conv.weight.detach().to(F64)
        out.append((w.reshape(w.shape[0], -1) * s[:, None], bn.bias.detach().to(F64) - bn.running_mean.to(F64) * s))
    return out


class _Folded(torch.nn.Module):
    def __init__(self, w, b):
        super().__init__()
        self.conv = torch.nn.Conv2d(w.shape[1], w.shape[0], 1, bias=False)
        self.conv.weight.data.copy_(w.reshape(*w.shape, 1, 1))
        self.register_buffer("b", b.clone())

    def folded(self):
        return self.conv.weight.reshape(self.conv.weight.shape[0], -1), self.b


class FoldedMLP(torch.nn.Module):
    """Stand-in for a _SharedMLP that hands the kernels' wrappers exactly the weights of a case: `.layers()[i].folded()`."""

    def __init__(self, folded):
        super().__init__()
        self.seq = torch.nn.ModuleList(_Folded(w, b) for w, b in folded)

    def layers(self):
        return list(self.seq)


def randomise_bn_(mlp, seed):
    """Non-trivial BatchNorm statistics for a _SharedMLP: running mean and var away from 0 and 1, affine weight negative on every
    third channel."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for l in mlp.layers():
            bn = l.normlayer.bn
            c = bn.weight.shape[0]
            r = lambda: torch.rand(c, generator=g).to(bn.weight)  # noqa: E731
            bn.running_mean.copy_(r() - 0.5)
            bn.running_var.copy_(0.25 + 2.0 * r())
            bn.weight.copy_((0.5 + r()) * torch.where(torch.arange(c) % 3 == 0, -1.0, 1.0).to(bn.weight))
            bn.bias.copy_(r() - 0.5)
    return mlp


# ------------------------------------------------------------------------------------------------------------ cases
def make_weights(seed):
    """[(W, b)] * 3 fp32: W = randn / sqrt(K) times logspace(-0.5, 0.5) per output channel (a decade of dynamic range), biases of
    both signs."""
    g = torch.Generator().manual_seed(seed)
    folded = []
    for k, c in ((6, 32), (32, 64), (64, 128)):
        scale = torch.logspace(-0.5, 0.5, c)[torch.randperm(c, generator=g)]
        folded.append(((torch.randn(c, k, generator=g) / math.sqrt(k)) * scale[:, None], 0.3 * torch.randn(c, generator=g)))
    return folded


def counts_rotation(S):
    rot = [S - 1 if v == "S-1" else S if v == "S" else v for v in ROTATION]
    return [v for v in rot if v <= S]


def make_case(B, N, S, seed, radius=0.25, device="cpu"):
    """Inputs of the MLP stage built to reach what a tile loop can get wrong (tensors on `device`; the random draws are the CPU
    generator's, so a case is the same everywhere):

    points uniform in [-0.6, 0.6]^3; frames a random rotation or reflection plus 0.1 * randn, so not orthonormal (to the
    kernel a frame is only a linear map) yet far from singular: the point farthest from the centre stays far in the local coordinates; lists (B,N,S) int16 of ids
    (a + k * step) mod N with a per-centre random start and a random step coprime to N -- distinct while k < N --, padded from
    slot cnt on with copies of entry 0 as the ball query pads; counts rotating over the centres through ROTATION (values above S
    left out; -1: S distinct ids; 0: S copies of point 0); for cnt > 1 slot cnt - 1, and no other, holds the point of the cloud farthest
    from the centre, which puts the maxima of many channels into the last valid slot; weights of `make_weights`; every 7th output
    channel of layer 3 with a bias below -max |W| x2, so that its reference output is exactly 0 for every centre (asserted)."""
    g = torch.Generator().manual_seed(seed)
    pts = (torch.rand(B, N, 3, generator=g) * 1.2 - 0.6).to(device)
    q = torch.linalg.qr(torch.randn(B, N, 3, 3, generator=g))[0]
    frames = (q + 0.1 * torch.randn(B, N, 3, 3, generator=g)).reshape(B, N, 9).to(device)
    coprime = torch.tensor([s for s in range(1, max(N, 2)) if math.gcd(s, N) == 1])
    start = torch.randint(0, N, (B, N), generator=g).to(device)
    step = coprime[torch.randint(0, len(coprime), (B, N), generator=g)].to(device)
    rot = torch.tensor(counts_rotation(S), dtype=torch.int32)
    counts = rot[torch.arange(B * N) % len(rot)].reshape(B, N).to(device)
    k = torch.arange(S, device=device)
    ids = (start[:, :, None] + k * step[:, :, None]) % N                                      # (B,N,S) int64
    far = torch.stack([torch.cdist(c, c).argmax(1) for c in pts.double()])                    # (B,N)
    cnt = counts.long()
    last = (cnt - 1).clamp_min(0)[:, :, None]
    has_far = (cnt > 1)[:, :, None]
    ids = torch.where((ids == far[:, :, None]) & (k < last) & has_far, ids.gather(2, last), ids)  # (a swap: the far point sits in slot cnt - 1 only)
    ids = torch.where((k == last) & has_far, far[:, :, None], ids)
    ids = torch.where((k >= cnt[:, :, None]) & (cnt >= 0)[:, :, None], ids[:, :, :1], ids)   # padding = entry 0
    ids = torch.where((cnt == 0)[:, :, None], torch.zeros_like(ids), ids)
    assert int(ids.min()) >= 0 and int(ids.max()) < N
    lists = ids.to(torch.int16)
    folded = [(w.to(device), b.to(device)) for w, b in make_weights(seed + 1000)]
    # dead channels: the largest value any input of layer 3 takes bounds its pre-activations
    x2max = torch.zeros(64, dtype=F64, device=device)
    for a, b in _chunks(B, N, S):
        x, _ = features(pts, radius, lists, frames, a, b)
        for w, bias in folded[:2]:
            x = torch.relu(x @ w.to(F64).t() + bias.to(F64))
        x2max = torch.maximum(x2max, x.amax((0, 1)))
    dead = torch.arange(0, 128, DEAD_EVERY, device=device)
    w3, b3 = folded[2]
    reach = w3[dead].abs().to(F64) @ x2max
    b3[dead] = -(1.25 * reach + 1.0).float()
    assert bool((reach + b3[dead].to(F64) < 0).all())  # relu(W x + b) <= relu(|W| x2max + b) = 0, exactly
    return SimpleNamespace(pts=pts, radius=radius, lists=lists, counts=counts, frames=frames, folded=folded, dead=dead, S=S)
