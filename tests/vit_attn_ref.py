"""Float64 reference, elementwise bounds and probe inputs of the ViT attention cores (csrc/vit_attn.hip: vit_attn_kernel<1,1,4>,
<2,2,4>, <2,2,8> and vit_attn_kernel_dma<4>; csrc/attn_f32.hip: vit_attn_f32_kernel; csrc/vit_attn_f32s.hip):

    out[b, t, h*64 + d] = sum_k p_k v[b, k, h, d],   p = softmax_k(q[b, t, h] . k[b, k, h] / 8)

`vit_attn_ref(qkv, H)` takes that in torch float64 on the inputs as given, on whatever device they are on, and returns it with
A[b, t, h*64 + d] = sum_k p_k |v_k,d|, the softmax-weighted magnitude.  Every bound is a multiple of A, elementwise.

bf16 kernels -- BF16_BOUND * A with BF16_BOUND = 1.05 * 2^-7.
    P is rounded to bf16 with relative error <= 2^-8 AT ANY MAGNITUDE (which is why the deferred reference point, under which P may
    reach 2^8 instead of 1, costs nothing), so sum_k P_k v_k,d is off by at most 2^-8 sum_k P_k |v_k,d|; l is summed from the unrounded
    fp32 P; the products of bf16 inputs are exact in fp32; the output is rounded to bf16: another 2^-8 of |out| <= A.  2^-7 A in all;
    the 5 % is for the fp32 accumulations and v_exp_f32.  `emulate_bf16` does that arithmetic in float64 (P rounded to bf16 after a
    random reference shift in [0, 8] in the exp2 domain, bf16 output); test_vit_attn_ref_cpu.py keeps it inside the bound.

fp32-class kernels (operands as bf16 hi + lo, three MFMAs per product) -- two bounds, both must hold.
    hard:   (expm1(2 eps_q) + 2^-14) * A,   eps_q = U_BF16X3 * max_k sum_d |q_d k_d| / 8,   U_BF16X3 = 3 * 2^-17
            (the split-product budget of test_linear_f32x3_vs_fp64_reference).  A logit error <= eps changes every p by at most
            e^(+-2 eps) (numerator and normaliser); 2^-14 covers the P.V split products, the split output and the fp32 accumulation.
    sharp:  C32 * A.  The hard bound is ~30x looser than the arithmetic, so a dropped lo term hides under it.  C32 is NOT derived
            from any kernel's output: it is 8 x the worst err / A of `emulate_f32x3` -- a float64 model of the declared arithmetic
            (hi = bf16(x), lo = bf16(x - hi); hi.hi + hi.lo + lo.hi in both contractions, P split the same way, output split) --
            over the cases of test_vit_attn_ref_cpu.py (every family, T in 40 / 293 / 1057, B = 2, H = 2).  The 8 is for fp32 instead
            of float64 accumulation over <= 1535 keys and for exp2.
            Measured 2026-10-20: the emulation's worst err / A = 3.082e-5 (family `match`, T = 293)  ->  C32 = 2.47e-4.
            The mutants that drop K's lo plane in q.k or V's lo plane move `sharp` by 3.1e-3 A and more, 12x above C32.

Probe inputs: functions of (B, T, H, seed) that return an fp32 (B, T, 3 H 64) qkv; with bf16=True the values are bf16-representable
(what the bf16 kernels get), otherwise un-rounded fp32 (what the fp32-class kernels get).  FAMILIES names them:
    sharp     randn, q scaled by 2.
    match     per (image, head) keys mag u_k with random unit u_k, query t = mag u_pi(t) for a random permutation pi: every key slot,
              T - 1 included, is THE key of exactly one query, so a dropped, misplaced or mis-headed K / V row is an O(A) error.
              mag = 40 (bf16) / 12 (fp32 class; the hard bound is then ~1e-3 A).
    lastkey   every query of every head aligned with key T - 1: a lane whose partial-tile mask lets a clamped duplicate of the last
              key through roughly halves its output.
    stair+9, stair+5, stair-9
              channel 0 makes the score, in the exp2 domain, rise or fall by `step` per 32 keys (q_0 and k_0 are bf16-exact, so the
              staircase is the same for every kernel); the other 63 channels are random at reduced scale (their part of a score
              has sigma 0.18, so a step of 9 stays above the kernels' threshold of 8 and one of 5 below it).  +9: the reference point moves
              and the fix-up runs in every tile, the partial one and the first of every chunk included; +5: every second tile, P up
              to 2^8 in between; -9: never after the first tile, and P underflows further along.
    bait      B = 2.  The first rows of image 1's keys are what image 0's queries are aligned with, at twice the magnitude of anything
              image 0 holds; the same for image 1's queries and the last rows of image 0's keys.  `bait(...)[b:b + 1]` is the
              single-image form.  A kernel that reads across an image border gets a different answer.

Nothing here is used by the package.  The mutants the GPU probes must be able to tell from the truth (`drop_key_ratios`,
`dup_last_key`, `swap_v_rows`, `swap_v_heads`, `leak_next_image`, `no_rescale`, and the two flags of `emulate_f32x3`) are here too, so
that test_vit_attn_ref_cpu.py can check the teeth of test_vit_attention_probes_gpu.py without a GPU."""
import math

import torch

F64 = torch.float64
LOG2E = 1.4426950408889634
BF16_BOUND = 1.05 * 2.0 ** -7
U_BF16X3 = 3 * 2.0 ** -17
C32 = 2.47e-4   # 8 x 3.082e-5, measured 2026-10-20 (module docstring)
MAG_BF16, MAG_F32, MAG_BAIT = 40.0, 12.0, 8.0
STAIR_STEPS = (9, 5, -9)


# ------------------------------------------------------------------------------------------------------------ layout
def heads_of(qkv, H, heads=None):
    """(B,T,3 H 64) -> q, k, v as float64 (B,h,T,64); `heads` picks a subset (before the conversion: the input may be huge)."""
    B, T, C3 = qkv.shape
    assert C3 == 3 * H * 64
    x = qkv.reshape(B, T, 3, H, 64)
    if heads is not None:
        x = x[:, :, :, torch.as_tensor(list(heads), device=qkv.device)]
    x = x.to(F64).permute(2, 0, 3, 1, 4)
    return x[0], x[1], x[2]


def merge(o):
    """(B,h,T,64) -> (B,T,h*64)"""
    B, h, T, _ = o.shape
    return o.transpose(1, 2).reshape(B, T, h * 64)


def unmerge(o):
    """(B,T,h*64) -> (B,h,T,64)"""
    B, T, C = o.shape
    return o.reshape(B, T, C // 64, 64).transpose(1, 2)


def split_planes(x):
    """bf16 hi and lo of the fp32 value of x (round to nearest even, as v_cvt_pk_bf16_f32), both as float64."""
    x = x.float()
    hi = x.bfloat16().float()
    lo = (x - hi).bfloat16()
    return hi.to(F64), lo.to(F64)


def to_split_layout(x2):
    """(M,K) fp32 -> the split layout of csrc/gemm_f32.hip as an (M,2K) bf16 tensor: per row and 32-channel block [hi (32) | lo (32)]."""
    M, K = x2.shape
    hi = x2.float().bfloat16()
    lo = (x2.float() - hi.float()).bfloat16()
    return torch.stack([hi.reshape(M, K // 32, 32), lo.reshape(M, K // 32, 32)], 2).reshape(M, 2 * K)


def from_split_layout(s):
    """(M,2K) bf16 in the split layout -> hi + lo as float64 (M,K)."""
    M, K2 = s.shape
    blk = s.reshape(M, K2 // 64, 2, 32).to(F64)
    return (blk[:, :, 0] + blk[:, :, 1]).reshape(M, K2 // 2)


# --------------------------------------------------------------------------------------------------------- reference
def attend(q, k, v):
    """softmax(q k^T / 8) v and softmax(q k^T / 8) |v| of float64 heads (..., T, 64), keys (..., Tk, 64)."""
    p = torch.softmax(q @ k.transpose(-1, -2) / 8.0, -1)
    return p @ v, p @ v.abs()


def vit_attn_ref(qkv, H, heads=None):
    """(ref, A), each float64 (B,T,h*64); one image at a time (12 x 1535^2 doubles = 226 MB)."""
    q, k, v = heads_of(qkv, H, heads)
    outs = [attend(q[b], k[b], v[b]) for b in range(q.shape[0])]
    return merge(torch.stack([o for o, _ in outs])), merge(torch.stack([a for _, a in outs]))


def eps_q(qkv, H, heads=None):
    """U_BF16X3 * max_k sum_d |q_d k_d| / 8 per query, broadcast over the head's 64 channels: (B,T,h*64)."""
    q, k, _ = heads_of(qkv, H, heads)
    e = torch.stack([(q[b].abs() @ k[b].abs().transpose(-1, -2)).max(-1)[0] for b in range(q.shape[0])]) * (U_BF16X3 / 8.0)
    return merge(e[..., None].expand(*e.shape, 64))


def bf16_bound(A):
    return BF16_BOUND * A


def f32_hard_bound(qkv, H, A, heads=None):
    return (torch.expm1(2.0 * eps_q(qkv, H, heads)) + 2.0 ** -14) * A


def f32_bound(qkv, H, A, heads=None):
    """Both fp32-class bounds at once: the elementwise smaller of the hard one and C32 * A."""
    return torch.minimum(f32_hard_bound(qkv, H, A, heads), C32 * A)


def worst(out, ref, bound):
    """(worst err / bound, its index tuple); 0 / 0 counts as 0, anything / 0 as inf."""
    err = (out.to(F64) - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0).to(F64))
    ratio = torch.nan_to_num(ratio, nan=math.inf)
    i = int(ratio.argmax())
    idx = []
    for n in reversed(ratio.shape):
        idx.append(i % n)
        i //= n
    return float(ratio.max()), tuple(reversed(idx))


def describe(out, ref, bound):
    """'worst err / bound r at (b, t, h, d)' for an assertion message."""
    r, (b, t, c) = worst(out, ref, bound)
    return "worst err / bound = %.3g at (b, t, h, d) = (%d, %d, %d, %d)" % (r, b, t, c // 64, c % 64)


# --------------------------------------------------------------------------------------------------------- emulations
def emulate_bf16(qkv, H, seed=0):
    """The bf16 kernels' declared arithmetic in float64: P = exp2(s - m + shift) with a random reference shift in [0, 8] per query,
    l from the unrounded P, P rounded to bf16 for P.V, the output rounded to bf16."""
    q, k, v = heads_of(qkv, H)
    s2 = (q @ k.transpose(-1, -2)) * (LOG2E / 8.0)
    shift = 8.0 * torch.rand(s2.shape[:-1], generator=torch.Generator().manual_seed(seed), dtype=F64).to(s2.device)
    P = torch.exp2(s2 - s2.max(-1, keepdim=True)[0] + shift[..., None])
    Pb = P.float().bfloat16().to(F64)
    return merge((Pb @ v) / P.sum(-1, keepdim=True)).float().bfloat16().to(F64)


def emulate_f32x3(qkv, H, drop_qk_lo=False, drop_v_lo=False, split_out=True):
    """The fp32-class kernels' declared arithmetic with float64 accumulation: every operand as bf16 hi + lo, products hi.hi + hi.lo +
    lo.hi in q.k and in P.V (P split the same way), the output as hi + lo.  drop_qk_lo: the K lo . Q hi product is left out;
    drop_v_lo: the P hi . V lo product is left out -- the two mutants the sharp bound C32 must catch."""
    q, k, v = heads_of(qkv, H)
    (qh, ql), (kh, kl), (vh, vl) = split_planes(q), split_planes(k), split_planes(v)
    s = qh @ kh.transpose(-1, -2) + ql @ kh.transpose(-1, -2)
    if not drop_qk_lo:
        s = s + qh @ kl.transpose(-1, -2)
    s2 = s * (LOG2E / 8.0)
    P = torch.exp2(s2 - s2.max(-1, keepdim=True)[0])
    ph, pl = split_planes(P)
    o = ph @ vh + pl @ vh
    if not drop_v_lo:
        o = o + ph @ vl
    o = o / P.sum(-1, keepdim=True)
    if split_out:
        oh, ol = split_planes(o)
        o = oh + ol
    return merge(o)


# ------------------------------------------------------------------------------------------------------------ mutants
def from_heads(q, k, v):
    """attend() per image on (B,h,T,64) heads whose key count may differ from T; merged (B,T,h*64)."""
    return merge(torch.stack([attend(q[b], k[b], v[b])[0] for b in range(q.shape[0])]))


def dup_last_key(qkv, H):
    """One unmasked slot past the sequence: a clamped duplicate of key T - 1 takes part in the softmax, with V = 0."""
    q, k, v = heads_of(qkv, H)
    return from_heads(q, torch.cat([k, k[:, :, -1:]], 2), torch.cat([v, torch.zeros_like(v[:, :, -1:])], 2))


def swap_v_rows(qkv, H, i):
    """V rows i and i + 1 change places (K stays)."""
    q, k, v = heads_of(qkv, H)
    v = v.clone()
    v[:, :, [i, i + 1]] = v[:, :, [i + 1, i]]
    return from_heads(q, k, v)


def swap_v_heads(qkv, H, h):
    """Heads h and h + 1 change places in V."""
    q, k, v = heads_of(qkv, H)
    v = v.clone()
    v[:, [h, h + 1]] = v[:, [h + 1, h]]
    return from_heads(q, k, v)


def leak_next_image(qkv, H, n=32):
    """Image b reads the first n key / value rows of image b + 1 as its keys T .. T + n - 1 (the last image reads nothing extra)."""
    q, k, v = heads_of(qkv, H)
    outs = []
    for b in range(q.shape[0]):
        kk, vv = (k[b], v[b]) if b + 1 == q.shape[0] else (torch.cat([k[b], k[b + 1][:, :n]], 1), torch.cat([v[b], v[b + 1][:, :n]], 1))
        outs.append(attend(q[b], kk, vv)[0])
    return merge(torch.stack(outs))


def no_rescale(qkv, H):
    """The fix-up mutant: on a move of the reference point the old accumulator is not scaled, i.e. every 32-key tile enters O with
    the weights it had under the running reference of its own time (weight 1 instead of alpha on all earlier tiles); l is right."""
    q, k, v = heads_of(qkv, H)
    s2 = (q @ k.transpose(-1, -2)) * (LOG2E / 8.0)
    T = s2.shape[-1]
    m_fin = s2.max(-1, keepdim=True)[0]
    l = torch.exp2(s2 - m_fin).sum(-1, keepdim=True)
    o = torch.zeros_like(q)
    m_run = torch.full_like(m_fin, -math.inf)
    for k0 in range(0, T, 32):
        st = s2[..., k0:k0 + 32]
        m_run = torch.maximum(m_run, st.max(-1, keepdim=True)[0])
        o = o + torch.exp2(st - m_run) @ v[..., k0:k0 + 32, :]
    return merge(o / l)


def drop_key_ratios(qkv, H, ref, bound):
    """For every key slot k: the largest |mutant_k - ref| / bound over all outputs, where mutant_k attends to every key but k (in every
    image and head at once).  (T,) float64.  Needs T >= 2."""
    q, k, v = heads_of(qkv, H)
    B, h, T, _ = q.shape
    assert T >= 2
    refh, bndh = unmerge(ref), unmerge(bound)
    best = torch.zeros(T, dtype=F64, device=qkv.device)
    for b in range(B):
        for j in range(h):
            s = q[b, j] @ k[b, j].T / 8.0
            pun = torch.exp(s - s.max(-1, keepdim=True)[0])
            l = pun.sum(-1, keepdim=True)
            N = pun @ v[b, j]
            p = pun / l
            stable = p <= 0.5   # N - P_k v_k and l - P_k lose nothing there; the other (t, k) are recomputed below
            for k0 in range(0, T, 64):
                pk = pun[:, k0:k0 + 64]
                o = (N[:, None, :] - pk[:, :, None] * v[b, j, k0:k0 + 64][None]) / (l - pk)[:, :, None]
                r = (o - refh[b, j][:, None, :]).abs() / bndh[b, j][:, None, :]
                r = torch.where(stable[:, k0:k0 + 64, None], r, torch.zeros_like(r))
                best[k0:k0 + 64] = torch.maximum(best[k0:k0 + 64], r.amax((0, 2)))
            ti, ki = torch.nonzero(~stable, as_tuple=True)
            if len(ti):
                rows = s[ti].clone()
                rows[torch.arange(len(ti)), ki] = -math.inf
                o = torch.softmax(rows, -1) @ v[b, j]
                r = ((o - refh[b, j][ti]).abs() / bndh[b, j][ti]).amax(1)
                best.scatter_reduce_(0, ki, r, "amax")
    return best


# ------------------------------------------------------------------------------------------------------------ families
def _finish(x, bf16):
    B, T = x.shape[:2]
    x = x.reshape(B, T, -1).float().contiguous()
    return x.bfloat16().float() if bf16 else x


def _units(g, *shape):
    u = torch.randn(*shape, 64, generator=g, dtype=F64)
    return u / u.norm(dim=-1, keepdim=True)


def sharp(B, T, H, seed, bf16=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, 3, H, 64, generator=g)
    x[:, :, 0] *= 2.0  # sharper softmax than unit-variance scores
    return _finish(x, bf16)


def match(B, T, H, seed, bf16=False, mag=None):
    mag = mag or (MAG_BF16 if bf16 else MAG_F32)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, 3, H, 64, generator=g)
    u = _units(g, B, H, T)                                                  # (B,H,T,64)
    pi = torch.stack([torch.randperm(T, generator=g) for _ in range(B * H)]).reshape(B, H, T)
    x[:, :, 1] = (mag * u).transpose(1, 2).float()
    x[:, :, 0] = (mag * torch.gather(u, 2, pi[..., None].expand(B, H, T, 64))).transpose(1, 2).float()
    return _finish(x, bf16)


def match_owner(B, T, H, seed):
    """pi of `match` with the same arguments: query t of (b, h) owns key pi[b, h, t]."""
    g = torch.Generator().manual_seed(seed)
    torch.randn(B, T, 3, H, 64, generator=g)
    _units(g, B, H, T)
    return torch.stack([torch.randperm(T, generator=g) for _ in range(B * H)]).reshape(B, H, T)


def lastkey(B, T, H, seed, bf16=False, mag=None):
    mag = mag or (MAG_BF16 if bf16 else MAG_F32)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, 3, H, 64, generator=g)
    u = (mag * _units(g, B, H)).float()                                     # (B,H,64)
    x[:, :, 0] += u[:, None]
    x[:, T - 1, 1] = u
    return _finish(x, bf16)


def stair(B, T, H, seed, bf16=False, step=9):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, 3, H, 64, generator=g)
    x[:, :, 0] *= 0.25
    x[:, :, 1] *= 0.5
    grp = torch.arange(T) // 32
    # k_0 = a quarter of the centred group index and q_0 = bf16(step * 8 / (log2 e / 4)): both bf16-exact, so no kernel rounds them
    x[:, :, 1, :, 0] = ((grp - ((T - 1) // 32) // 2).float() * 0.25)[None, :, None]
    x[:, :, 0, :, 0] = float(torch.tensor(step * 8.0 / (LOG2E * 0.25)).bfloat16())
    return _finish(x, bf16)


def bait(B, T, H, seed, bf16=False, mag=MAG_BAIT):
    assert B == 2, "bait is a two-image probe"
    g = torch.Generator().manual_seed(seed)
    n = min(T, 128)
    x = torch.randn(2, T, 3, H, 64, generator=g)
    x[:, :, 1] = (mag * _units(g, 2, T, H)).float()
    u, w = _units(g, n, H).float(), _units(g, n, H).float()                 # (n,H,64)
    rep = torch.arange(T) % n
    x[0, :, 0] = mag * u[rep]          # image 0's queries look for u ...
    x[1, :n, 1] = 2 * mag * u          # ... which image 1's first key rows hold, twice as large as anything in image 0
    x[1, :, 0] = mag * w[rep]
    x[0, T - n:, 1] = 2 * mag * w
    return _finish(x, bf16)


FAMILIES = {"sharp": sharp, "match": match, "lastkey": lastkey,
            "stair+9": lambda *a, **k: stair(*a, step=9, **k), "stair+5": lambda *a, **k: stair(*a, step=5, **k),
            "stair-9": lambda *a, **k: stair(*a, step=-9, **k), "bait": bait}


def sharp_on_device(B, T, H, seed, device):
    """`sharp` drawn on the device directly as bf16 (the 2-GiB cases: 1.07e9 values), (B,T,3 H 64)."""
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn(B, T, 3, H * 64, generator=g, device=device, dtype=torch.bfloat16)
    x[:, :, 0] *= 2.0
    return x.reshape(B, T, 3 * H * 64)
