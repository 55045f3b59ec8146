"""GPU: the dense layers' focused linear attention -- csrc/linattn.hip (linear_attn_kernel<0/1> in bf16, linear_attn_f32_kernel<0/1> in
the fp32 class, linear_attn_kv_state_kernel) and `ops.focused_linear_attention` -- against a plain float64 reference, across query
counts, key counts, batches, row windows, per-channel scales and adversarial values.

Reference (LinearAttention.forward): q0 = (relu(y) + 1e-6) s with s = 1 / softplus(scale) per channel; the focusing
q = q0^3 |q0| / |q0^3| with both norms over the whole 256-channel row; keys alike; per head h (64 channels)
out_h = z q_h K_h with K_h[c][d] = sum_j k_jc v_jd and z = 1 / (q_h . S_h + 1e-6), S = sum_j k_j.  Everything is float64, from
exactly the operands the path sees (the bf16-rounded inputs; at kernel level the kvt and ksum passed in).  u = 2^-24 is the fp32 unit
roundoff and u_b = 2^-8 the bf16 one (8 significant bits, round to nearest: half of a 2^-7 spacing).  Each result element is checked
against a bound derived from the arithmetic (`attend`); the magnitude the roundings scale with is z P_d, P_d = sum_c q_c |K_cd| (at op
level the larger M_d = z sum_c q_c sum_j k_jc |v_jd|: the per-key magnitude, which a sum that cancels does not shrink).  q, k > 0.
  * fp32 focusing (`EPS_F`): relu + 1e-6 and the scale (2u), the cube (8u), the squared sums (5u and 17u per term) summed over 128
    terms per lane plus one exchange (129u), two square roots and a division: fac within (134 + 146) / 2 + 3 = 143u; the focused value
    within 8 + 143 + 1 = 152u.  EPS_F = 160u.  The op-level scale 1 / softplus is fp32 arithmetic as well: 8u more per channel.
  * bf16 mode 0: q rounded to bf16 for the MFMA (u_b + EPS_F), the kvt operand exact, 64 exact products summed in fp32 (64u of
    sum q |K|); z from the unrounded fp32 q (EPS_F) and ksum summed over 32 + 1 terms (33u of q . S), the + 1e-6 and the reciprocal
    (2u); the product acc * z (u) and the bf16 store (u_b of the value).  Together about (u_b + 2 EPS_F + 100u) z P + u_b |out|.
  * fp32 mode 0: the hi / lo split holds each operand to 2^-16 of itself (hi = bf16(x): |x - hi| <= 2^-8 |x|, lo = bf16(x - hi) within
    2^-8 of that) and drops lo.lo (<= 2^-16 |a||b|): 3 x 2^-16 per product (`SPLIT`), 3 x 64 = 192 fp32 accumulations, the z terms as
    above, an fp32 store: about 2^-14 z P + 2u |out|.
  * mode 1 (focused features): EPS_F |q|, and the bf16 store u_b |q| on top in bf16.
  * kv_state: the kernel's focused keys are bf16(k) of an fp32 value within EPS_F |k|: the reference takes bf16 of the float64 key and
    allows the neighbour where k -+ EPS_F |k| rounds to another bf16 value (`rounded`).  ksum is then exact up to that and J u of the
    fp32 sum; kvt up to that, J u of its fp32 sum (exact bf16 products) and the bf16 store u_b |kvt|.
  * op level: the projections' own rounding enters as an interval of each projected value (bf16: one GEMM with its bias, fp32
    accumulation of 256 exact products within 2^-16 of sum |x||W| + |b|, rounded once to bf16 as the reference rounds the float64
    value, neighbour allowed: `rounded`; fp32: the split GEMMs, 3 x 2^-16 per product plus 2^-16 of accumulation: 2^-14 of the
    absolute sum).  relu and the scale are monotone,
    so each q0 lies in [q0_lo, q0_hi] and the focused value in [q_lo^3 |q_lo| / |q_hi^3|, q_hi^3 |q_hi| / |q_lo^3|] (the cube's 3x and
    the norms' rescale, exactly); keys alike.  kvt and ksum then carry the keys' and values' intervals, their fp32 sums, the kv
    contraction's split (7-launch route) and the bf16 store of kvt.
`attend` propagates all of it: |d num| <= sum_c (dq_c |K_cd| + (q_c + dq_c) dK_cd) + g_num sum_c (q_c + dq_c)(|K_cd| + dK_cd),
rho = |d den| / den, |d out| <= z |d num| + (|out| + z |d num|) rho / (1 - rho), then the multiply and the store.
The mean error is checked as well on random data: a rounding error spread evenly over its interval averages half its maximum, and a
sum of them no more than the sum of those halves, so the mean error must stay within MEAN_FRAC = 1/2 of the mean bound.  A
systematic error (a wrong scale channel, a dropped term) moves every element and fails it.
Out of scope: 1 / softplus(scale) < 1/2 together with rows the ReLU kills.  A dead row is 1e-6 s in every channel and its sixth powers
(1e-6 s)^6 leave the normal fp32 range there, in any fp32 implementation of the reference as well; the scales here span 0.6 to 20.
The padding rows of the kernels' last tile are such rows by construction; `test_tiny_scale_padding_rows_stay_out` checks that they
contribute nothing even at s = 1e-3."""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
U, U_B = 2.0 ** -24, 2.0 ** -8
EPS = float(torch.tensor(1e-6, dtype=torch.float32))  # the kernels' and the fp32 reference's 1e-6
EPS_F = 160 * U
SPLIT = 3 * 2.0 ** -16
MEAN_FRAC = 0.5
TINY = 1e-300
NAN_BITS = {BF: 0x7FE5, F32: 0x7FE5A5A5}  # a NaN with a payload no kernel produces: a guard element must keep these bits
INT_OF = {BF: torch.int16, F32: torch.int32}


def _lib():
    from unopose_amd import _lib

    return _lib


def vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _call(name, *args):
    _lib().call(name, *args)


def _s():
    return _lib().stream_ptr()


# ------------------------------------------------------------------------------------------ float64 reference and its bound
def focus(y, s, dy=None, p=3):
    """Focused rows of y (..., C) with per-channel scale s, float64.  With dy (absolute uncertainty of y) also the uncertainty of the
    result: the interval of the focusing over y -+ dy."""
    y, s = y.double(), s.double()
    nrm = lambda t: t.norm(dim=-1, keepdim=True)  # noqa: E731
    q0 = (y.clamp_min(0) + EPS) * s
    q = q0 ** p * (nrm(q0) / nrm(q0 ** p))
    if dy is None:
        return q
    lo = ((y - dy).clamp_min(0) + EPS) * s
    hi = ((y + dy).clamp_min(0) + EPS) * s
    q_lo = lo ** p * (nrm(lo) / nrm(hi ** p))
    q_hi = hi ** p * (nrm(hi) / nrm(lo ** p))
    return q, torch.maximum(q_hi - q, q - q_lo)


def rounded(y, eps):
    """bf16(y) and its uncertainty when the path computes y to within eps before rounding: 0 unless y - eps or y + eps rounds to
    another bf16 value (then the farther of those)."""
    yr = y.to(BF).double()
    return yr, torch.maximum(((y - eps).to(BF).double() - yr).abs(), ((y + eps).to(BF).double() - yr).abs())


def attend(q, K, S, *, heads=4, dq=None, dqz=None, dK=None, dS=None, Ka=None, g_num, g_den, out_rel):
    """q (B,N,C) focused queries; K (B,h,d,c) = sum_j v_jd k_jc per head (the kernel's kvt layout); S (B,C) = sum_j k_j.
    dq: uncertainty of the q the contraction uses, dqz: of the q in z; dK, dS: of the operands; Ka: the magnitude of K the path's sums
    scale with (default |K|); g_num / g_den: relative error of the sums sum_c q_c Ka_cd and q . S; out_rel: the store's rounding.
    Returns (out, bound), (B,N,C) float64."""
    B, N, C = q.shape
    hd = C // heads
    z0 = lambda t, sh: torch.zeros(sh, dtype=torch.float64, device=q.device) if t is None else t.double().reshape(sh)  # noqa: E731
    q4 = q.double().reshape(B, N, heads, hd)
    dq4, dqz4 = z0(dq, q4.shape), z0(dqz, q4.shape)
    K = K.double()
    dK = z0(dK, K.shape)
    Ka = K.abs() if Ka is None else Ka.double()
    S4, dS4 = S.double().reshape(B, heads, hd), z0(dS, (B, heads, hd))
    num = torch.einsum("bnhc,bhdc->bnhd", q4, K)
    qs = torch.einsum("bnhc,bhc->bnh", q4, S4)
    den = qs + EPS
    out = num / den.unsqueeze(-1)
    qq = q4 + dq4
    dnum = (torch.einsum("bnhc,bhdc->bnhd", dq4, Ka) + torch.einsum("bnhc,bhdc->bnhd", qq, dK)
            + g_num * torch.einsum("bnhc,bhdc->bnhd", qq, Ka + dK))
    dden = (torch.einsum("bnhc,bhc->bnh", dqz4, S4) + torch.einsum("bnhc,bhc->bnh", q4 + dqz4, dS4)
            + g_den * torch.einsum("bnhc,bhc->bnh", q4 + dqz4, S4 + dS4) + 2 * U * den)
    rho = dden / den
    assert (rho < 0.5).all(), "the denominator's uncertainty is not small: the bound does not apply"
    zd = dnum / den.unsqueeze(-1)
    E1 = zd + (out.abs() + zd) * (rho / (1 - rho)).unsqueeze(-1)
    bound = E1 + (out_rel + U) * (out.abs() + E1) + TINY
    return out.reshape(B, N, C), bound.reshape(B, N, C)


def check(out, ref, bound, what="", mean=True):
    e = (out.double() - ref).abs()
    bad = ~(e <= bound)  # (NaN fails)
    if bad.any():
        idx = tuple(int(i) for i in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {e.numel()} elements outside the bound; first at {idx}: got "
                             f"{out[idx].item()!r}, want {ref[idx].item()!r} +- {bound[idx].item():.3e}")
    em, bm = e.mean().item(), bound.mean().item()
    assert not mean or em <= MEAN_FRAC * bm, f"{what}: mean error {em:.3e} vs mean bound {bm:.3e}"


# ------------------------------------------------------------------------------------------ operands and kernel calls
def wide_scale(g, lo=0.6, hi=20.0, C=256):
    """The learned `scale` parameter (fp32) with 1 / softplus(scale) log-uniform over [lo, hi], and that 1 / softplus as the host
    forms it (fp32)."""
    inv = torch.exp(math.log(lo) + (math.log(hi) - math.log(lo)) * torch.rand(C, generator=g, device="cuda", dtype=torch.float64))
    scale = torch.log(torch.expm1(1.0 / inv)).float()
    return scale, (1.0 / torch.nn.functional.softplus(scale)).contiguous()


def la(x, s, kvt, ksum, mode, dt, out=None):
    """One launch of linear_attn(_f32)_kernel<mode> into a NaN-prefilled output (every element must be written)."""
    B, N, _ = x.shape
    if out is None:
        out = torch.full((B, N, 256), float("nan"), dtype=dt, device="cuda")
    name = "unopose_linear_attention" if dt == BF else "unopose_linear_attention_f32"
    _call(name, vp(x), vp(s), vp(kvt), vp(ksum), B, N, 3, mode, vp(out), _s())
    return out


def kv_state(ykv, s, B, J, rows, first, kvt=None, ksum=None):
    if kvt is None:
        kvt = torch.full((B, 4, 64, 64), float("nan"), dtype=BF, device="cuda")
        ksum = torch.full((B, 256), float("nan"), device="cuda")
    _call("unopose_linear_attention_kv_state", vp(ykv), vp(s), B, J, rows, first, 3, vp(kvt), vp(ksum), _s())
    return kvt, ksum


def state_of(k, v, s, dt):
    """The kvt / ksum a mode-0 launch is fed, formed in float64 from the independently focused keys (bf16-rounded in bf16)."""
    kf = focus(k, s).to(dt).double()
    B, J, _ = kf.shape
    ksum = kf.sum(1).float().contiguous()
    kvt = torch.einsum("bjhd,bjhc->bhdc", v.double().reshape(B, J, 4, 64), kf.reshape(B, J, 4, 64)).to(dt).contiguous()
    return kvt, ksum


def ref_mode0(x, s, kvt, ksum, dt):
    q = focus(x, s)
    if dt == BF:
        return attend(q, kvt, ksum, dq=(U_B + EPS_F * (1 + U_B)) * q, dqz=EPS_F * q, g_num=64 * U, g_den=33 * U, out_rel=U_B)
    return attend(q, kvt, ksum, dq=EPS_F * q, dqz=EPS_F * q, g_num=SPLIT + 192 * U, g_den=33 * U, out_rel=U)


def ref_mode1(x, s, dt):
    q = focus(x, s)
    return q, (EPS_F + (U_B * (1 + EPS_F) if dt == BF else 0.0)) * q + TINY


def ref_kv_state(k, v, s):
    """float64 kvt (B,4,64,64) and ksum (B,256) of the bf16 focused keys, with their bounds."""
    B, J, _ = k.shape
    kf = focus(k, s)
    kb, dkb = rounded(kf, EPS_F * kf)
    va = v.double().abs().reshape(B, J, 4, 64)
    kb4, dkb4 = kb.reshape(B, J, 4, 64), dkb.reshape(B, J, 4, 64)
    ks = kb.sum(1)
    ks_bound = dkb.sum(1) + J * U * (kb + dkb).sum(1) + TINY
    kv = torch.einsum("bjhd,bjhc->bhdc", v.double().reshape(B, J, 4, 64), kb4)
    A = torch.einsum("bjhd,bjhc->bhdc", va, dkb4) + J * U * torch.einsum("bjhd,bjhc->bhdc", va, kb4 + dkb4)
    return kv, (1 + U_B) * A + U_B * kv.abs() + TINY, ks, ks_bound


def check_state(kvt, ksum, k, v, s, what):
    kv, kv_b, ks, ks_b = ref_kv_state(k, v, s)
    check(ksum, ks, ks_b, f"{what} ksum", mean=False)  # (bounds of 0 where no key sits near a rounding boundary)
    check(kvt, kv, kv_b, f"{what} kvt", mean=False)


def operands(dt, B, N, J, seed, qs=1.0, ks=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = (torch.randn(B, N, 256, generator=g, device="cuda") * qs).to(dt)
    k = (torch.randn(B, J, 256, generator=g, device="cuda") * ks).to(dt)
    v = torch.randn(B, J, 256, generator=g, device="cuda").to(dt)
    return g, x, k, v


def run_kernels(dt, x, k, v, s, what, mean=True):
    """Mode 1 on the queries and mode 0 with a float64-formed state, both against the reference; bf16: kv_state on [k | v] too."""
    kvt, ksum = state_of(k, v, s, dt)
    check(la(x, s, None, None, 1, dt), *ref_mode1(x, s, dt), f"{what} mode 1", mean=mean)
    check(la(x, s, kvt, ksum, 0, dt), *ref_mode0(x, s, kvt, ksum, dt), f"{what} mode 0", mean=mean)
    if dt == BF:
        B, J, _ = k.shape
        kvt2, ksum2 = kv_state(torch.cat([k, v], -1), s, B, J, J, 0)
        check_state(kvt2, ksum2, k, v, s, what)


DTS = [pytest.param(BF, id="bf16"), pytest.param(F32, id="f32")]
SWEEP_N = [1, 31, 32, 33, 127, 128, 129, 2047, 2048, 2049, 4096, 4097]


# ------------------------------------------------------------------------------------------ kernel shapes
@torch.no_grad()
@pytest.mark.parametrize("N", SWEEP_N)
@pytest.mark.parametrize("dt", DTS)
def test_kernel_shapes(dt, N):
    """Both modes at every position of the last 32-row wave and 128-row workgroup, 1 and 3 pairs, wide per-channel scales."""
    for B in (1, 3):
        g, x, k, v = operands(dt, B, N, 196, seed=10 * N + B)
        _, s = wide_scale(g)
        run_kernels(dt, x, k, v, s, f"B={B} N={N}")


@torch.no_grad()
@pytest.mark.parametrize("dt", DTS)
def test_kernel_stacked_batch(dt):
    """B = 64 (2 x 32 stacked pairs), ragged N: the batch index of every pair."""
    g, x, k, v = operands(dt, 64, 33, 196, seed=64)
    _, s = wide_scale(g)
    run_kernels(dt, x, k, v, s, "B=64")


@torch.no_grad()
@pytest.mark.parametrize("J", [1, 7, 31, 127, 128, 129, 196, 256, 257, 300])
def test_kv_state_shapes(J):
    """Rounds of 128 keys ending anywhere; 1, 3 and 64 pairs."""
    for B in (1, 3, 64):
        g, _, k, v = operands(BF, B, 1, J, seed=J * 100 + B)
        _, s = wide_scale(g)
        check_state(*kv_state(torch.cat([k, v], -1), s, B, J, J, 0), k, v, s, f"B={B} J={J}")


@torch.no_grad()
@pytest.mark.parametrize("fill", ["nan", "huge"])
@pytest.mark.parametrize("first", [0, 1, 5])
@pytest.mark.parametrize("J", [1, 31, 196, 257])
def test_kv_state_window(J, first, fill):
    """Keys as rows [first, first + J) of rows_per_pair > first + J rows: every other row (and a 128-row tail after the last pair)
    holds NaN or -+3e38.  The state must equal the compact call's (whose rows are followed by NaN) bit for bit."""
    B, rows = 3, first + J + 3
    g, _, k, v = operands(BF, B, 1, J, seed=J + 17 * first)
    _, s = wide_scale(g)
    ykv = _in_pool(torch.cat([k, v], -1), 128 * 512)
    want = kv_state(ykv, s, B, J, J, 0)
    pool = torch.empty(B * rows * 512 + 128 * 512, dtype=BF, device="cuda")
    if fill == "nan":
        pool.fill_(float("nan"))
    else:
        pool.copy_(3e38 * torch.sign(torch.randn(pool.numel(), generator=g, device="cuda")))
    wide = pool[: B * rows * 512].view(B, rows, 512)
    wide[:, first:first + J] = ykv
    got = kv_state(wide, s, B, J, rows, first)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), "windowed state differs from the compact one"
    check_state(*got, k, v, s, f"window {first}")


# ------------------------------------------------------------------------------------------ adversarial values
ADV = ["dead_rows", "dead_heads", "dead_keys", "dominant", "large", "cancel"]


def adversarial(case, dt, B, N, J, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *sh: torch.randn(*sh, generator=g, device="cuda")  # noqa: E731
    x, k, v = r(B, N, 256), r(B, J, 256), r(B, J, 256)
    if case == "dead_rows":  # every third query and fifth key row: all 256 channels <= 0
        x[:, ::3] = -x[:, ::3].abs()
        k[:, ::5] = -k[:, ::5].abs()
    elif case == "dead_heads":  # one head of most rows <= 0 (head = row mod 4; every fifth row keeps all four)
        for h in range(4):
            x[:, h::5, h * 64:(h + 1) * 64] = -x[:, h::5, h * 64:(h + 1) * 64].abs()
            k[:, h::5, h * 64:(h + 1) * 64] = -k[:, h::5, h * 64:(h + 1) * 64].abs()
    elif case == "dead_keys":  # all keys dead: q . S ~ 1e-6 for the dead and the faint queries, so the + 1e-6 carries z
        k = -k.abs()
        x = x * 10.0 ** (-7 + 6 * torch.rand(B, N, 1, generator=g, device="cuda"))
        x[:, ::4] = -x[:, ::4].abs()
    elif case == "dominant":  # one channel per row far above the rest: the cube hands it nearly all of the row
        x, k = 0.1 * x, 0.1 * k
        x.scatter_(2, torch.randint(0, 256, (B, N, 1), generator=g, device="cuda"), 8.0)
        k.scatter_(2, torch.randint(0, 256, (B, J, 1), generator=g, device="cuda"), 8.0)
    elif case == "large":  # |y| up to 50: q0 up to 1000, its cube 1e9 and the sum of squares ~1e20
        x = 50.0 * (2 * torch.rand(B, N, 256, generator=g, device="cuda") - 1)
        k = 50.0 * (2 * torch.rand(B, J, 256, generator=g, device="cuda") - 1)
    elif case == "cancel":  # keys in identical pairs with opposite v (+ 1e-3 noise): kv ~ 0 while sum k |v| is not
        h = J // 2
        k[:, h:2 * h] = k[:, :h]
        v[:, h:2 * h] = -v[:, :h] + 1e-3 * r(B, h, 256)
    return g, x.to(dt), k.to(dt), v.to(dt)


@torch.no_grad()
@pytest.mark.parametrize("case", ADV)
@pytest.mark.parametrize("dt", DTS)
def test_adversarial_values(dt, case):
    B, N, J = 2, 129, 196
    g, x, k, v = adversarial(case, dt, B, N, J, seed=ADV.index(case))
    _, s = wide_scale(g)
    run_kernels(dt, x, k, v, s, case, mean=case not in ("dead_keys", "cancel"))  # (there one rounding dominates many elements)
    if case == "dead_keys":  # the + 1e-6 is a large share of the denominator of many rows: a kernel that drops it fails above
        kvt, ksum = state_of(k, v, s, dt)
        q = focus(x, s).reshape(B, N, 4, 64)
        qs = torch.einsum("bnhc,bhc->bnh", q, ksum.double().reshape(B, 4, 64))
        assert (qs < 10 * EPS).float().mean().item() > 0.1 and (qs > 0.1 * EPS).float().mean().item() > 0.1, "dead-key case lost its point"


@torch.no_grad()
def test_tiny_scale_padding_rows_stay_out():
    """1 / softplus = 1e-3 and every channel of the real rows live (y in [500, 1500]): the zero rows a kernel pads its last tile with
    focus to inf there ((1e-9)^6 underflows), so they must not reach kvt / ksum (kv_state: J = 7, 196) nor any real row (mode 0 / 1,
    ragged N = 33, 129)."""
    g = torch.Generator(device="cuda").manual_seed(5)
    s = torch.full((256,), 1e-3, device="cuda")
    for dt in (BF, F32):
        for N, J in ((33, 7), (129, 196)):
            B = 2
            x = (500 + 1000 * torch.rand(B, N, 256, generator=g, device="cuda")).to(dt)
            k = (500 + 1000 * torch.rand(B, J, 256, generator=g, device="cuda")).to(dt)
            v = torch.randn(B, J, 256, generator=g, device="cuda").to(dt)
            run_kernels(dt, x, k, v, s, f"tiny scale N={N} J={J}", mean=False)


# ------------------------------------------------------------------------------------------ output hygiene
def _pool(shape, dt, guard):
    """A NaN-payload-filled allocation: the view of `shape` at its front and the `guard` elements after it."""
    n = math.prod(shape)
    p = torch.empty(n + guard, dtype=dt, device="cuda")
    p.view(INT_OF[dt]).fill_(NAN_BITS[dt])
    return p[:n].view(shape), p[n:]


def _in_pool(t, guard):
    view, tail = _pool(t.shape, t.dtype, guard)
    view.copy_(t)
    return view


def _clean(view, tail, what):
    assert torch.isfinite(view.float()).all(), f"{what}: an element was left unwritten or is not finite"
    assert (tail.view(INT_OF[tail.dtype]) == NAN_BITS[tail.dtype]).all(), f"{what}: a guard element after the output was written"


@torch.no_grad()
@pytest.mark.parametrize("dt", DTS)
def test_output_hygiene(dt):
    """All five outputs into NaN-prefilled buffers with guard elements after them (32 rows after B N 256, a whole 32-row wave's
    worth; 4096 after kvt, 256 after ksum): every in-range element written and finite, every guard element untouched.  Inputs sit
    in NaN-tailed allocations too."""
    B, N, J = 2, 129, 197
    g, x, k, v = operands(dt, B, N, J, seed=99)
    _, s = wide_scale(g)
    x = _in_pool(x, 32 * 256)
    kvt, ksum = state_of(k, v, s, dt)
    kvt, ksum = _in_pool(kvt, 4096), _in_pool(ksum, 256)
    for mode in (0, 1):
        out, tail = _pool((B, N, 256), dt, 32 * 256)
        la(x, s, kvt, ksum, mode, dt, out)
        torch.cuda.synchronize()
        _clean(out, tail, f"mode {mode}")
        ref = ref_mode0(x, s, kvt, ksum, dt) if mode == 0 else ref_mode1(x, s, dt)
        check(out, *ref, f"mode {mode}")
    if dt == BF:
        ykv = _in_pool(torch.cat([k, v], -1), 128 * 512)
        kvt2, kt = _pool((B, 4, 64, 64), BF, 4096)
        ksum2, st = _pool((B, 256), F32, 256)
        kv_state(ykv, s, B, J, J, 0, kvt2, ksum2)
        torch.cuda.synchronize()
        _clean(kvt2, kt, "kvt")
        _clean(ksum2, st, "ksum")
        check_state(kvt2, ksum2, k, v, s, "kv_state")


# ------------------------------------------------------------------------------------------ ABI
@torch.no_grad()
def test_abi_rejects_bad_arguments():
    """Each entry point returns an error and launches nothing (its NaN-prefilled outputs keep their bits)."""
    s = torch.ones(256, device="cuda")
    for dt in (BF, F32):
        name = "unopose_linear_attention" if dt == BF else "unopose_linear_attention_f32"
        x = torch.ones(2, 40, 256, dtype=dt, device="cuda")
        kvt = torch.zeros(2, 4, 64, 64, dtype=dt, device="cuda")
        ksum = torch.ones(2, 256, device="cuda")
        out = torch.full((2, 40, 256), float("nan"), dtype=dt, device="cuda")
        bad = [((vp(x), vp(s), vp(kvt), vp(ksum), 2, 40, 2, 0), "focusing_factor"),
               ((vp(x), vp(s), None, None, 2, 40, 4, 1), "focusing_factor"),
               ((vp(x), vp(s), vp(kvt), vp(ksum), 2, 0, 3, 0), "bad sizes"),
               ((vp(x), vp(s), vp(kvt), vp(ksum), 2, -1, 3, 1), "bad sizes"),
               ((vp(x), vp(s), None, vp(ksum), 2, 40, 3, 0), "null pointer"),
               ((vp(x), vp(s), vp(kvt), None, 2, 40, 3, 0), "null pointer")]
        for args, msg in bad:
            with pytest.raises(RuntimeError, match=msg):
                _call(name, *args, vp(out), _s())
        torch.cuda.synchronize()
        assert out.isnan().all(), f"{name}: a rejected call wrote its output"
    ykv = torch.ones(2, 10, 512, dtype=BF, device="cuda")
    kvt = torch.full((2, 4, 64, 64), float("nan"), dtype=BF, device="cuda")
    ksum = torch.full((2, 256), float("nan"), device="cuda")
    bad = [((2, 7, 10, 0, 2), "focusing_factor"), ((2, 0, 10, 0, 3), "bad sizes"), ((2, 8, 10, 3, 3), "bad sizes"),
           ((2, 7, 10, -1, 3), "bad sizes"), ((2, 11, 10, 0, 3), "bad sizes")]
    for (B, J, rows, first, focus_), msg in bad:
        with pytest.raises(RuntimeError, match=msg):
            _call("unopose_linear_attention_kv_state", vp(ykv), vp(s), B, J, rows, first, focus_, vp(kvt), vp(ksum), _s())
    with pytest.raises(RuntimeError, match="null pointer"):
        _call("unopose_linear_attention_kv_state", vp(ykv), vp(s), 2, 7, 10, 0, 3, None, vp(ksum), _s())
    torch.cuda.synchronize()
    assert kvt.isnan().all() and ksum.isnan().all(), "a rejected kv_state call wrote its outputs"


# ------------------------------------------------------------------------------------------ op level
def _att(seed, C=256):
    from unopose_amd.model.modules import _LinearAttention

    torch.manual_seed(seed)
    att = _LinearAttention(C).cuda().eval()
    g = torch.Generator(device="cuda").manual_seed(seed)
    with torch.no_grad():
        for lin in (att.proj_q, att.proj_k, att.proj_v):
            lin.weight.normal_(0, C ** -0.5)
            lin.bias.normal_(0, 0.1)
        att.scale.copy_(wide_scale(g, C=C)[0].reshape(1, 1, C))
    return att


def op_reference(xq, xkv, att, prec, heads=4, focusing=3, composite=False):
    """float64 LinearAttention.forward from the module's weights, with the path's rounding points modelled (module docstring)."""
    bf = prec == "bf16"
    r = (lambda t: t.detach().to(BF).double()) if bf else (lambda t: t.detach().double())  # noqa: E731

    def proj(a, lin):
        w, b = r(lin.weight), r(lin.bias)
        y, ya = a @ w.T + b, a.abs() @ w.abs().T + b.abs()
        return rounded(y, 2.0 ** -16 * ya) if bf else (y, 2.0 ** -14 * ya)

    xd, md = r(xq), r(xkv)
    s = 1.0 / torch.nn.functional.softplus(att.scale.detach().double()).reshape(-1)
    yq, dyq = proj(xd, att.proj_q)
    yk, dyk = proj(md, att.proj_k)
    v, dv = proj(md, att.proj_v)
    q, dq = focus(yq, s, dyq, focusing)
    k, dk = focus(yk, s, dyk, focusing)
    f = EPS_F + 8 * U  # the fp32 focusing and the fp32 1 / softplus
    dq, dk = dq + f * (q + dq), dk + f * (k + dk)
    B, J, C = k.shape
    hd = C // heads
    k4, dk4 = k.reshape(B, J, heads, hd), dk.reshape(B, J, heads, hd)
    v4, va4, dv4 = v.reshape(B, J, heads, hd), v.abs().reshape(B, J, heads, hd), dv.reshape(B, J, heads, hd)
    K = torch.einsum("bjhd,bjhc->bhdc", v4, k4)
    Ka = torch.einsum("bjhd,bjhc->bhdc", va4, k4)  # M_d / z
    if bf:
        dk = dk + U_B * (k + dk)  # the focused keys are stored as bf16
        dk4 = dk.reshape(B, J, heads, hd)
    G = torch.einsum("bjhd,bjhc->bhdc", va4 + dv4, k4 + dk4)
    dK = torch.einsum("bjhd,bjhc->bhdc", va4 + dv4, dk4) + torch.einsum("bjhd,bjhc->bhdc", dv4, k4)
    S, dS = k.sum(1), dk.sum(1) + J * U * (k + dk).sum(1)
    if composite:  # fp32 torch: kv or qk form, fp32 sums of hd and J terms
        return attend(q, K, S, heads=heads, dq=dq, dqz=dq, dK=dK, dS=dS, Ka=Ka, g_num=(J + 2 * hd) * U, g_den=(J + hd) * U,
                      out_rel=0.0)
    dK = dK + (SPLIT + 3 * J * U) * G  # the kv contraction (fp32 MFMAs, or the split fp32 GEMM of the 7-launch route)
    if bf:
        dK = dK + U_B * (G + dK)  # kvt stored as bf16
        return attend(q, K, S, dq=dq + U_B * (q + dq), dqz=dq, dK=dK, dS=dS, Ka=Ka, g_num=64 * U, g_den=33 * U, out_rel=U_B)
    return attend(q, K, S, dq=dq, dqz=dq, dK=dK, dS=dS, Ka=Ka, g_num=SPLIT + 192 * U, g_den=33 * U, out_rel=U)


def _op(xq, xkv, att, prec, kv_skip=0, heads=4, focusing=3):
    from unopose_amd import ops

    with torch.autocast("cuda", dtype=BF, enabled=prec == "bf16"):
        return ops.focused_linear_attention(xq, xkv, att, heads, focusing, kv_skip=kv_skip)


@torch.no_grad()
@pytest.mark.parametrize("J", [1, 196, 300])
@pytest.mark.parametrize("N", [1, 2048, 2049, 4096])
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_op_focused_linear_attention(prec, N, J):
    """ops.focused_linear_attention on a _LinearAttention with random weights and wide per-channel scales, fp32 and under bf16
    autocast.  bf16: the 7-launch route (USE_LA_KV_STATE off) within the same bound, and within 2 u_b (|out| + z M) + 2 J u z M of the
    one-launch route (one bf16 step of the output, one of any kvt element, the fp32 sums' order; 4 u_b of it for second-order terms)."""
    from unopose_amd import ops

    att = _att(N + J)
    g = torch.Generator(device="cuda").manual_seed(N * 7 + J)
    xq = torch.randn(2, N, 256, generator=g, device="cuda")
    xkv = torch.randn(2, J, 256, generator=g, device="cuda")
    out = _op(xq, xkv, att, prec)
    assert out.dtype == (BF if prec == "bf16" else F32) and out.shape == xq.shape
    ref, bound = op_reference(xq, xkv, att, prec)
    check(out, ref, bound, f"{prec} N={N} J={J}")
    if prec == "bf16":
        ops.USE_LA_KV_STATE = False
        try:
            old = _op(xq, xkv, att, prec)
        finally:
            ops.USE_LA_KV_STATE = True
        check(old, ref, bound, f"7-launch N={N} J={J}")
        zM = attend_magnitude(xq, xkv, att)
        mag = torch.maximum(old.double().abs(), out.double().abs())
        tol = (1 + 4 * U_B) * (2 * U_B * (mag + zM) + 2 * J * U * zM)
        assert ((old.double() - out.double()).abs() <= tol).all(), "the two kv-state routes differ by more than their rounding"


def attend_magnitude(xq, xkv, att):
    """z M_d of the bf16 path's operands (float64)."""
    r = lambda t: t.detach().to(BF).double()  # noqa: E731
    s = 1.0 / torch.nn.functional.softplus(att.scale.detach().double()).reshape(-1)
    p = lambda a, lin: (a @ r(lin.weight).T + r(lin.bias)).to(BF).double()  # noqa: E731
    q, k, v = focus(p(r(xq), att.proj_q), s), focus(p(r(xkv), att.proj_k), s), p(r(xkv), att.proj_v)
    B, N, _ = q.shape
    J = k.shape[1]
    Ka = torch.einsum("bjhd,bjhc->bhdc", v.abs().reshape(B, J, 4, 64), k.reshape(B, J, 4, 64))
    q4 = q.reshape(B, N, 4, 64)
    z = 1.0 / (torch.einsum("bnhc,bhc->bnh", q4, k.sum(1).reshape(B, 4, 64)) + EPS)
    return (torch.einsum("bnhc,bhdc->bnhd", q4, Ka) * z.unsqueeze(-1)).reshape(B, N, 256)


@torch.no_grad()
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_op_kv_skip_background_row(prec):
    """kv_skip = 1 on a stacked (2B, 1 + J, 256) block whose background row is NaN (SparseToDenseTransformer.forward_stacked): bit-equal
    to the call on xkv[:, 1:], and within the bound."""
    att = _att(3)
    g = torch.Generator(device="cuda").manual_seed(3)
    xq = torch.randn(4, 2049, 256, generator=g, device="cuda")
    blk = torch.randn(4, 197, 256, generator=g, device="cuda")
    blk[:, 0] = float("nan")
    got = _op(xq, blk, att, prec, kv_skip=1)
    want = _op(xq, blk[:, 1:].contiguous(), att, prec)
    assert torch.equal(got, want), "kv_skip = 1 differs from the sliced call"
    check(got, *op_reference(xq, blk[:, 1:], att, prec), f"{prec} kv_skip")


@torch.no_grad()
@pytest.mark.parametrize("heads,focusing", [(8, 3), (4, 2)])
def test_op_composite_for_other_configurations(heads, focusing, monkeypatch):
    """heads != 4 or focusing != 3 is not what the kernels are built for: the fp32 torch composite runs, with its RuntimeWarning, and
    matches the reference."""
    from unopose_amd.ops import common

    monkeypatch.setattr(common, "_fallbacks_seen", set())
    att = _att(heads * 10 + focusing)
    g = torch.Generator(device="cuda").manual_seed(heads)
    xq = torch.randn(2, 2049, 256, generator=g, device="cuda")
    xkv = torch.randn(2, 196, 256, generator=g, device="cuda")
    with pytest.warns(RuntimeWarning, match="focused_linear_attention"):
        out = _op(xq, xkv, att, "fp32", heads=heads, focusing=focusing)
    check(out, *op_reference(xq, xkv, att, "fp32", heads, focusing, composite=True), f"composite heads={heads} focusing={focusing}")
