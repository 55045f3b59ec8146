"""Float64 reference, test data, a-priori tolerances and two fp32 models of the training-mode BatchNorm2d + ReLU (+ max-pool) of
csrc/bn_train.hip.  Nothing here is used by the package; test_bn_train_ref_cpu.py checks all of it without a GPU and
test_bn_train_gpu.py holds the kernels against it.

Reference (`reference`), plain torch float64 on the CPU from the fp32 inputs, M = B N S values per channel:

    mean = sum x / M,  var = sum (x - mean)^2 / M (biased),  rstd = 1 / sqrt(var + eps),  xhat = (x - mean) rstd
    z = gamma xhat + beta,  y = max(z, 0);   pooled: out = max_s y, the gradient g of a row goes to its first arg max
    dz = dy [z > 0],  dbeta = sum dz,  dgamma = sum dz xhat,  dx = gamma rstd (dz - dbeta / M - xhat dgamma / M)
    running_mean <- (1 - m) running_mean + m mean,   running_var <- (1 - m) running_var + m var M / (M - 1)

Data (`make_case`): one tensor carries every family, a channel has its own (offset, sigma) -- FAMILIES, repeated every 12 channels.
u = round(randn / q) q clipped to +-6 lies on a lattice of step q (pooled op: plus column * colstep, which makes the S values of a row
distinct), x = fp32(offset + sigma u).  q = 1/4 and colstep = 1/4096 everywhere but on the tight family (256, 1/16): there
kappa ~ 4100 and the guard band below, 64 tol_y = 0.125 |gamma|, is wider than half a lattice gap of 1/4 (0.1246 |gamma|, pooled
0.0935 |gamma|), and a column step of 2^-16 in x is below the fp32 spacing 2^-15 at 256, so columns would collide.  That family alone
uses q = 1/2 and colstep = 1/2048; the guard band and the uniqueness of the maxima are asserted for it as for every other.
beta is chosen AFTER the data: beta = -gamma * (the midpoint of the widest gap between neighbouring distinct float64 xhat values
near a random quantile in 30..70 %), so that no pre-activation is within rounding of the ReLU threshold.  The builder asserts, in float64 from the
fp32 tensors it returns, |z| >= 64 tol_y[c] for every element of every non-constant channel and, pooled, that the maximum of every
row with a positive maximum is unique (a constant row is all ties: its gradient goes to column 0, the first arg max).  No element
is ever left out of a comparison; these assertions are what makes that safe.
The first row n = 0 of every (b, c) is pushed to the dead side of the threshold (pooled op: a row whose maximum is not positive).

Tolerances (`tolerances`), per channel and a priori -- none is read off a kernel:

    kappa_c = (|mean_c| + max |x - mean_c|) / sqrt(var_c + eps),   f_c = max(1, kappa_c / 8)

kappa_c is how far the data sits from zero in its own standard deviations: fp32 storage of x and mean costs 2^-24 kappa_c in xhat
whatever a kernel does (torch's fp32 BatchNorm has the same floor).  The tolerances of tests/test_train_gpu.py keep their form, per
channel and times f_c (f_c = 1 on the centred families: exactly those tolerances):

    y, dx           2e-6 f_c max |reference| over the channel
    dgamma, dbeta   1e-5 f_c max |reference| over the channels
    running_mean    max(1e-6, 2^-23 |reference|)        (an fp32 buffer cannot hold 1000 to 1e-6; nor can it hold any value closer
                    than half an ulp, up to 2^-24 |reference|, which alone is up to half of this tolerance: "a quarter" below is
                    asked of what a kernel adds to that one rounding of the stored result, `running_mean_store`)
    running_var     1e-6 f_c |reference|
    guard band      tol_y[c] = 8 * 2^-24 (|gamma_c| kappa_c + |beta_c|)
    constant channels (exact data: no excuse)   y = relu(beta) to 2^-20 (|beta| + |gamma|),  saved mean = the constant bit for bit,
                    dx to 2e-6 |gamma| / sqrt(eps) max |dy|

fp32 models (`model`): (a) "exact": statistics exact in double, rounded to fp32 mean and rstd, everything else as the kernels do
it in fp32 -- the pre-activation fma(x - mean, gamma rstd, beta), the 64-sequential-adds-per-lane-then-tree sums of the backward --
which is what a correct kernel can achieve; (b) "sumsq": fp32 sum x / sum x^2 per 16384-chunk, combined in double, var = E[x^2] - E[x]^2,
pre-activation fma(x, a, beta - mean a): the kernels before the statistics were centred.  The CPU test asserts (a) under a quarter
of every tolerance and (b) above the y tolerance on the constant 1000.0 channel and where |offset| / sigma >= 256 in every case,
where 16 <= |offset| / sigma < 256 in some (the error there is a few roundings of sum x^2, about the tolerance's own size: luck)."""
import functools
import math
from types import SimpleNamespace

import torch

F64 = torch.float64
F32 = torch.float32
CHUNK = 16384  # elements of a (b, c) slab per workgroup

# (offset, sigma, lattice step q, column step); sigma None = a constant channel
FAMILIES = (
    (0.0, 1.0, 0.25, 1 / 4096), (0.4, 1.7, 0.25, 1 / 4096),                                 # centred controls
    (16.0, 1.0, 0.25, 1 / 4096), (64.0, 1.0, 0.25, 1 / 4096), (-300.0, 3.0, 0.25, 1 / 4096), (1000.0, 1.0, 0.25, 1 / 4096),
    (256.0, 1 / 16, 0.5, 1 / 2048),                                                          # tight
    (0.0, 1e-3, 0.25, 1 / 4096),                                                             # eps dominates the variance
    (5.0, None, None, None), (1000.0, None, None, None),                                     # constant
    (-64.0, 1.0, 0.25, 1 / 4096), (1000.0, 0.5, 0.25, 1 / 4096),
)
CONST_5, CONST_1000 = 8, 9

# (shape, seed) of test_bn_train_gpu.py; test_bn_train_ref_cpu.py builds and models every one of them
CASES_BN = (((2, 12, 257, 64), 11), ((3, 12, 512, 64), 12), ((1, 12, 7, 4), 13))
CASES_POOL = (((2, 12, 257, 64), 21), ((2, 12, 40, 32), 22), ((2, 12, 129, 128), 23), ((1, 12, 65, 256), 24), ((2, 24, 2800, 64), 25))
STATE_SHAPE = (2, 12, 33, 64)  # the module-state cases (momentum=None, no running statistics, eps / momentum, a second call)
STATE_SEEDS = {False: (31, 33, 35), True: (32, 34, 36)}  # pooled? -> (first data, the second call's fresh data, the eps = 1e-3 data)


def all_cases():
    """(shape, seed, pool, eps) of every tensor test_bn_train_gpu.py builds."""
    out = [(s, seed, False, 1e-5) for s, seed in CASES_BN] + [(s, seed, True, 1e-5) for s, seed in CASES_POOL]
    for pool, seeds in STATE_SEEDS.items():
        out += [(STATE_SHAPE, seed, pool, eps) for seed, eps in zip(seeds, (1e-5, 1e-5, 1e-3))]
    return out


def family(c):
    return FAMILIES[c % 12]


def off_centre(c):
    """|offset| / sigma >= 16: where E[x^2] - E[x]^2 is outside what fp32 allows."""
    off, sig = family(c)[:2]
    return sig is not None and abs(off) / sig >= 16


def is_const(c):
    return family(c)[1] is None


# ------------------------------------------------------------------------------------------------------------ reference
def _first_max(y):
    """max over the last axis and the FIRST index that attains it (the documented tie rule: a constant row pools to column 0)."""
    m = y.amax(3)
    cols = torch.arange(y.shape[3]).expand_as(y)
    return m, torch.where(y == m[..., None], cols, y.shape[3]).amin(3)


def reference(x, gamma, beta, dy, eps=1e-5, momentum=0.1, running_mean=None, running_var=None, pool=False):
    """x (B,C,N,S), dy like x (pooled: (B,C,N)) -> float64 y / out, idx, z, dx, dgamma, dbeta, mean, var, running statistics."""
    x, dy = x.to(F64), dy.to(F64)
    gm, bt = gamma.to(F64)[None, :, None, None], beta.to(F64)[None, :, None, None]
    M = x.numel() // x.shape[1]
    mean = x.sum((0, 2, 3)) / M
    d = x - mean[None, :, None, None]
    var = (d * d).sum((0, 2, 3)) / M
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = d * rstd[None, :, None, None]
    z = gm * xhat + bt
    r = SimpleNamespace(mean=mean, var=var, rstd=rstd, z=z, M=M, idx=None)
    if pool:
        r.y, r.idx = _first_max(torch.relu(z))
        dy = torch.zeros_like(z).scatter_(3, r.idx[..., None], dy[..., None])
    else:
        r.y = torch.relu(z)
    dz = dy * (z > 0)
    r.dbeta = dz.sum((0, 2, 3))
    r.dgamma = (dz * xhat).sum((0, 2, 3))
    r.dx = gm * rstd[None, :, None, None] * (dz - r.dbeta[None, :, None, None] / M - xhat * r.dgamma[None, :, None, None] / M)
    r.running_mean = r.running_var = None
    if running_mean is not None:
        r.running_mean = (1 - momentum) * running_mean.to(F64) + momentum * mean
        r.running_var = (1 - momentum) * running_var.to(F64) + momentum * var * (M / (M - 1) if M > 1 else 1.0)
    return r


# ------------------------------------------------------------------------------------------------------------ data
def _kappa(x64, mean, var, eps):
    return (mean.abs() + (x64 - mean[None, :, None, None]).abs().amax((0, 2, 3))) / torch.sqrt(var + eps)


def guard_tol(gamma, beta, kappa):
    return 8 * 2.0 ** -24 * (gamma.to(F64).abs() * kappa + beta.to(F64).abs())


def _threshold(xh, g):
    """The midpoint of the widest gap between neighbouring distinct values of xh whose lower end lies between the 30 % and 70 %
    quantiles; among gaps of (nearly) that width, the one nearest to a random quantile in that range."""
    v = torch.sort(xh.reshape(-1))[0]
    vals, counts = torch.unique_consecutive(v, return_counts=True)
    assert len(vals) >= 2
    cdf = counts.cumsum(0).to(F64) / v.numel()         # share of the elements <= vals[i]
    gaps = vals[1:] - vals[:-1]
    ok = (cdf[:-1] >= 0.3) & (cdf[:-1] <= 0.7)
    if not bool(ok.any()):
        ok = torch.ones_like(ok)
    wide = ok & (gaps >= 0.75 * gaps[ok].max())
    q = 0.3 + 0.4 * float(torch.rand((), generator=g))
    i = int(torch.where(wide, (cdf[:-1] - q).abs(), torch.full_like(gaps, 9.0)).argmin())
    return 0.5 * float(vals[i] + vals[i + 1])


def make_case(shape, seed, pool=False, eps=1e-5):
    """fp32 x (B,C,N,S), gamma, beta, dy, initial running statistics; every third channel has a negative gamma."""
    B, C, N, S = shape
    g = torch.Generator().manual_seed(seed)
    gamma = ((0.5 + torch.rand(C, generator=g)) * torch.where((torch.arange(C) + torch.arange(C) // 12) % 3 == 0, -1.0, 1.0)).to(F32)
    x = torch.empty(shape, dtype=F32)
    for c in range(C):
        off, sig, q, colstep = family(c)
        if sig is None:
            x[:, c] = off
            continue
        u = (torch.round(torch.randn(B, N, S, generator=g, dtype=F64) / q) * q).clamp(-6, 6)
        # row n = 0: every value on the side of the threshold where the ReLU is dead (the threshold lies within |u| < 1)
        u[:, 0] = -math.copysign(1.0, float(gamma[c])) * (1 + u[:, 0].abs()).clamp(max=6)
        if pool:
            u = u + torch.arange(S, dtype=F64) * colstep
        x[:, c] = (off + sig * u).to(F32)
    x64 = x.to(F64)
    M = B * N * S
    mean = x64.sum((0, 2, 3)) / M
    var = ((x64 - mean[None, :, None, None]) ** 2).sum((0, 2, 3)) / M
    xhat = (x64 - mean[None, :, None, None]) / torch.sqrt(var + eps)[None, :, None, None]
    beta = torch.empty(C, dtype=F32)
    for c in range(C):
        if is_const(c):  # both signs, |beta| >= 0.1: the 1000.0 channel is alive, the 5.0 channel dead
            beta[c] = (0.1 + 0.4 * float(torch.rand((), generator=g))) * (1.0 if c % 12 == CONST_1000 else -1.0)
        else:
            beta[c] = -float(gamma[c]) * _threshold(xhat[:, c], g)
    dy = torch.randn((B, C, N) if pool else shape, generator=g)
    case = SimpleNamespace(shape=shape, pool=pool, eps=eps, x=x, gamma=gamma, beta=beta, dy=dy,
                           running_mean=torch.randn(C, generator=g), running_var=torch.rand(C, generator=g) + 0.5)
    # ---- what makes it safe to compare every element
    z = gamma.to(F64)[None, :, None, None] * xhat + beta.to(F64)[None, :, None, None]
    tol = guard_tol(gamma, beta, _kappa(x64, mean, var, eps))
    live = torch.tensor([not is_const(c) for c in range(C)])
    margin = z.abs().amin((0, 2, 3)) / tol
    assert bool((margin[live] >= 64).all()), ("a pre-activation within the guard band of the ReLU threshold", margin)
    assert bool(((z[:, live] > 0).sum((0, 2, 3)) > 0).all()) and bool(((z[:, live] < 0).sum((0, 2, 3)) > 0).all())
    if pool:
        top = z.topk(2, dim=3)[0]
        assert bool(((top[..., 0] <= 0) | (top[..., 0] > top[..., 1]))[:, live].all()), "a positive row maximum is not unique"
        assert bool(((top[..., 0] <= 0).sum((0, 2))[live] > 0).all()), "no row without a positive value"
    return case


@functools.lru_cache(maxsize=None)
def case_and_reference(shape, seed, pool, eps=1e-5):
    """(case, reference with momentum 0.1, tolerances), computed once and shared: never change them."""
    c = make_case(shape, seed, pool, eps)
    r = reference(c.x, c.gamma, c.beta, c.dy, c.eps, 0.1, c.running_mean, c.running_var, pool)
    return c, r, tolerances(c, r)


# ------------------------------------------------------------------------------------------------------------ tolerances
def _chmax(t):
    return t.abs().amax([d for d in range(t.dim()) if d != 1])


def tolerances(case, ref):
    """Per-channel (C,) float64 tolerances of every compared quantity, from the reference and the inputs alone."""
    kappa = _kappa(case.x.to(F64), ref.mean, ref.var, case.eps)
    f = (kappa / 8).clamp_min(1.0)
    t = SimpleNamespace(kappa=kappa, f=f)
    t.y = 2e-6 * f * _chmax(ref.y)
    t.dx = 2e-6 * f * _chmax(ref.dx)
    t.dgamma = 1e-5 * f * ref.dgamma.abs().max()
    t.dbeta = 1e-5 * f * ref.dbeta.abs().max()
    if ref.running_mean is not None:
        t.running_mean = (2.0 ** -23 * ref.running_mean.abs()).clamp_min(1e-6)
        t.running_mean_store = 2.0 ** -24 * ref.running_mean.abs()
        t.running_var = 1e-6 * f * ref.running_var.abs()
    const = torch.tensor([is_const(c) for c in range(case.x.shape[1])])
    gm, bt = case.gamma.to(F64).abs(), case.beta.to(F64).abs()
    t.y = torch.where(const, torch.minimum(t.y, 2.0 ** -20 * (bt + gm)), t.y)
    t.dx = torch.where(const, torch.minimum(t.dx, 2e-6 * gm / math.sqrt(case.eps) * case.dy.abs().max().to(F64)), t.dx)
    t.y_guard = guard_tol(case.gamma, case.beta, kappa)
    return t


def ratios(got, ref, tol):
    """{quantity: (C,) error / tolerance} for everything `got` carries (y, dx, dgamma, dbeta, running_mean, running_var: tensors of
    any float type on any device); a ratio of 0 / 0 (a dead constant channel) counts as 0."""
    out = {}
    for k in ("y", "dx", "dgamma", "dbeta", "running_mean", "running_var"):
        v = getattr(got, k, None)
        if v is None:
            continue
        e = (v.detach().cpu().to(F64) - getattr(ref, k)).abs()
        e = _chmax(e) if e.dim() > 1 else e
        t = getattr(tol, k)
        out[k] = torch.where(e == 0, torch.zeros_like(e), e / t)
    return out


# ------------------------------------------------------------------------------------------------------------ fp32 models
def _tree(acc):
    """(..., 256) lane sums -> (...,): halving tree inside each wave of 64, then the four waves in order."""
    w = acc.reshape(*acc.shape[:-1], 4, 64)
    for h in (32, 16, 8, 4, 2, 1):
        w = w[..., :h] + w[..., h:2 * h]
    w = w[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def _chunk_sums(t, pairs=False):
    """t (B,C,L) fp32 -> (B,C,nchunk) fp32 as a workgroup of 256 lanes sums a chunk: lane l adds elements 1024 i + 4 l + j one
    after the other (pairs: (e0 + e1) + (e2 + e3) first, as the forward statistics pass did), then `_tree`.  Zero padding adds 0."""
    B, C, L = t.shape
    n = -(-L // CHUNK)
    t = torch.nn.functional.pad(t, (0, n * CHUNK - L)).reshape(B, C, n, 16, 256, 4)
    acc = torch.zeros(B, C, n, 256, dtype=F32)
    for i in range(16):
        if pairs:
            acc = acc + ((t[..., i, :, 0] + t[..., i, :, 1]) + (t[..., i, :, 2] + t[..., i, :, 3]))
        else:
            for j in range(4):
                acc = acc + t[..., i, :, j]
    return _tree(acc)


def _row_sums(t):
    """t (B,C,N) fp32 -> (B,C): the pooled backward's sums, lane l adding rows l, l + 256, ... in order."""
    B, C, N = t.shape
    k = -(-N // 256)
    t = torch.nn.functional.pad(t, (0, k * 256 - N)).reshape(B, C, k, 256)
    acc = torch.zeros(B, C, 256, dtype=F32)
    for i in range(k):
        acc = acc + t[:, :, i]
    return _tree(acc)


def _fma(a, b, c):
    """fp32 fma(a, b, c): the product of two fp32 values is exact in double."""
    return (a.to(F64) * b.to(F64) + c.to(F64)).to(F32)


def model(case, stats="exact", momentum=0.1):
    """The kernels' arithmetic in fp32 on the CPU -> y, idx, dx, dgamma, dbeta, mean, running statistics (fp32).
    stats = "exact": model (a) of the module docstring; "sumsq": model (b)."""
    x, B, C = case.x, case.x.shape[0], case.x.shape[1]
    M = x.numel() // C
    bc = lambda t: t[None, :, None, None]  # noqa: E731
    eps = float(torch.tensor(case.eps, dtype=F32))
    if stats == "exact":
        x64 = x.to(F64)
        mean = x64.sum((0, 2, 3)) / M
        var = ((x64 - bc(mean)) ** 2).sum((0, 2, 3)) / M
    else:
        xl = x.reshape(B, C, -1)
        mean = _chunk_sums(xl, pairs=True).to(F64).sum((0, 2)) / M
        var = (_chunk_sums(xl * xl, pairs=True).to(F64).sum((0, 2)) / M - mean * mean).clamp_min(0.0)
    o = SimpleNamespace(mean=mean.to(F32), idx=None)
    rstd = (1.0 / torch.sqrt(var + eps)).to(F32)
    mom = float(torch.tensor(momentum, dtype=F32))
    o.running_mean = ((1 - mom) * case.running_mean.to(F64) + mom * mean).to(F32)
    o.running_var = ((1 - mom) * case.running_var.to(F64) + mom * var * (M / (M - 1) if M > 1 else 1.0)).to(F32)
    m, r, a, bt = bc(o.mean), bc(rstd), bc(case.gamma * rstd), bc(case.beta)
    z = _fma(x - m, a, bt) if stats == "exact" else _fma(x, a, bt - m * a)
    y = z.clamp_min(0.0)
    xh = (x - m) * r
    if case.pool:
        o.y, o.idx = _first_max(y)
        xw, zw = x.gather(3, o.idx[..., None])[..., 0], z.gather(3, o.idx[..., None])[..., 0]
        dzw = torch.where(zw > 0, case.dy, torch.zeros_like(case.dy))
        xhw = (xw - m[..., 0]) * r[..., 0]
        o.dbeta = _row_sums(dzw).to(F64).sum(0).to(F32)
        o.dgamma = _row_sums(dzw * xhw).to(F64).sum(0).to(F32)
        dz = torch.zeros_like(x).scatter_(3, o.idx[..., None], dzw[..., None])
    else:
        o.y = y
        dz = torch.where(z > 0, case.dy, torch.zeros_like(case.dy))
        o.dbeta = _chunk_sums(dz.reshape(B, C, -1)).to(F64).sum((0, 2)).to(F32)
        o.dgamma = _chunk_sums((dz * xh).reshape(B, C, -1)).to(F64).sum((0, 2)).to(F32)
    inv = torch.tensor(1.0 / M, dtype=F32)
    o.dx = a * (dz - bc(o.dbeta * inv) - xh * bc(o.dgamma * inv))
    return o
