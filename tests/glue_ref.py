"""float64 references, derived bounds and the cases of the one-pass fp32 kernels between the GEMMs: csrc/glue.hip, the three routes of
csrc/bmm_f32.hip and the two row kernels of csrc/fused.hip (add_layernorm, bilinear_sample).  Plain torch on the CPU.

Every kernel K below is a small namespace with the same members:
    K.CASES            the cases (tuples) that tests/test_glue_kernels_gpu.py runs on the device
    K.inputs(case)     the CPU tensors of a case, from a generator seeded by the case (memoised; never changed afterwards)
    K.check(inp, got)  (ok, ratio): every element of `got` within its `bound_*` of the `*_64` result (both memoised in `inp`), and the
                       worst error / bound; a bf16 output judged by `rne_ok` enters the ratio as 0 (inside) or inf
    K.emulate(inp, mutant=None)  a float32 restatement of the kernel's own arithmetic on the CPU, or one of K.MUTANTS: what the kernel
                       would compute with a dropped element, a skipped tail loop, a wrong comparison ...
tests/test_glue_ref_cpu.py shows that the restatement meets every bound and that every mutant leaves it on some case.

The bounds are derived, not tuned.  U = 2^-24 is the unit roundoff of fp32 (half an ulp, relative):
  * an fp32 sum of n terms over `chains` accumulators and a fixed combination tree: (ceil(n / chains) + tree depth) U sum|x|
  * a k-ordered fma chain of length K: K U sum|a b|
  * a bf16 output adds 2^-9 |ref| -- or, where the fp32 value is itself bounded, the output must be the RNE rounding of SOME fp32 value
    within that bound (`rne_ok`)
  * a division or a sqrtf adds one ulp (2 U |result|)
Where the inputs make fp32 arithmetic exact (integer-valued operands in [-8, 8] with at most 512 terms; points on the 2^-6 lattice in
[-1, 1]) the bound is 0 and the comparison is torch.equal with the float64 result."""
import math
import os
import sys
import types
import zlib

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

U = 2.0 ** -24
FLT_MAX = float(np.finfo(np.float32).max)
_MEMO = {}


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _memo(name, case, make):
    key = (name, case)
    if key not in _MEMO:
        if len(_MEMO) > 64:
            _MEMO.clear()
        _MEMO[key] = make()
    return _MEMO[key]


def _once(inp, key, make):
    if key not in inp:
        inp[key] = make()
    return inp[key]


def f32(x):
    """Python float -> the fp32 value a C `float` argument carries, as a Python float."""
    return float(np.float32(x))


def bf16_rne(x):
    return x.float().bfloat16().float()


def bf16_trunc(x):
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32)


def compare(got, ref, bound):
    """(ok, ratio) of |got - ref| <= bound elementwise (ref float64; bound a float64 tensor or 0).  A NaN in `got` -- an element the kernel
    never wrote -- fails.  ratio: the worst error / bound over the elements with a positive bound; where the bound is 0 equality is required."""
    got = got.double()
    ref = ref.double()
    if got.shape != ref.shape:
        return False, math.inf
    bound = torch.as_tensor(bound, dtype=torch.float64).expand(ref.shape)
    err = torch.where(got == ref, torch.zeros_like(ref), (got - ref).abs())   # (equal infinities are equal)
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    ok = bool((err <= bound).all())
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
    if not bool((err[~pos] == 0).all()):
        ratio = math.inf
    return ok, ratio


def rne_ok(got, ref, bound32):
    """A bf16 output (given as float values) of an fp32 value v with |v - ref| <= bound32: RNE is monotone, so RNE(v) lies between
    lo = RNE(ref - bound32) and hi = RNE(ref + bound32).  Where lo == hi that value is required; where they differ (the float64 value lies
    within the fp32 bound of a rounding boundary) either neighbour is accepted.  Returns (ok, share of elements with lo != hi)."""
    ref = ref.double()
    bound32 = torch.as_tensor(bound32, dtype=torch.float64).expand(ref.shape)
    lo, hi = bf16_rne(ref - bound32).double(), bf16_rne(ref + bound32).double()
    g = got.double()
    ok = bool(((g >= lo) & (g <= hi)).all())
    return ok, float((lo != hi).double().mean())


def _tree32(x):
    """Pairwise fp32 sum over the last dimension (a power of two): the shape of the wave / workgroup combination trees."""
    x = x.float()
    while x.shape[-1] > 1:
        x = x[..., 0::2] + x[..., 1::2]
    return x[..., 0]


def _strided32(x, lanes):
    """Sum over the last dimension the way `for (i = t; i < n; i += lanes)` does it in `lanes` threads, then a pairwise tree: fp32."""
    n = x.shape[-1]
    L = (n + lanes - 1) // lanes
    p = torch.zeros(*x.shape[:-1], L * lanes, dtype=torch.float32)
    p[..., :n] = x
    p = p.reshape(*x.shape[:-1], L, lanes)
    acc = torch.zeros(*x.shape[:-1], lanes, dtype=torch.float32)
    for i in range(L):
        acc = acc + p[..., i, :]
    return _tree32(acc)


def _fma32(a, b, c):
    """fp32 fma: a b is exact in float64 (48 bits), the sum is rounded to float64 and then to fp32 (a double rounding differs from the
    single one only on a 2^-29 sliver around an fp32 tie: far inside every bound here)."""
    return (a.double() * b.double() + c.double()).float()


def _sqrt32(x):
    """Correctly rounded fp32 square root, like sqrtf (torch's vectorised fp32 sqrt on the CPU is an ulp off on ~1% of its arguments; a
    float64 root rounds to fp32 like the exact one: 53 >= 2 * 24 + 2)."""
    return torch.sqrt(x.double()).float()


def _ns(**kw):
    return types.SimpleNamespace(**kw)


# ============================================================================================================================ bmm_f32
BMM_K = (1, 2, 3, 7, 8, 9, 12, 13, 64, 257)
BMM_NM32 = ((1, 1), (31, 33), (32, 32), (33, 65), (197, 197))
BMM_NM64 = ((256, 256), (257, 300), (321, 449))
BMM_K64 = (13, 20)
BMM_BATCH = ((1, 1), (3, 4))
BMM_ALPHA = (1.0, 10.0)
BMM_CASES = [(n, m, K, bo, bi, al, kind) for (n, m) in BMM_NM32 for K in BMM_K for (bo, bi) in BMM_BATCH for al in BMM_ALPHA for kind in ("int", "rand")]
BMM_CASES += [(n, m, K, bo, bi, al, kind) for (n, m) in BMM_NM64 for K in BMM_K64 for (bo, bi) in BMM_BATCH for al in BMM_ALPHA for kind in ("int", "rand")]


def bmm_inputs(case):
    n, m, K, bo, bi, _, kind = case

    def make():
        g = _gen("bmm", n, m, K, bo, bi, kind)
        if kind == "int":
            A = torch.randint(-8, 9, (bo, bi, n, K), generator=g).float()
            B = torch.randint(-8, 9, (bo, bi, m, K), generator=g).float()
        else:
            A = torch.randn(bo, bi, n, K, generator=g)
            B = torch.randn(bo, bi, m, K, generator=g)
        return {"A": A, "B": B}

    d = dict(_memo("bmm", (n, m, K, bo, bi, kind), make))   # (the data and what is derived from it are shared by both alphas)
    d["_shared"] = _memo("bmm_shared", (n, m, K, bo, bi, kind), dict)
    d["alpha"], d["kind"], d["K"] = case[5], kind, K
    return d


def bmm_64(A, B, alpha):
    """C[bo, bi, i, j] = alpha sum_k A[bo, bi, i, k] B[bo, bi, j, k]"""
    return torch.einsum("abik,abjk->abij", A.double(), B.double()) * float(alpha)


def bound_bmm(inp):
    """v_mfma_f32_32x32x2_f32 accumulates a k-ordered fma chain: K roundings, each at most U times the running sum, which never exceeds
    sum_k |a b|: K U sum|a b|.  The epilogue's `acc * alpha` rounds once more (exact for alpha = 1): + U |ref|.  Integer-valued operands in
    [-8, 8] with K <= 512: every partial sum is an integer below 2^15 and 10 times it below 2^19 -- exact, bound 0."""
    if inp["kind"] == "int":
        return 0.0
    s = _once(inp["_shared"], "abs", lambda: torch.einsum("abik,abjk->abij", inp["A"].double().abs(), inp["B"].double().abs()))
    al = abs(inp["alpha"])
    return inp["K"] * U * s * al + (U * bmm_ref(inp).abs() if al != 1.0 else 0.0)


def bmm_ref(inp):
    r1 = _once(inp["_shared"], "ref1", lambda: bmm_64(inp["A"], inp["B"], 1.0))
    return r1 * float(inp["alpha"])


def bmm_emulate(inp, mutant=None):
    A, B, K = inp["A"], inp["B"], inp["K"]

    def chain():
        acc = torch.zeros(*A.shape[:3], B.shape[2], dtype=torch.float32)
        Ke = K - K % 8 if mutant == "skip_tail" else (K - 1 if mutant == "drop_last" else K)
        a = lambda k: A[..., :, k, None] if k < Ke else torch.zeros_like(A[..., :, 0, None])  # noqa: E731
        b = lambda k: B[..., None, :, k] if k < Ke else torch.zeros_like(B[..., None, :, 0])  # noqa: E731
        for k in range(0, Ke, 2):   # one MFMA step: the pair (k, k + 1), a zero for the k past the end
            if mutant == "swap_pair":
                acc = _fma32(a(k), b(k + 1), acc)
                acc = _fma32(a(k + 1), b(k), acc)
            else:
                acc = _fma32(a(k), b(k), acc)
                acc = _fma32(a(k + 1), b(k + 1), acc)
        if mutant == "twice":
            acc = _fma32(A[..., :, K - 1, None], B[..., None, :, K - 1], acc)
        return acc

    acc = _once(inp["_shared"], ("emu", mutant), chain)
    return acc * torch.tensor(inp["alpha"], dtype=torch.float32)


def bmm_check(inp, got):
    return compare(got, bmm_ref(inp), bound_bmm(inp))


bmm = _ns(CASES=BMM_CASES, inputs=bmm_inputs, check=bmm_check, emulate=bmm_emulate, MUTANTS=("drop_last", "twice", "skip_tail", "swap_pair"))

# ============================================================================================================== cloud_radius, scale_by_radius
N_LIST = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 5000)
RADIUS_KINDS = ("centred", "off10", "off1000", "outlier0", "outlier_last", "outlier256")
RADIUS_CASES = [(N,) for N in N_LIST]


def radius_inputs(case):
    """One cloud per kind (the batch): extent 1 around the origin, around a centre 10 and 1000 extents away, and with one point 50 extents
    out at index 0, N - 1 and 256 (index min(256, N - 1): a short cloud has it at the end)."""
    (N,) = case

    def make():
        g = _gen("radius", N)
        pts = torch.rand(len(RADIUS_KINDS), N, 3, generator=g) * 2 - 1
        pts[1] += torch.tensor([10.0, -7.0, 3.0])
        pts[2] += torch.tensor([1000.0, 300.0, -700.0])
        pts[3, 0] = torch.tensor([50.0, 1.0, -2.0])
        pts[4, N - 1] = torch.tensor([-1.0, 50.0, 2.0])
        pts[5, min(256, N - 1)] = torch.tensor([3.0, -2.0, -50.0])
        return {"pts": pts.contiguous()}

    return dict(_memo("radius", case, make))


def cloud_radius_64(pts):
    """radius[b] = max_i |p_i - mean(p)|"""
    p = pts.double()
    return (p - p.mean(1, keepdim=True)).norm(dim=2).max(1)[0]


def bound_cloud_radius(inp):
    """The mean is summed in float64 and rounded once: each component is off by at most U |mean_c|, which moves every distance by at most
    U |mean|.  d = p - mean rounds once per component (U |d_c|: at most U r in the norm); (dx^2 + dy^2) + dz^2 is three products and two
    additions of positive terms (at most 3 U relative on d^2, 1.5 U on d, rounded up to 2 U); sqrtf adds one ulp (2 U).  A maximum carries
    the largest error of its arguments: U (|mean| + 5 r) with r the radius itself."""
    p = inp["pts"].double()
    return U * (p.mean(1).norm(dim=1) + 5 * cloud_radius_64(inp["pts"]))


def cloud_radius_emulate(inp, mutant=None):
    P = inp["pts"]
    N = P.shape[1]
    keep = N - N % 256 if mutant == "skip_tail" else (N - 1 if mutant == "drop_last" else N)
    if keep == 0:
        return torch.zeros(P.shape[0])
    Q = P[:, :keep]
    s = Q.double().sum(1)
    if mutant == "twice":
        s = s + P[:, N - 1].double()
    mean = (s / N).float()
    d = Q - mean[:, None]
    return _sqrt32((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).max(1)[0]


def radius_check(inp, got):
    return compare(got, _once(inp, "_ref", lambda: cloud_radius_64(inp["pts"])), _once(inp, "_bound", lambda: bound_cloud_radius(inp)))


cloud_radius = _ns(CASES=RADIUS_CASES, inputs=radius_inputs, check=radius_check,
                   emulate=cloud_radius_emulate, MUTANTS=("drop_last", "twice", "skip_tail"))

SCALE_CASES = [(n, mode) for n in (1, 3, 255, 257, 6144) for mode in (0, 1)]
SCALE_EPS = 1e-6


def scale_inputs(case):
    n, mode = case
    g = _gen("scale", n)
    return {"x": torch.randn(3, n, generator=g), "radius": torch.tensor([0.37, 1.0, 123.456]), "eps": f32(SCALE_EPS), "mode": mode}


def scale_by_radius_64(x, radius, eps, mode):
    """x / (radius[b] + eps) (mode 0) or x * (radius[b] + eps) (mode 1) with s = radius + eps rounded to fp32 as the kernel forms it; the
    result rounded once to fp32: the correctly rounded fp32 quotient / product (a float64 quotient of two fp32 values rounds to fp32 like the
    exact one: 53 >= 2 * 24 + 2)."""
    s = (radius.double() + eps).float().double()[:, None]
    return (x.double() * s if mode else x.double() / s).float().double()


def bound_scale_by_radius(inp):
    """One correctly rounded operation per element (the library is built with correctly rounded fp32 division): bound 0 against the
    correctly rounded result."""
    return 0.0


def scale_emulate(inp, mutant=None):
    s = (inp["radius"] + torch.tensor(inp["eps"]))[:, None]
    out = inp["x"] * s if inp["mode"] else inp["x"] / s
    if mutant == "drop_last":
        out[:, -1] = float("nan")
    if mutant == "eps_missing":
        out = inp["x"] * inp["radius"][:, None] if inp["mode"] else inp["x"] / inp["radius"][:, None]
    return out


def scale_check(inp, got):
    return compare(got, scale_by_radius_64(inp["x"], inp["radius"], inp["eps"], inp["mode"]), bound_scale_by_radius(inp))


scale_by_radius = _ns(CASES=SCALE_CASES, inputs=scale_inputs, check=scale_check, emulate=scale_emulate, MUTANTS=("drop_last", "eps_missing"))

# ============================================================================================================================ pose_score
POSE_THR = 0.25   # (an fp32 value: `dis == thr` is attained exactly)
POSE_CASES = [(N,) for N in N_LIST]


def pose_inputs(case):
    """Rows of one call: random non-negative weights with a tenth of the distances exactly at the threshold (twice, different draws); all
    weights zero; one non-zero weight (distance below the threshold) at index 0, N - 1, 255, 256, 257 where the row has them."""
    (N,) = case

    def make():
        g = _gen("pose", N)
        pos = sorted({0, N - 1} | {p for p in (255, 256, 257) if p < N})
        B = 3 + len(pos)
        dis = torch.rand(B, N, generator=g) * 0.5
        dis[torch.rand(B, N, generator=g) < 0.1] = POSE_THR
        w = torch.rand(B, N, generator=g)
        w[2:] = 0
        for r, p in enumerate(pos):
            w[3 + r, p] = 0.75
            dis[3 + r, p] = 0.1
        return {"dis": dis.contiguous(), "w": w.contiguous(), "thr": POSE_THR}

    return dict(_memo("pose", case, make))


def pose_score_64(dis, w, thr):
    """sum_i [dis_i < thr] w_i / (sum_i w_i + 1e-8) * mean_i w_i, the 1e-8 as the kernel's fp32 constant"""
    d, w = dis.double(), w.double()
    s1, s2 = (w * (d < thr)).sum(1), w.sum(1)
    return s1 / (s2 + f32(1e-8)) * (s2 / dis.shape[1])


def bound_pose_score(inp):
    """Weights are non-negative.  Each of the two sums runs over 256 accumulators (ceil(N / 256) terms each) and a tree of depth 8 (four
    DPP steps and two levels in the wave, two levels across the waves): relative error c = (ceil(N / 256) + 8) U.  In
    s1 / (s2 + 1e-8) * (s2 / N) the first sum enters once and the second twice (3 c), the addition and the product round once each (2 U),
    the two divisions add one ulp each (4 U): |ref| (3 c + 6 U).  All weights zero: 0 / 1e-8 * 0 = 0 exactly, and the bound is 0."""
    N = inp["dis"].shape[1]
    c = ((N + 255) // 256 + 8) * U
    return pose_score_64(inp["dis"], inp["w"], inp["thr"]).abs() * (3 * c + 6 * U)


def pose_emulate(inp, mutant=None):
    D, W = inp["dis"], inp["w"]
    N = D.shape[1]
    keep = N - N % 256 if mutant == "skip_tail" else (N - 1 if mutant == "drop_last" else N)
    thr = torch.tensor(inp["thr"], dtype=torch.float32)
    hit = (D <= thr) if mutant == "le_for_lt" else (D < thr)
    t1, t2 = torch.where(hit, W, torch.zeros(())), W.clone()
    if mutant == "twice":
        t1, t2 = torch.cat([t1, t1[:, -1:]], 1), torch.cat([t2, t2[:, -1:]], 1)
        keep = N + 1
    s1, s2 = _strided32(t1[:, :keep], 256), _strided32(t2[:, :keep], 256)
    return s1 / (s2 + torch.tensor(1e-8, dtype=torch.float32)) * (s2 / torch.tensor(float(N), dtype=torch.float32))


def pose_check(inp, got):
    return compare(got, _once(inp, "_ref", lambda: pose_score_64(inp["dis"], inp["w"], inp["thr"])), _once(inp, "_bound", lambda: bound_pose_score(inp)))


pose_score = _ns(CASES=POSE_CASES, inputs=pose_inputs, check=pose_check, emulate=pose_emulate, MUTANTS=("drop_last", "twice", "skip_tail", "le_for_lt"))

# ============================================================================================================================ token_sum_bf16
TOKEN_CASES = [(J, C, kind) for J in (1, 2, 3, 4, 5, 7, 196, 2049) for C in (1, 64, 256, 300) for kind in ("int", "rand")]


def token_inputs(case):
    J, C, kind = case

    def make():
        g = _gen("token", J, C, kind)
        x = torch.randint(-8, 9, (2, J, C), generator=g).float() if kind == "int" else bf16_rne(torch.randn(2, J, C, generator=g))
        return {"x": x, "kind": kind}   # (bf16 values held as fp32)

    return dict(_memo("token", case, make))


def token_sum_64(x):
    """out[b, c] = sum_j x[b, j, c]"""
    return x.double().sum(1)


def bound_token_sum(inp):
    """Four accumulators take the tokens j % 4 of the whole groups of four, the first one also the J % 4 left over: at most
    J // 4 + J % 4 terms in a chain, then (a0 + a1) + (a2 + a3), depth 2: (J // 4 + J % 4 + 2) U sum|x|.  Integer values in [-8, 8],
    J = 2049: every partial sum is an integer below 2^15: exact, bound 0."""
    if inp["kind"] == "int":
        return 0.0
    J = inp["x"].shape[1]
    return (J // 4 + J % 4 + 2) * U * inp["x"].double().abs().sum(1)


def token_emulate(inp, mutant=None):
    x = inp["x"]
    J = x.shape[1]
    a = [torch.zeros(x.shape[0], x.shape[2]) for _ in range(4)]
    for j in range(0, J - J % 4, 4):
        for q in range(4):
            a[q] = a[q] + x[:, j + q]
    tail = range(J - J % 4, J)
    if mutant == "skip_tail":
        tail = range(0)
    if mutant == "drop_last":
        tail = range(J - J % 4, J - 1)
        if J % 4 == 0:
            a[3] = a[3] - x[:, J - 1]   # (exact on the integer cases, which are the ones that tell)
    for j in tail:
        a[0] = a[0] + x[:, j]
    if mutant == "twice":
        a[0] = a[0] + x[:, J - 1]
    return (a[0] + a[1]) + (a[2] + a[3])


def token_check(inp, got):
    return compare(got, _once(inp, "_ref", lambda: token_sum_64(inp["x"])), _once(inp, "_bound", lambda: bound_token_sum(inp)))


token_sum = _ns(CASES=TOKEN_CASES, inputs=token_inputs, check=token_check, emulate=token_emulate, MUTANTS=("drop_last", "twice", "skip_tail"))

# ============================================================================================================== row_dot, normalize_rows
ROWS_LIST = (1, 3, 4, 5, 1023)
ROW_KINDS = ("unit", "zero", "tiny", "huge")   # row i of a case is of kind (i + shift) % 4: spread 1, all zero, scaled by 1e-20 and by 1e18
_ROW_SHIFTS = [(rows, s) for rows in ROWS_LIST for s in ((0, 1, 2, 3) if rows == 1 else (0,))]
ROWDOT_CASES = [(rows, s, xb, ob) for rows, s in _ROW_SHIFTS for xb in (0, 1) for ob in (0, 1)]
NORMALIZE_CASES = [(rows, s, xb, mode, temp) for rows, s in _ROW_SHIFTS for xb in (0, 1) for mode in (0, 1, 2) for temp in (0.1, 1.0)]
AMBIGUOUS_SHARE = 0.01


def _rows256(rows, shift, x_bf16, g):
    x = torch.rand(rows, 256, generator=g) * 2 - 1   # (uniform: 256 squares of the rows scaled by 1e18 stay below FLT_MAX)
    kind = (torch.arange(rows) + shift) % 4
    x[kind == 1] = 0
    x[kind == 2] *= 1e-20
    x[kind == 3] *= 1e18
    return bf16_rne(x) if x_bf16 else x


def rowdot_inputs(case):
    rows, shift, xb, ob = case

    def make():
        g = _gen("rowdot", rows, shift, xb)
        return {"x": _rows256(rows, shift, xb, g), "w": torch.randn(256, generator=g) * 0.1, "b": f32(0.3)}

    d = dict(_memo("rowdot", (rows, shift, xb), make))
    d["x_bf16"], d["out_bf16"] = xb, ob
    return d


def row_dot_64(x, w, b):
    """out[r] = sum_c x[r, c] w[c] + b"""
    return x.double() @ w.double() + b


def bound_row_dot(inp):
    """256 products, one rounding each (U sum|x w|); four of them per lane as (p0 + p1) + (p2 + p3) and the wave tree of depth 6: at most
    (2 + 6) U sum|x w|; the bias is added last (U |ref|): 9 U sum|x w| + U |ref|.  A bf16 output is the RNE rounding of that fp32 value."""
    s = inp["x"].double().abs() @ inp["w"].double().abs()
    return 9 * U * s + U * row_dot_64(inp["x"], inp["w"], inp["b"]).abs()


def rowdot_emulate(inp, mutant=None):
    p = inp["x"] * inp["w"]
    if mutant == "drop_last":
        p[:, -1] = 0
    if mutant == "twice":
        p[:, -1] = p[:, -1] * 2
    p = p.reshape(-1, 64, 4)
    s = _tree32((p[..., 0] + p[..., 1]) + (p[..., 2] + p[..., 3])) + torch.tensor(inp["b"], dtype=torch.float32)
    if inp["out_bf16"]:
        return bf16_trunc(s) if mutant == "trunc_bf16" else bf16_rne(s)
    return s


def _check_rounded(inp, got, ref, bound, rounded):
    if not rounded:
        return compare(got, ref, bound)
    ok, share = rne_ok(got, ref, bound)
    inp["_ambiguous"] = (share * ref.numel(), ref.numel())   # (the tests add these up over the kernel's cases: below 1% of all elements)
    # (ratio of a rounded output: the error beyond half a bf16 ulp of the accepted interval is not a number worth a table; 0 or inf)
    return ok, 0.0 if ok else math.inf


def rowdot_check(inp, got):
    ref = _once(inp, "_ref", lambda: row_dot_64(inp["x"], inp["w"], inp["b"]))
    return _check_rounded(inp, got, ref, _once(inp, "_bound", lambda: bound_row_dot(inp)), inp["out_bf16"])


row_dot = _ns(CASES=ROWDOT_CASES, inputs=rowdot_inputs, check=rowdot_check, emulate=rowdot_emulate, MUTANTS=("drop_last", "twice", "trunc_bf16"))


def normalize_inputs(case):
    rows, shift, xb, mode, temp = case
    d = dict(_memo("normalize", (rows, shift, xb), lambda: {"x": _rows256(rows, shift, xb, _gen("normalize", rows, shift, xb))}))
    d["mode"], d["temp"], d["x_bf16"] = mode, f32(temp), xb
    return d


def normalize_rows_64(x, temp):
    """x[r, :] / max(|x[r, :]|, 1e-12) / temp, the clamp as the kernel's fp32 constant"""
    x = x.double()
    return x / x.norm(dim=1, keepdim=True).clamp(min=f32(1e-12)) / temp


def bound_normalize_rows(inp):
    """The sum of 256 squares as in row_dot (no bias): 9 U relative, positive terms; a square below 2^-126 (the rows scaled by 1e-20) is
    rounded on the subnormal grid, half its spacing (2^-150) absolute each, which no relative bound covers: + 256 * 2^-150 / sum.  The square
    root halves both and adds one ulp (2 U); the two divisions add one ulp each (4 U): |ref| (10.5 U + 64 * 2^-149 / sum x^2).  A zero row
    gives exactly 0.
    Modes 0 and 1 store the RNE rounding of that fp32 value to bf16."""
    ss = (inp["x"].double() ** 2).sum(1, keepdim=True)
    sub = torch.where(ss > 0, 64 * 2.0 ** -149 / ss.clamp(min=1e-300), torch.zeros_like(ss))
    return normalize_rows_64(inp["x"], inp["temp"]).abs() * (10.5 * U + sub)


def normalize_emulate(inp, mutant=None):
    x = inp["x"]
    p = x * x
    if mutant == "drop_last":
        p[:, -1] = 0
    if mutant == "twice":
        p[:, -1] = p[:, -1] * 2
    p = p.reshape(-1, 64, 4)
    nrm = _sqrt32(_tree32((p[..., 0] + p[..., 1]) + (p[..., 2] + p[..., 3]))).clamp(min=1e-12)[:, None]
    y = x / nrm / torch.tensor(inp["temp"], dtype=torch.float32)
    if inp["mode"] == 2:
        return y
    return bf16_trunc(y) if mutant == "trunc_bf16" else bf16_rne(y)


def normalize_check(inp, got):
    ref = _once(inp, "_ref", lambda: normalize_rows_64(inp["x"], inp["temp"]))
    return _check_rounded(inp, got, ref, _once(inp, "_bound", lambda: bound_normalize_rows(inp)), inp["mode"] != 2)


normalize_rows = _ns(CASES=NORMALIZE_CASES, inputs=normalize_inputs, check=normalize_check, emulate=normalize_emulate,
                     MUTANTS=("drop_last", "twice", "trunc_bf16"))

# ============================================================================================================================ overlap_scores
OVERLAP_VALUES = (0.0, 1e-3, -1e-3, 20.0, -20.0, 100.0, -100.0)
OVERLAP_TOL = 2e-7   # (the sigmoid's tolerance of test_small_fp32_glue_kernels_vs_torch)
OVERLAP_CASES = [(n1, n2, xb, 0) for (n1, n2) in ((1, 1), (196, 150), (255, 2), (256, 257)) for xb in (0, 1)]
OVERLAP_CASES += [(n1, n1, xb, 1) for n1 in (1, 196, 255, 256) for xb in (0, 1)]   # (the two-halves form needs clouds of one size)


def overlap_inputs(case):
    """scores: the concatenated form (B, 1 + n1 + 1 + n2), or the two halves as one batch (2 B, 1 + n1) with cloud 2 of pair b at B + b."""
    n1, n2, xb, halves = case
    g = _gen("overlap", case)
    B = 3
    shape = (2 * B, n1 + 1) if halves else (B, n1 + n2 + 2)
    v = torch.tensor(OVERLAP_VALUES)[torch.randint(0, len(OVERLAP_VALUES), shape, generator=g)]
    return {"scores": bf16_rne(v) if xb else v, "n1": n1, "n2": n2, "halves": halves, "x_bf16": xb, "B": B}


def _overlap_pick(inp, s, shift=0):
    n1, B = inp["n1"], inp["B"]
    if inp["halves"]:
        return torch.cat([s[:B, 1 - shift:n1 + 1 - shift], s[B:, 1 - shift:n1 + 1 - shift]], 1)
    return torch.cat([s[:, 1 - shift:1 + n1 - shift], s[:, n1 + 2 - shift:s.shape[1] - shift]], 1)


def overlap_scores_64(inp):
    """sigmoid of the scores of the two clouds, their background tokens (position 0 of each) dropped, clamped to [0, 1]"""
    return torch.sigmoid(_overlap_pick(inp, inp["scores"].double())).clamp(0, 1)


def bound_overlap_scores(inp):
    """1 / (1 + expf(-x)): expf is good to a few ulp, the sum and the quotient round once each -- the 2e-7 absolute that
    test_small_fp32_glue_kernels_vs_torch already asks of it (a sigmoid is at most 1).  At +-100, expf gives a subnormal and infinity:
    the result is exactly 1 and 0, which the test requires on top of the bound."""
    return OVERLAP_TOL


def overlap_emulate(inp, mutant=None):
    x = _overlap_pick(inp, inp["scores"].float(), shift=1 if mutant == "shift" else 0)
    return (1.0 / (1.0 + torch.exp(-x))).clamp(0, 1)


def overlap_check(inp, got):
    ref = overlap_scores_64(inp)
    ok, ratio = compare(got, ref, bound_overlap_scores(inp))
    if ok:
        x = _overlap_pick(inp, inp["scores"].double())
        ok = bool((got[x == 100] == 1).all() and (got[x == -100] == 0).all() and (got >= 0).all() and (got <= 1).all())
    return ok, ratio


overlap_scores = _ns(CASES=OVERLAP_CASES, inputs=overlap_inputs, check=overlap_check, emulate=overlap_emulate, MUTANTS=("shift",))

# ============================================================================================================================ rigid_rows_bf16
RIGID_CASES = [(N, B) for N in (1, 255, 256, 257) for B in (1, 3)]


def rigid_inputs(case):
    N, B = case
    g = _gen("rigid", case)
    R = torch.linalg.qr(torch.randn(B, 3, 3, generator=g))[0].contiguous()
    return {"p": torch.randn(B, N, 3, generator=g), "t": torch.randn(B, 3, generator=g) * 0.3, "R": R}


def rigid_rows_64(p, t, R):
    """bf16((bf16(p - t)) @ bf16(R)) with every rounding explicit: the fp32 difference (its float64 value rounded once), RNE to bf16, the
    products of two bf16 values (exact in fp32 and in float64), (x0 r0 + x1 r1) + x2 r2 rounded to fp32 after each addition, RNE to bf16."""
    x = bf16_rne((p.double() - t.double()[:, None]).float()).double()
    Rb = bf16_rne(R).double()
    out = []
    for j in range(3):
        s = (x[..., 0] * Rb[:, None, 0, j] + x[..., 1] * Rb[:, None, 1, j]).float().double()
        out.append(bf16_rne((s + x[..., 2] * Rb[:, None, 2, j]).float()).double())
    return torch.stack(out, -1)


def bound_rigid_rows(inp):
    """Products of two bf16 values have 16 significant bits: exact in fp32, so a contraction into an fma cannot change a bit, and every
    other operation is a single correctly rounded one: bound 0 against the evaluation with explicit roundings."""
    return 0.0


def rigid_emulate(inp, mutant=None):
    rb = bf16_trunc if mutant == "trunc_bf16" else bf16_rne
    x = rb(inp["p"] - inp["t"][:, None])
    Rb = rb(inp["R"])
    out = torch.stack([rb((x[..., 0] * Rb[:, None, 0, j] + x[..., 1] * Rb[:, None, 1, j]) + x[..., 2] * Rb[:, None, 2, j]) for j in range(3)], -1)
    if mutant == "drop_last":
        out[:, -1] = float("nan")
    return out


def rigid_check(inp, got):
    return compare(got, rigid_rows_64(inp["p"], inp["t"], inp["R"]), bound_rigid_rows(inp))


rigid_rows = _ns(CASES=RIGID_CASES, inputs=rigid_inputs, check=rigid_check, emulate=rigid_emulate, MUTANTS=("trunc_bf16", "drop_last"))

# ============================================================================================================================ nearest_partner
NEAREST_THR = 0.25
NEAREST_CASES = [(n, m, over_b) for (n, m) in ((1, 1), (1, 700), (255, 257), (256, 256), (300, 513)) for over_b in (1, 0)]


def lattice(B, n, g):
    """Points whose coordinates are multiples of 2^-6 in [-1, 1]; every other one on the coarse multiples of 1/4, so that exact ties,
    coincident points and the distance 0.25 are common.  Squares, dot products and |a|^2 - 2 a.b + |b|^2 are exact in fp32."""
    fine = torch.randint(-64, 65, (B, n, 3), generator=g)
    coarse = torch.randint(-4, 5, (B, n, 3), generator=g) * 16
    pick = (torch.arange(n) % 2 == 0)[None, :, None]
    return (torch.where(pick, coarse, fine).float() / 64).contiguous()


def nearest_inputs(case):
    n, m, over_b = case

    def make():
        g = _gen("nearest", n, m)
        a, b = lattice(2, n, g), lattice(2, m, g)
        if m > 3 and n > 1:   # make sure the threshold itself and an exact tie are there whatever the draw
            b[:, 1] = a[:, 0] + torch.tensor([0.25, 0.0, 0.0]) * (1 if float(a[0, 0, 0]) < 0.5 else -1)
            b[:, 3] = b[:, 1]
        return {"a": a, "b": b}

    d = dict(_memo("nearest", (n, m), make))
    d["over_b"], d["thr"] = over_b, NEAREST_THR
    return d


def _nearest_dist64(a, b):
    a, b = a.double(), b.double()
    d2 = ((a * a).sum(-1)[:, :, None] - 2 * torch.einsum("bik,bjk->bij", a, b)) + (b * b).sum(-1)[:, None, :]
    return torch.sqrt(d2.clamp(min=0)).float().double()   # (sqrtf is correctly rounded; a float64 root rounds to fp32 like the exact one)


def nearest_partner_64(a, b, over_b, thr):
    """(dmin, arg, any_close) over the other cloud, for every point of a (over_b) or of b: the distance from the reference's expansion
    |a|^2 - 2 a.b + |b|^2 (exact on the lattice), the FIRST index that attains the minimum, whether any distance is <= thr."""
    d = _nearest_dist64(a, b)
    if not over_b:
        d = d.transpose(1, 2)
    dmin = d.min(2)[0]
    arg = (d == dmin[..., None]).int().argmax(2)   # (argmax returns the first of equal maxima)
    return dmin, arg, (d <= thr).any(2)


def bound_nearest_partner(inp):
    """On the lattice every operation before the square root is exact and sqrtf is correctly rounded: dmin is bit-equal, and so are the
    index (first among ties) and the flag (0.25 is attained exactly)."""
    return 0.0


def nearest_emulate(inp, mutant=None):
    a, b = inp["a"], inp["b"]
    aa, bb = (a * a).sum(-1), (b * b).sum(-1)
    dot = (a[:, :, None, 0] * b[:, None, :, 0] + a[:, :, None, 1] * b[:, None, :, 1]) + a[:, :, None, 2] * b[:, None, :, 2]
    d = _sqrt32(((aa[:, :, None] - 2 * dot) + bb[:, None, :]).clamp(min=0))
    if not inp["over_b"]:
        d = d.transpose(1, 2)
    nred = d.shape[2]
    keep = nred - nred % 256 if mutant == "skip_tail" else (nred - 1 if mutant == "drop_last" else nred)
    if keep == 0:
        return torch.full(d.shape[:2], 3.4e38), torch.zeros(d.shape[:2], dtype=torch.int64), torch.zeros(d.shape[:2], dtype=torch.bool)
    d = d[:, :, :keep]
    dmin = d.min(2)[0]
    hit = (d == dmin[..., None]).int()
    arg = keep - 1 - hit.flip(2).argmax(2) if mutant == "last_tie" else hit.argmax(2)
    thr = torch.tensor(inp["thr"], dtype=torch.float32)
    return dmin, arg, ((d < thr) if mutant == "lt_for_le" else (d <= thr)).any(2)


def nearest_check(inp, got):
    ref = _once(inp, ("_ref", inp["over_b"]), lambda: nearest_partner_64(inp["a"], inp["b"], inp["over_b"], inp["thr"]))
    ok = (torch.equal(got[0].double(), ref[0]) and torch.equal(got[1].long(), ref[1].long()) and torch.equal(got[2].bool(), ref[2]))
    return ok, 0.0 if ok else math.inf


nearest_partner = _ns(CASES=NEAREST_CASES, inputs=nearest_inputs, check=nearest_check, emulate=nearest_emulate,
                      MUTANTS=("drop_last", "skip_tail", "last_tie", "lt_for_le"))

# ============================================================================================================== gather_rows, copy_rows
# (B, N, J, words, off, prepend, alt: 0 none / 1 one row per batch / 2 one row for all, idx64)
GATHER_CASES = [
    (2, 50, 4200, 256, 0, 1, 1, 0),   # (J + prepend) * words = 4201 * 256 > 4096 * 256: the grid-stride loop runs
    (2, 50, 4200, 256, 1, 0, 1, 1),
    (3, 77, 5, 1, 0, 0, 0, 0),
    (3, 77, 33, 3, 1, 1, 1, 1),
    (3, 77, 33, 64, 1, 1, 2, 0),
    (1, 1, 1, 2, 0, 0, 0, 1),
]


def gather_inputs(case):
    """idx in [0, N - 1 + off]: N - 1 is there with off = 0, N (the last row) and 0 (the alternative row) with off = 1."""
    B, N, J, words, off, prepend, alt, idx64 = case
    g = _gen("gather", case)
    idx = torch.randint(0, N + off, (B, J), generator=g)
    idx[:, 0] = N - 1 + off
    idx[:, -1] = 0
    feats = torch.randint(-2 ** 31, 2 ** 31 - 1, (B, N, words), generator=g).int()
    altr = None
    if alt:
        altr = torch.randint(-2 ** 31, 2 ** 31 - 1, (B if alt == 1 else 1, words), generator=g).int()
    return {"feats": feats, "idx": idx.long() if idx64 else idx.int(), "alt": altr, "off": off, "prepend": prepend, "alt_stride": words if alt == 1 else 0}


def gather_rows_64(inp, alt_row=0, off=None):
    """out[b, p + j] = feats[b, idx[b, j] - off] (clamped to the last row), the alternative row of batch b where idx - off < 0 and, with
    `prepend`, in front.  Rows are 4-byte words: a copy, bound 0."""
    feats, idx, alt = inp["feats"], inp["idx"].long(), inp["alt"]
    B, N, words = feats.shape
    off = inp["off"] if off is None else off
    src = idx - off
    out = feats[torch.arange(B)[:, None], src.clamp(0, N - 1)]
    if alt is None:
        a = torch.zeros(B, words, dtype=torch.int32)
    else:
        flat = torch.cat([alt.reshape(-1), torch.zeros(words, dtype=torch.int32)])   # (room for the mutant that reads one row on)
        a = torch.stack([flat[(b + alt_row) * inp["alt_stride"]:][:words] for b in range(B)])
    out = torch.where((src < 0)[..., None], a[:, None], out)
    if inp["prepend"]:
        out = torch.cat([a[:, None], out], 1)
    return out


def gather_emulate(inp, mutant=None):
    out = gather_rows_64(inp, alt_row=1 if mutant == "alt_row1" else 0, off=0 if mutant == "off_ignored" else None)
    if mutant == "drop_last":
        out = out.clone()
        out[:, -1, -1] = -1 - out[:, -1, -1]
    return out


def _check_equal(ref, got):
    ok = got.shape == ref.shape and got.dtype == ref.dtype and torch.equal(got, ref)
    return ok, 0.0 if ok else math.inf


gather_rows = _ns(CASES=GATHER_CASES, inputs=gather_inputs, check=lambda inp, got: _check_equal(gather_rows_64(inp), got),
                  emulate=gather_emulate, MUTANTS=("alt_row1", "off_ignored", "drop_last"))

COPY_GRID_WORDS = 64 * 256   # the launcher caps the grid at 64 workgroups of 256 words: a longer row runs the grid-stride loop
COPY_CASES = [(rows, words, stride0) for rows in (1, 7) for words in (1, COPY_GRID_WORDS, COPY_GRID_WORDS + 1) for stride0 in (0, 1)]


def copy_inputs(case):
    """src: `rows` rows words + 3 apart, or one row for all (stride 0); the destination pitch is words + 5."""
    rows, words, stride0 = case
    g = _gen("copy", case)
    sp = 0 if stride0 else words + 3
    src = torch.randint(-2 ** 31, 2 ** 31 - 1, (1 if stride0 else rows, words + 3), generator=g).int()
    return {"src": src, "rows": rows, "words": words, "src_pitch": sp, "dst_pitch": words + 5}


def copy_rows_64(inp):
    """dst[r, :words] = src[r * src_pitch : r * src_pitch + words]: a copy, bound 0 (the rest of the destination pitch is not written)."""
    s = inp["src"].reshape(-1)
    return torch.stack([s[r * inp["src_pitch"]:][:inp["words"]] for r in range(inp["rows"])])


def copy_emulate(inp, mutant=None):
    out = copy_rows_64(inp).clone()
    if mutant == "drop_last":
        out[:, -1] = -1 - out[:, -1]
    if mutant == "skip_tail":
        out[:, COPY_GRID_WORDS:] = 0x7FC00000
    return out


copy_rows = _ns(CASES=COPY_CASES, inputs=copy_inputs, check=lambda inp, got: _check_equal(copy_rows_64(inp), got), emulate=copy_emulate,
                MUTANTS=("drop_last", "skip_tail"))

# ============================================================================================================================ nan_to_num_multi
NAN_SIZES = (1, 255, 256, 64 * 256 + 1, 100000)   # the grid is 64 workgroups of 256: from 64 * 256 + 1 elements on the grid-stride loop runs
NAN_REPL = (0.0, 1e5, -1e5)
NAN_CASES = [("table",)]
_SPECIALS = (float("nan"), float("inf"), float("-inf"), -0.0, 1e-45, -1e-40, FLT_MAX, -FLT_MAX)


def nan_inputs(case):
    """One table of five tensors; NaN, +-inf, -0.0, subnormals and +-FLT_MAX at the first and last positions and on both sides of every
    multiple of the grid (64 * 256), every non-finite value at least once at each of them."""
    g = _gen("nan", case)
    ts = []
    for t, n in enumerate(NAN_SIZES):
        x = torch.randn(n, generator=g)
        marks = sorted({p for p in (0, 1, 2, n - 3, n - 2, n - 1) if 0 <= p < n} | {q * COPY_GRID_WORDS + d for q in range(1, 7) for d in (-2, -1, 0, 1, 2) if 0 <= q * COPY_GRID_WORDS + d < n})
        for k, p in enumerate(marks):
            x[p] = _SPECIALS[(k + t) % 3 if p in (0, n - 1, COPY_GRID_WORDS) else (k + t) % len(_SPECIALS)]
        x[torch.rand(n, generator=g) < 0.01] = float("nan")
        ts.append(x)
    return {"tensors": ts, "repl": tuple(f32(v) for v in NAN_REPL)}


def nan_to_num_64(x, repl):
    """NaN, +inf, -inf replaced; every finite bit pattern (-0.0 and subnormals included) kept: compared as int32, bound 0"""
    out = x.clone()
    out[torch.isnan(x)] = repl[0]
    out[x == math.inf] = repl[1]
    out[x == -math.inf] = repl[2]
    return out.view(torch.int32)


def nan_emulate(inp, mutant=None):
    outs = []
    for x in inp["tensors"]:
        y = nan_to_num_64(x, inp["repl"]).clone()
        raw = x.view(torch.int32)
        if mutant == "drop_last":
            y[-1] = raw[-1]
        if mutant == "skip_tail":
            y[COPY_GRID_WORDS:] = raw[COPY_GRID_WORDS:]
        outs.append(y)
    return outs


def nan_check(inp, got):
    ok = all(torch.equal(g.view(torch.int32), nan_to_num_64(x, inp["repl"])) for g, x in zip(got, inp["tensors"])) and len(got) == len(inp["tensors"])
    return ok, 0.0 if ok else math.inf


nan_to_num_multi = _ns(CASES=NAN_CASES, inputs=nan_inputs, check=nan_check, emulate=nan_emulate, MUTANTS=("drop_last", "skip_tail"))

# ============================================================================================================================ patchify
PATCHIFY_CASES = [(S, na, nb, Kp, split) for S in (14, 224, 518) for (na, nb) in ((1, 0), (2, 3)) for (Kp, split) in
                  ((588, 0), (640, 0), (704, 0), (608, 1), (640, 1))]


def patchify_inputs(case):
    S, na, nb, Kp, split = case

    def make():
        g = _gen("patchify", S, na, nb)
        return {"a": torch.randn(na, 3, S, S, generator=g), "b": torch.randn(nb, 3, S, S, generator=g) if nb else None}

    d = dict(_memo("patchify", (S, na, nb), make))
    d["Kp"], d["split"] = Kp, split
    return d


def patch_matrix_64(a, b, Kp):
    """Both crops unfolded into 14 x 14 patches: row = (crop, gy, gx), column = c * 196 + py * 14 + px, zero-padded to Kp columns.  (fp32:
    nothing is computed.)"""
    x = a if b is None else torch.cat([a, b], 0)
    n, _, S, _ = x.shape
    g = S // 14
    mat = x.reshape(n, 3, g, 14, g, 14).permute(0, 2, 4, 1, 3, 5).reshape(n * g * g, 588)
    return F.pad(mat, (0, Kp - 588))


def split_layout(mat, rb=bf16_rne):
    """The split layout of the fp32-class GEMM: per row and 32-column block one line [hi (32 bf16) | lo (32 bf16)], hi = bf16(x),
    lo = bf16(x - hi) (the fp32 difference is exact): (rows, 2 K) bf16 values, returned as fp32."""
    hi = rb(mat)
    lo = rb(mat - hi)
    M, K = mat.shape
    return torch.stack([hi.reshape(M, K // 32, 32), lo.reshape(M, K // 32, 32)], 2).reshape(M, 2 * K)


def patchify_64(inp, rb=bf16_rne):
    mat = patch_matrix_64(inp["a"], inp["b"], inp["Kp"])
    return split_layout(mat, rb) if inp["split"] else rb(mat)


def bound_patchify(inp):
    """A rearrangement and one RNE rounding (two for the split form, the second of an exact difference): bound 0, compared as bf16 bits."""
    return 0.0


def patchify_emulate(inp, mutant=None):
    out = patchify_64(inp, bf16_trunc if mutant == "trunc_bf16" else bf16_rne).clone()
    if mutant == "drop_last":
        out[-1, 586:588] = float("nan")
    return out


def patchify_check(inp, got):
    ref = _once(inp, "_ref", lambda: patchify_64(inp).bfloat16())
    ok = got.shape == ref.shape and torch.equal(got.bfloat16().view(torch.int16), ref.view(torch.int16))
    return ok, 0.0 if ok else math.inf


patchify = _ns(CASES=PATCHIFY_CASES, inputs=patchify_inputs, check=patchify_check, emulate=patchify_emulate, MUTANTS=("trunc_bf16", "drop_last"))

# ============================================================================================================================ add_layernorm
LN_C = (4, 30, 100, 256, 257, 1000, 1024)
LN_ROWS = (1, 5, 777)
LN_DTYPES = [(ab, bk, ob) for ab in (0, 1) for bk in ("none", "f32", "bf16") for ob in (0, 1)]   # a fp32 / bf16; b absent / fp32 / bf16; out fp32 / bf16
LN_EPS = 1e-6
LN_CASES = [(C, rows, fam, ab, bk, ob) for C in LN_C for rows in LN_ROWS for fam in range(9 if rows < 777 else 1) for (ab, bk, ob) in LN_DTYPES]


def ln_inputs(case):
    """Rows of the families of test_layernorm_rows_gpu.py: family `fam` for the short cases, all nine stacked (86 or 87 rows each) for 777."""
    from test_layernorm_rows_gpu import FAMILIES, family_rows

    C, rows, fam, ab, bk, ob = case

    def make():
        if rows < 777:
            x = family_rows(FAMILIES[fam], rows, C, seed=3)
        else:
            parts = [family_rows(f, rows // 9 + (i < rows % 9), C, seed=3 + i) for i, f in enumerate(FAMILIES)]
            x = torch.cat(parts, 0)
        g = _gen("ln", C)
        return {"x": x, "b32": family_rows("centred", rows, C, seed=4), "w": 1 + 0.3 * torch.randn(C, generator=g), "bias": 0.2 * torch.randn(C, generator=g)}

    m = _memo("ln", (C, rows, fam), make)
    d = {"a": bf16_rne(m["x"]) if ab else m["x"], "b": None if bk == "none" else (bf16_rne(m["b32"]) if bk == "bf16" else m["b32"]),
         "w": m["w"], "bias": m["bias"], "eps": LN_EPS, "a_bf16": ab, "b_bf16": int(bk == "bf16"), "out_bf16": ob}
    return d


def add_layernorm_64(inp):
    """LayerNorm(a + b) w + bias of the kernel's own (fp32 or bf16) inputs: (s, result)"""
    from test_layernorm_rows_gpu import ln64

    s = inp["a"].double() + (0 if inp["b"] is None else inp["b"].double())
    return s, ln64(s, inp["w"], inp["bias"], inp["eps"])[1]


def bound_add_layernorm(inp):
    """The tolerances of test_layernorm_rows_gpu.py::test_standalone_layernorm_kernels, unchanged.  bf16 output: 2^-8 |ref| + 2e-3.  fp32
    output: 1e-5 |ref| + 1e-4 + the resolution of the fp32 row sums, 2^-20 max|row| / sqrt(var + eps) |w|."""
    s, ref = _once(inp, "_ref", lambda: add_layernorm_64(inp))
    if inp["out_bf16"]:
        return 2.0 ** -8 * ref.abs() + 2e-3
    var = ((s - s.mean(1, keepdim=True)) ** 2).mean(1, keepdim=True)
    floor = 2.0 ** -20 * s.abs().amax(1, keepdim=True) / torch.sqrt(var + inp["eps"]) * inp["w"].double().abs()
    return 1e-5 * ref.abs() + 1e-4 + floor


def ln_emulate(inp, mutant=None):
    s = inp["a"] if inp["b"] is None else inp["a"] + inp["b"]
    C = s.shape[1]
    keep = C - C % 4 if mutant == "skip_tail" else (C - 1 if mutant == "drop_last" else C)

    def total(v):
        t = _strided32(v[:, :keep], 64) if keep else torch.zeros(v.shape[0])
        return t + v[:, -1] if mutant == "twice" else t

    mean = (total(s) / C)[:, None]
    d = s - mean
    rstd = 1.0 / _sqrt32(total(d * d) / C + torch.tensor(inp["eps"], dtype=torch.float32))[:, None]
    y = d * rstd * inp["w"] + inp["bias"]
    return bf16_rne(y) if inp["out_bf16"] else y


def ln_check(inp, got):
    return compare(got, _once(inp, "_ref", lambda: add_layernorm_64(inp))[1], bound_add_layernorm(inp))


add_layernorm = _ns(CASES=LN_CASES, inputs=ln_inputs, check=ln_check, emulate=ln_emulate, MUTANTS=("drop_last", "twice", "skip_tail"))

# ============================================================================================================================ bilinear_sample
BILINEAR_GEOM = ((16, 224, 224), (37, 518, 518), (1, 14, 14), (4, 56, 42), (16, 224, 160), (5, 70, 70))
BILINEAR_CASES = [(side, H, W, zb, off) for (side, H, W) in BILINEAR_GEOM for zb in (0, 1) for off in (0, 5)]
BILINEAR_PREFIX = 1e9
BILINEAR_EMULATION_SHARE = 0.8 * 0.5   # the fp32 restatement of bilinear_tap stays below 0.8 of HALF the bound


def bilinear_inputs(case):
    """z (1, off + side^2, 4, 4, 256): the up-projection output in its native order behind `off` prefix tokens filled with 1e9; choose:
    every border pixel of the (H, W) crop and 2000 random ones.  A bf16 map is judged on its own rounded values."""
    side, H, W, zb, off = case

    def make():
        g = _gen("bilinear", side, H, W)
        z = torch.randn(1, side * side, 4, 4, 256, generator=g)
        ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        border = (ys == 0) | (ys == H - 1) | (xs == 0) | (xs == W - 1)
        choose = torch.cat([(ys * W + xs)[border], torch.randint(0, H * W, (2000,), generator=g)])[None].contiguous()
        return {"z32": z, "choose": choose}

    m = _memo("bilinear", (side, H, W), make)
    z = bf16_rne(m["z32"]) if zb else m["z32"]
    shared = _memo("bilinear_shared", (side, H, W, zb), dict)
    zz = torch.cat([torch.full((1, off, 4, 4, 256), BILINEAR_PREFIX), z], 1) if off else z
    return {"z": zz, "map": z, "choose": m["choose"], "side": side, "H": H, "W": W, "off": off, "z_bf16": zb, "_shared": shared}


def _map_hwc(inp):
    side = inp["side"]
    return inp["map"].reshape(1, side, side, 4, 4, 256).permute(0, 1, 3, 2, 4, 5).reshape(1, 4 * side, 4 * side, 256)


def bilinear_sample_64(inp):
    """F.interpolate(map, (H, W), bilinear, align_corners=False) in float64 on the permuted map, read at the chosen pixels (evaluated 32
    channels at a time: the whole (256, 518, 518) float64 image is 550 MB)."""
    def make():
        m = _map_hwc(inp).permute(0, 3, 1, 2).double()
        ch = inp["choose"][0]
        out = [F.interpolate(m[:, c:c + 32], size=(inp["H"], inp["W"]), mode="bilinear", align_corners=False).reshape(32, -1)[:, ch].t() for c in range(0, 256, 32)]
        return torch.cat(out, 1)[None]

    return _once(inp["_shared"], "ref", make)


def _taps(py, px, H, W, hw, dt, variant=None):
    """The source cell and weights of pixel (py, px) as bilinear_tap forms them, in `dt` arithmetic (torch dtype)."""
    def axis(p, n):
        p = p.to(dt)
        scale = (torch.tensor(float(hw), dtype=dt) / torch.tensor(float(n), dtype=dt))
        if variant == "align_corners":
            s = p * (torch.tensor(float(hw - 1), dtype=dt) / torch.tensor(float(max(n - 1, 1)), dtype=dt))
        elif variant == "no_half":
            s = ((p + 0.5) * scale).clamp(min=0)
        else:
            s = ((p + 0.5) * scale - 0.5).clamp(min=0)
        i0 = s.long().clamp(max=hw - 1)
        i1 = (i0 + 1).clamp(max=hw - 1)
        return i0, i1, s - i0.to(dt), ((p + 0.5) * scale - 0.5) < 0

    y0, y1, ly, cy = axis(py, H)
    x0, x1, lx, cx = axis(px, W)
    return y0, y1, ly, x0, x1, lx, cy | cx


def bound_bilinear_sample(inp):
    """The source coordinate is computed in fp32 from values up to 4 side: it carries at most 2 ulp(4 side) per axis, and the interpolant
    (continuous across cell boundaries) changes by at most (max - min of the cell's four taps) per unit of either coordinate:
    4 ulp(4 side) (max - min).  The three lerps round six times in all on values no larger than the taps: + 6 U max|tap|."""
    def make():
        hw = 4 * inp["side"]
        ch = inp["choose"][0]
        y0, y1, _, x0, x1, _, _ = _taps(ch // inp["W"], ch % inp["W"], inp["H"], inp["W"], hw, torch.float64)
        m = _map_hwc(inp)[0].double()
        t = torch.stack([m[y0, x0], m[y0, x1], m[y1, x0], m[y1, x1]])
        ulp = float(np.spacing(np.float32(hw)))
        return (4 * ulp * (t.max(0)[0] - t.min(0)[0]) + 6 * U * t.abs().max(0)[0])[None]

    return _once(inp["_shared"], "bound", make)


def bilinear_emulate(inp, mutant=None):
    hw = 4 * inp["side"]
    ch = inp["choose"][0]
    y0, y1, ly, x0, x1, lx, clamped = _taps(ch // inp["W"], ch % inp["W"], inp["H"], inp["W"], hw, torch.float32,
                                            variant=mutant if mutant in ("align_corners", "no_half") else None)
    m = _map_hwc(inp)[0]
    ly, lx = ly[:, None], lx[:, None]
    top = (1 - lx) * m[y0, x0] + lx * m[y0, x1]
    bot = (1 - lx) * m[y1, x0] + lx * m[y1, x1]
    out = (1 - ly) * top + ly * bot
    if mutant == "border_mean":   # the pixels whose source coordinate is clamped to 0 read the FIRST tap alone, not the mean of the cell
        mean = 0.25 * (m[y0, x0] + m[y0, x1] + m[y1, x0] + m[y1, x1])
        out = torch.where(clamped[:, None], mean, out)
    if mutant == "drop_last":
        out[:, -1] = float("nan")
    return out[None]


def bilinear_check(inp, got):
    return compare(got, bilinear_sample_64(inp), bound_bilinear_sample(inp))


bilinear_sample = _ns(CASES=BILINEAR_CASES, inputs=bilinear_inputs, check=bilinear_check, emulate=bilinear_emulate,
                      MUTANTS=("border_mean", "align_corners", "no_half", "drop_last"))

# ============================================================================================================================ the registry
KERNELS = {
    "bmm_f32": bmm, "cloud_radius": cloud_radius, "scale_by_radius": scale_by_radius, "pose_score": pose_score, "token_sum_bf16": token_sum,
    "row_dot": row_dot, "normalize_rows": normalize_rows, "overlap_scores": overlap_scores, "rigid_rows_bf16": rigid_rows,
    "nearest_partner": nearest_partner, "gather_rows": gather_rows, "copy_rows": copy_rows, "nan_to_num_multi": nan_to_num_multi,
    "patchify": patchify, "add_layernorm": add_layernorm, "bilinear_sample": bilinear_sample,
}


def ratio_table(ratios, title):
    """`ratios`: kernel -> worst error / bound (0 where the bound is 0 and the result equal)."""
    lines = ["%-18s %s" % ("kernel", title)]
    lines += ["%-18s %.3f" % (k, ratios[k]) if k in ratios else "%-18s -" % k for k in KERNELS]
    return "\n".join(lines)
