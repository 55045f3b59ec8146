// fp32-class attention kernels for gfx950 (C ABI part 2): the SAME algorithms as attn.hip (token
// attention of the correspondence transformer) and vit_attn.hip (ViT patch attention), for float32
// inputs / outputs, so that the fp32 configuration the reference runs by default
// (configs/main_cfg.py:87-89, test.amp.enabled=False) -- and all golden parity tests -- also go through
// hand-written HIP.  gfx950 has no reduced-precision fast path for fp32 matrix inputs (no xf32), and its
// exact fp32 MFMA runs at 1/16 of the bf16 rate; instead every operand is split on the fly into
// hi + lo bfloat16 parts and each product is issued as 3 bf16 MFMAs (a_hi b_hi + a_hi b_lo + a_lo b_hi,
// fp32 accumulation): ~2^-16 relative error per product, i.e. fp32-class results at 5x the fp32 MFMA rate.
#include "attn_common.h"      // (TA_NT / TA_MP, row16_sum / row16_max, zero8)
#include "vit_attn_common.h"  // (va_store_split: the split-layout output of vit_attn_f32_kernel<true>)

namespace unopose {

__device__ __forceinline__ bf16x8_hl af_load8(const float *p) {  // 8 consecutive fp32 (32-byte aligned)
  const float4 a = *reinterpret_cast<const float4 *>(p), b = *reinterpret_cast<const float4 *>(p + 4);
  const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  return split8_bf16(v);
}
__device__ __forceinline__ bf16x8_hl af_zero() { return bf16x8_hl{zero8(), zero8()}; }

// ---- The two MFMA loops of the token attention, forward and backward.  Operand streams straight from global memory (K is L2-resident,
// the geometric embedding E is a 2.5 GB HBM stream per launch): the raw 32-byte pieces of the next AF_PF_DEPTH operand pairs are in
// flight while the current one is split and multiplied -- the compiler had issued every pair of loads directly in front of its three
// MFMAs (one exposed memory round trip per 3 MFMAs).
constexpr int AF_PF_DEPTH = 4;  // operand pairs in flight ahead of the MFMAs of the token attention
struct AfRaw {
  float4 a, b;
};
__device__ __forceinline__ AfRaw af_ld8(const float *p) {
  return AfRaw{*reinterpret_cast<const float4 *>(p), *reinterpret_cast<const float4 *>(p + 4)};
}
__device__ __forceinline__ bf16x8_hl af_sp8(const AfRaw &r) {
  const float v[8] = {r.a.x, r.a.y, r.a.z, r.a.w, r.b.x, r.b.y, r.b.z, r.b.w};
  return split8_bf16(v);
}

// A fragment of k-step ks of a block-diagonal A operand: row li = (query row, head a_h) of A_row only sees head a_h's 64 channels
__device__ __forceinline__ bf16x8_hl af_head_frag(const float *A_row, bool a_valid, int a_h, int kg, int ks) {
  const int kk = ks * 32 + kg * 8;
  bf16x8_hl a = af_zero();
  if (a_valid && (kk >> 6) == a_h) a = af_load8(A_row + kk);
  return a;
}

// acc[t] += A B^T over the 8 k-steps x TA_NT key tiles, k-step outermost.  a_frag(ks): this lane's A fragment of k-step ks, asked for
// once per k-step and in order; B_rows: m rows of 256 channels with stride ldb (rows >= m read row m - 1: masked by the caller).
template <class AFrag>
__device__ __forceinline__ void af_scores(AFrag a_frag, const float *B_rows, size_t ldb, int m, int nt_valid, int li, int kg,
                                          f32x4 (&acc)[TA_NT]) {
  constexpr int NPAIR = 8 * TA_NT;
  auto addr = [&](int i) { return B_rows + (size_t)min((i % TA_NT) * 16 + li, m - 1) * ldb + (i / TA_NT) * 32 + kg * 8; };
  AfRaw ring[AF_PF_DEPTH];
#pragma unroll
  for (int i = 0; i < AF_PF_DEPTH; ++i) ring[i] = af_ld8(addr(i));
  bf16x8_hl a = af_zero();
#pragma unroll
  for (int i = 0; i < NPAIR; ++i) {
    const int ks = i / TA_NT, t = i % TA_NT;
    if (t == 0) a = a_frag(ks);
    const AfRaw cur = ring[i % AF_PF_DEPTH];
    if (i + AF_PF_DEPTH < NPAIR) ring[i % AF_PF_DEPTH] = af_ld8(addr(i + AF_PF_DEPTH));
    if (t < nt_valid) acc[t] = mfma3_hh_hl_lh_16x16(a, af_sp8(cur), acc[t]);
  }
}

// emit(nt, o) for the 16 channel tiles nt of frags . BT, where BT (256, TA_MP) is the channel-major, zero-padded B^T of this cloud and
// o the value of row (query row kg, head nt >> 2), channel nt * 16 + li: only the head-matching quarter of the D tile is kept.
template <class Emit>
__device__ __forceinline__ void af_apply(const bf16x8_hl (&frags)[TA_MP / 32], const float *BT, int li, int kg, Emit emit) {
  constexpr int NKS = TA_MP / 32, NP2 = 16 * NKS;
  auto addr = [&](int i) { return BT + (size_t)((i / NKS) * 16 + li) * TA_MP + kg * 8 + (i % NKS) * 32; };
  AfRaw ring[AF_PF_DEPTH];
#pragma unroll
  for (int i = 0; i < AF_PF_DEPTH; ++i) ring[i] = af_ld8(addr(i));
  f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < NP2; ++i) {
    const int nt = i / NKS, ks = i % NKS;
    if (ks == 0) o = f32x4{0.f, 0.f, 0.f, 0.f};
    const AfRaw cur = ring[i % AF_PF_DEPTH];
    if (i + AF_PF_DEPTH < NP2) ring[i % AF_PF_DEPTH] = af_ld8(addr(i + AF_PF_DEPTH));
    o = mfma3_hh_hl_lh_16x16(frags[ks], af_sp8(cur), o);
    if (ks == NKS - 1) emit(nt, o[nt >> 2]);
  }
}

// ---- token attention (see attn.hip for the scheme): one wave = 4 query rows x 4 heads ----------------
// STORE_P (training forward): P is also written to pst (B,4,n,TA_MP), zero on the padded keys, for the backward below.
template <bool RPE, bool STORE_P = false>
__global__ __launch_bounds__(256) void token_attn_f32_kernel(const float *__restrict__ q, int ldq,
                                                             const float *__restrict__ k, int ldk,
                                                             const float *__restrict__ vt,
                                                             const float *__restrict__ qp, int ldqp,
                                                             const float *__restrict__ E, int n, int m, float scale,
                                                             float *__restrict__ out, float *__restrict__ pst) {
  __shared__ __attribute__((aligned(16))) float Pl[4][16][TA_MP + 4];
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = (blockIdx.x * 4 + wave) * 4;
  if (n0 >= n) return;
  const int li = lane & 15, kg = lane >> 4;
  const int a_nl = li >> 2, a_h = li & 3;
  const bool a_valid = n0 + a_nl < n;
  const float *Q = q + ((size_t)b * n + n0 + a_nl) * ldq;
  const float *K = k + (size_t)b * m * ldk;
  f32x4 acc[TA_NT];
#pragma unroll
  for (int t = 0; t < TA_NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nt_valid = (m + 15) >> 4;
  af_scores([&](int ks) { return af_head_frag(Q, a_valid, a_h, kg, ks); }, K, ldk, m, nt_valid, li, kg, acc);
  if (RPE) {
    for (int nl = 0; nl < 4; ++nl) {
      if (n0 + nl >= n) break;
      const float *QP = qp + ((size_t)b * n + n0 + nl) * ldqp + a_h * 256;
      AfRaw araw = af_ld8(QP + kg * 8);  // the query-side fragment of k-step 0; the next one is fetched a whole k-step ahead
      auto a_frag = [&](int ks) {
        bf16x8_hl a = af_zero();
        if (a_nl == nl) a = af_sp8(araw);
        if (ks + 1 < 8) araw = af_ld8(QP + (ks + 1) * 32 + kg * 8);
        return a;
      };
      af_scores(a_frag, E + ((size_t)b * n + n0 + nl) * (size_t)m * 256, 256, m, nt_valid, li, kg, acc);
    }
  }
  float mx[4] = {-3e38f, -3e38f, -3e38f, -3e38f};
#pragma unroll
  for (int t = 0; t < TA_NT; ++t) {
    const bool ok = t * 16 + li < m;
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      acc[t][h] = ok ? acc[t][h] * scale : -3e38f;
      mx[h] = fmaxf(mx[h], acc[t][h]);
    }
  }
  float sm[4];
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    mx[h] = row16_max(mx[h]);
    sm[h] = 0.f;
  }
#pragma unroll
  for (int t = 0; t < TA_NT; ++t) {
    const bool ok = t * 16 + li < m;
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const float p = ok ? expf(acc[t][h] - mx[h]) : 0.f;
      acc[t][h] = p;
      sm[h] += p;
    }
  }
#pragma unroll
  for (int h = 0; h < 4; ++h) sm[h] = 1.f / row16_sum(sm[h]);
#pragma unroll
  for (int t = 0; t < TA_NT; ++t)
#pragma unroll
    for (int h = 0; h < 4; ++h) Pl[wave][kg * 4 + h][t * 16 + li] = acc[t][h] * sm[h];
  if (STORE_P && n0 + kg < n) {
    float *Pr = pst + ((size_t)b * 4 * n + n0 + kg) * TA_MP + li;
#pragma unroll
    for (int t = 0; t < TA_NT; ++t)
#pragma unroll
      for (int h = 0; h < 4; ++h) Pr[(size_t)h * n * TA_MP + t * 16] = acc[t][h] * sm[h];
  }
  wave_lds_handover();
  bf16x8_hl pa[TA_MP / 32];
#pragma unroll
  for (int ks = 0; ks < TA_MP / 32; ++ks) pa[ks] = af_load8(&Pl[wave][li][ks * 32 + kg * 8]);
  af_apply(pa, vt + (size_t)b * 256 * TA_MP, li, kg, [&](int nt, float o) {
    if (n0 + kg < n) out[((size_t)b * n + n0 + kg) * 256 + nt * 16 + li] = o;
  });
}

// ---- token attention backward (training): S = scale (q k^T [+ qp . E]), P = softmax(S), O = P v; given dO:
//   dP = dO v^T, delta = rowsum(P dP) (= rowsum(dO O)), dS = P (dP - delta)
//   dq = scale dS k, dk = scale dS^T q, dv = P^T dO, dqp = scale dS E, dE = scale sum_h dS_h qp_h
// Three kernels, each output element owned by one thread (no atomics): dq + dS (the forward's scheme: hi / lo-split MFMAs), the RPE terms
// (E streamed once, dE written once; exact fp32 FMA: 8 per element of E, far under the memory time) and dk / dv (fp32 FMA, LDS tiles).

// One wave = 4 query rows x 4 heads, as in the forward.  P: the forward's (B,4,n,TA_MP) (zero on padded keys, so dS is too);
// kt (B,256,TA_MP) = k^T zero-padded.  Writes dS (B,4,n,TA_MP) and dq (B,n,256).
__global__ __launch_bounds__(256) void token_attn_f32_bwd_dq_kernel(const float *__restrict__ dout, const float *__restrict__ v, int ldv,
                                                                    const float *__restrict__ P, const float *__restrict__ kt, int n, int m,
                                                                    float scale, float *__restrict__ dS, float *__restrict__ dq) {
  __shared__ __attribute__((aligned(16))) float Sl[4][16][TA_MP + 4];
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = (blockIdx.x * 4 + wave) * 4;
  if (n0 >= n) return;
  const int li = lane & 15, kg = lane >> 4;
  const int a_nl = li >> 2, a_h = li & 3;
  const bool a_valid = n0 + a_nl < n, row_ok = n0 + kg < n;
  const float *G = dout + ((size_t)b * n + n0 + a_nl) * 256;
  const float *V = v + (size_t)b * m * ldv;
  // dP: the forward's score loop with (dO, v) in place of (q, k)
  f32x4 acc[TA_NT];
#pragma unroll
  for (int t = 0; t < TA_NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  af_scores([&](int ks) { return af_head_frag(G, a_valid, a_h, kg, ks); }, V, ldv, m, (m + 15) >> 4, li, kg, acc);
  // acc[t][h]: dP of query n0 + kg, head h, key t * 16 + li
  const size_t hstride = (size_t)n * TA_MP;
  const size_t prow = ((size_t)b * 4 * n + n0 + kg) * TA_MP + li;
  float p[TA_NT][4], dl[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < TA_NT; ++t)
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      p[t][h] = row_ok ? P[prow + h * hstride + t * 16] : 0.f;
      dl[h] = fmaf(p[t][h], acc[t][h], dl[h]);
    }
#pragma unroll
  for (int h = 0; h < 4; ++h) dl[h] = row16_sum(dl[h]);
#pragma unroll
  for (int t = 0; t < TA_NT; ++t)
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const float ds = p[t][h] * (acc[t][h] - dl[h]);
      Sl[wave][kg * 4 + h][t * 16 + li] = ds;
      if (row_ok) dS[prow + h * hstride + t * 16] = ds;
    }
  wave_lds_handover();
  // dq: the forward's P v loop with (dS, k^T) in place of (P, v^T)
  bf16x8_hl sa[TA_MP / 32];
#pragma unroll
  for (int ks = 0; ks < TA_MP / 32; ++ks) sa[ks] = af_load8(&Sl[wave][li][ks * 32 + kg * 8]);
  af_apply(sa, kt + (size_t)b * 256 * TA_MP, li, kg, [&](int nt, float o) {
    if (row_ok) dq[((size_t)b * n + n0 + kg) * 256 + nt * 16 + li] = o * scale;
  });
}

// RPE terms: one wave per query row i; lane l owns channels 4 l .. 4 l + 3 of every key's E row (one coalesced 1 KiB row per key).
// dqp (B,n,1024) contiguous; dE may be null (no gradient wanted: E is still read for dqp).
constexpr int AB_UNROLL = 8;  // E rows in flight per wave
__global__ __launch_bounds__(256) void token_attn_f32_bwd_rpe_kernel(const float *__restrict__ dS, const float *__restrict__ qp, int ldqp,
                                                                     const float *__restrict__ E, int n, int m, float scale,
                                                                     float *__restrict__ dqp, float *__restrict__ dE) {
  __shared__ __attribute__((aligned(16))) float4 Sl[4][TA_MP];  // [wave][key]: scale dS of the 4 heads
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + wave;
  if (i >= n) return;
  const size_t row = (size_t)b * n + i, hstride = (size_t)n * TA_MP;
  const float *S = dS + ((size_t)b * 4 * n + i) * TA_MP;
  for (int j = lane; j < m; j += 64)
    Sl[wave][j] = make_float4(scale * S[j], scale * S[hstride + j], scale * S[2 * hstride + j], scale * S[3 * hstride + j]);
  wave_lds_handover();
  float4 qv[4], acc[4];
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    qv[h] = *reinterpret_cast<const float4 *>(qp + row * ldqp + h * 256 + lane * 4);
    acc[h] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const float *Er = E + row * (size_t)m * 256 + lane * 4;
  float *dEr = dE ? dE + row * (size_t)m * 256 + lane * 4 : nullptr;
  auto step = [&](int j, const float4 &e) {
    const float4 s = Sl[wave][j];
    const float sh[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      acc[h].x = fmaf(sh[h], e.x, acc[h].x);
      acc[h].y = fmaf(sh[h], e.y, acc[h].y);
      acc[h].z = fmaf(sh[h], e.z, acc[h].z);
      acc[h].w = fmaf(sh[h], e.w, acc[h].w);
    }
    if (dEr) {
      float4 d = make_float4(sh[0] * qv[0].x, sh[0] * qv[0].y, sh[0] * qv[0].z, sh[0] * qv[0].w);
#pragma unroll
      for (int h = 1; h < 4; ++h) {
        d.x = fmaf(sh[h], qv[h].x, d.x);
        d.y = fmaf(sh[h], qv[h].y, d.y);
        d.z = fmaf(sh[h], qv[h].z, d.z);
        d.w = fmaf(sh[h], qv[h].w, d.w);
      }
      *reinterpret_cast<float4 *>(dEr + (size_t)j * 256) = d;
    }
  };
  int j = 0;
  for (; j + AB_UNROLL <= m; j += AB_UNROLL) {
    float4 e[AB_UNROLL];
#pragma unroll
    for (int u = 0; u < AB_UNROLL; ++u) e[u] = *reinterpret_cast<const float4 *>(Er + (size_t)(j + u) * 256);
#pragma unroll
    for (int u = 0; u < AB_UNROLL; ++u) step(j + u, e[u]);
  }
  for (; j < m; ++j) step(j, *reinterpret_cast<const float4 *>(Er + (size_t)j * 256));
#pragma unroll
  for (int h = 0; h < 4; ++h) *reinterpret_cast<float4 *>(dqp + row * 1024 + h * 256 + lane * 4) = acc[h];
}

// dk / dv: one workgroup per (32 keys, head, batch); thread = key j0 + (tid & 31) x 8 channels of the head.  The query rows go through
// LDS in chunks of 32 (dS, P: 32 x 32; q, dO: 32 x 64 of the head).
constexpr int AB_JT = 32, AB_IC = 32;
__global__ __launch_bounds__(256) void token_attn_f32_bwd_dkv_kernel(const float *__restrict__ q, int ldq, const float *__restrict__ dout,
                                                                     const float *__restrict__ P, const float *__restrict__ dS, int n, int m,
                                                                     float scale, float *__restrict__ dk, float *__restrict__ dv) {
  __shared__ __attribute__((aligned(16))) float sS[AB_IC][AB_JT], sP[AB_IC][AB_JT], sQ[AB_IC][64 + 4], sG[AB_IC][64 + 4];
  const int b = blockIdx.z, h = blockIdx.y, j0 = blockIdx.x * AB_JT, tid = threadIdx.x;
  const int jl = tid & 31, c0 = (tid >> 5) * 8;
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 ak0 = z4, ak1 = z4, av0 = z4, av1 = z4;
  auto fma4 = [](float s, const float4 &x, float4 &a) {
    a.x = fmaf(s, x.x, a.x);
    a.y = fmaf(s, x.y, a.y);
    a.z = fmaf(s, x.z, a.z);
    a.w = fmaf(s, x.w, a.w);
  };
  const size_t pbase = ((size_t)b * 4 + h) * n * TA_MP + j0;
  for (int i0 = 0; i0 < n; i0 += AB_IC) {
    __syncthreads();
    {
      const int r = tid >> 3, k4 = (tid & 7) * 4, c8 = (tid & 7) * 8;
      const bool ok = i0 + r < n;
      auto ld4 = [&](const float *p) { return ok ? *reinterpret_cast<const float4 *>(p) : make_float4(0.f, 0.f, 0.f, 0.f); };
      const size_t pi = pbase + (size_t)(i0 + r) * TA_MP + k4;  // j0 + k4 + 3 < TA_MP: the padded width holds every tile
      *reinterpret_cast<float4 *>(&sS[r][k4]) = ld4(dS + pi);
      *reinterpret_cast<float4 *>(&sP[r][k4]) = ld4(P + pi);
      const float *qr = q + ((size_t)b * n + i0 + r) * ldq + h * 64 + c8;
      const float *gr = dout + ((size_t)b * n + i0 + r) * 256 + h * 64 + c8;
      *reinterpret_cast<float4 *>(&sQ[r][c8]) = ld4(qr);
      *reinterpret_cast<float4 *>(&sQ[r][c8 + 4]) = ld4(qr + 4);
      *reinterpret_cast<float4 *>(&sG[r][c8]) = ld4(gr);
      *reinterpret_cast<float4 *>(&sG[r][c8 + 4]) = ld4(gr + 4);
    }
    __syncthreads();
    const int ni = min(AB_IC, n - i0);
    for (int r = 0; r < ni; ++r) {
      const float s = sS[r][jl], pr = sP[r][jl];
      fma4(s, *reinterpret_cast<const float4 *>(&sQ[r][c0]), ak0);
      fma4(s, *reinterpret_cast<const float4 *>(&sQ[r][c0 + 4]), ak1);
      fma4(pr, *reinterpret_cast<const float4 *>(&sG[r][c0]), av0);
      fma4(pr, *reinterpret_cast<const float4 *>(&sG[r][c0 + 4]), av1);
    }
  }
  if (j0 + jl >= m) return;
  float *K = dk + ((size_t)b * m + j0 + jl) * 256 + h * 64 + c0, *Vd = dv + ((size_t)b * m + j0 + jl) * 256 + h * 64 + c0;
  *reinterpret_cast<float4 *>(K) = make_float4(ak0.x * scale, ak0.y * scale, ak0.z * scale, ak0.w * scale);
  *reinterpret_cast<float4 *>(K + 4) = make_float4(ak1.x * scale, ak1.y * scale, ak1.z * scale, ak1.w * scale);
  *reinterpret_cast<float4 *>(Vd) = av0;
  *reinterpret_cast<float4 *>(Vd + 4) = av1;
}

// ---- ViT attention (see vit_attn.hip): flash-style; K / V^T chunks in LDS ALREADY SPLIT into bf16 hi / lo planes ---------------
// (the staging threads split every element once per workgroup; round 2 kept fp32 in LDS and every wave re-split every fragment at
// every use -- ~190 of the ~340 vector instructions of a 32-key tile.  Same hi / lo values, so the results are bit-identical.)
constexpr int AV_CHUNK = 64, AV_LDH = 64 + 8, AV_LDVH = AV_CHUNK + 8;  // u16 row strides of the K planes / the V^T planes

// SPLIT: the output is written in the split layout of csrc/gemm_f32.hip (per token and 32-channel block one 128-byte line
// [hi (32 bf16) | lo (32 bf16)]) -- the operand form of the projection GEMM that follows, instead of fp32 + a split pass.
template <bool SPLIT>
__global__ __launch_bounds__(256) void vit_attn_f32_kernel(const float *__restrict__ qkv, int T, int H, float scale_log2e,
                                                           float *__restrict__ out) {
  // K hi | K lo | V^T hi | V^T lo planes (4 x 9 KiB); the same memory is re-used as the output transpose buffer at the end
  constexpr int PLANE_K = AV_CHUNK * AV_LDH, PLANE_V = 64 * AV_LDVH;
  __shared__ __attribute__((aligned(16))) u16 smem16[2 * PLANE_K + 2 * PLANE_V];
  u16 *Kh = smem16, *Kl = smem16 + PLANE_K, *Vh = smem16 + 2 * PLANE_K, *Vl = Vh + PLANE_V;
  float (*Ot)[32][68] = reinterpret_cast<float (*)[32][68]>(smem16);
  static_assert(4 * 32 * 68 * 4 <= (2 * PLANE_K + 2 * PLANE_V) * 2, "output staging must fit the chunk buffers");
  const int b = blockIdx.z, h = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q0 = (blockIdx.x * 4 + wave) * 32;
  const bool active = q0 < T;
  const int col = lane & 31, hb = lane >> 5;
  const int C3 = 3 * H * 64;
  const float *base = qkv + (size_t)b * T * C3;
  bf16x8_hl qf[4];
  {
    const float *qp = base + (size_t)min(q0 + col, T - 1) * C3 + h * 64 + hb * 8;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[ks] = af_load8(qp + ks * 16);
  }
  f32x16 o[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[t][r] = 0.f;
  float m_run = -3e38f, l_run = 0.f;
  for (int c0 = 0; c0 < T; c0 += AV_CHUNK) {
    __syncthreads();
    // 64 keys x 64 channels fp32 for K and V: 1024 float4 each, 4 per thread; split once here
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = tid + i * 256, key = e >> 4, c4 = e & 15;
      const float *src = base + (size_t)min(c0 + key, T - 1) * C3 + h * 64 + c4 * 4;
      const float4 kv = *reinterpret_cast<const float4 *>(src + H * 64);
      float4 vv = *reinterpret_cast<const float4 *>(src + 2 * H * 64);
      if (c0 + key >= T) vv = make_float4(0.f, 0.f, 0.f, 0.f);
      uint2 kh, kl;
      kh.x = cvt_pk_bf16_f32(kv.x, kv.y);
      kh.y = cvt_pk_bf16_f32(kv.z, kv.w);
      kl.x = cvt_pk_bf16_lo(kv.x, kv.y, kh.x);
      kl.y = cvt_pk_bf16_lo(kv.z, kv.w, kh.y);
      *reinterpret_cast<uint2 *>(Kh + key * AV_LDH + c4 * 4) = kh;
      *reinterpret_cast<uint2 *>(Kl + key * AV_LDH + c4 * 4) = kl;
      const uint32_t vh0 = cvt_pk_bf16_f32(vv.x, vv.y), vh1 = cvt_pk_bf16_f32(vv.z, vv.w);
      const uint32_t vl0 = cvt_pk_bf16_lo(vv.x, vv.y, vh0), vl1 = cvt_pk_bf16_lo(vv.z, vv.w, vh1);
      Vh[(c4 * 4 + 0) * AV_LDVH + key] = (u16)(vh0 & 0xFFFF);
      Vh[(c4 * 4 + 1) * AV_LDVH + key] = (u16)(vh0 >> 16);
      Vh[(c4 * 4 + 2) * AV_LDVH + key] = (u16)(vh1 & 0xFFFF);
      Vh[(c4 * 4 + 3) * AV_LDVH + key] = (u16)(vh1 >> 16);
      Vl[(c4 * 4 + 0) * AV_LDVH + key] = (u16)(vl0 & 0xFFFF);
      Vl[(c4 * 4 + 1) * AV_LDVH + key] = (u16)(vl0 >> 16);
      Vl[(c4 * 4 + 2) * AV_LDVH + key] = (u16)(vl1 & 0xFFFF);
      Vl[(c4 * 4 + 3) * AV_LDVH + key] = (u16)(vl1 >> 16);
    }
    __syncthreads();
    if (!active) continue;
    const int nk = min(AV_CHUNK, T - c0);
    for (int kt = 0; kt < nk; kt += 32) {
      const int k0 = c0 + kt;
      f32x16 s;
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const int off = (kt + col) * AV_LDH + ks * 16 + hb * 8;
        const bf16x8_hl kf{*reinterpret_cast<const bf16x8 *>(Kh + off), *reinterpret_cast<const bf16x8 *>(Kl + off)};
        s = mfma3_hh_hl_lh_32x32(kf, qf[ks], s);
      }
      float mx = -3e38f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = k0 + (r & 3) + 8 * (r >> 2) + 4 * hb;
        s[r] = key < T ? s[r] * scale_log2e : -3e38f;
        mx = fmaxf(mx, s[r]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      const float m_new = fmaxf(m_run, mx);
      const float alpha = exp2f(m_run - m_new);
      float ls = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s[r] = exp2f(s[r] - m_new);
        ls += s[r];
      }
      ls += __shfl_xor(ls, 32);
      l_run = l_run * alpha + ls;
      m_run = m_new;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[t][r] *= alpha;
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        float pv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) pv[e] = s[s2 * 8 + e];
        const bf16x8_hl pf = split8_bf16(pv);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          // keys kt + 16 s2 + 4 hb + {0..3} and + 8 + {0..3}: two 8-byte reads per plane
          const int off = (t * 32 + col) * AV_LDVH + kt + s2 * 16 + 4 * hb;
          union { bf16x8 v; uint2 h2[2]; } VH, VL;
          VH.h2[0] = *reinterpret_cast<const uint2 *>(Vh + off);
          VH.h2[1] = *reinterpret_cast<const uint2 *>(Vh + off + 8);
          VL.h2[0] = *reinterpret_cast<const uint2 *>(Vl + off);
          VL.h2[1] = *reinterpret_cast<const uint2 *>(Vl + off + 8);
          const bf16x8_hl vf{VH.v, VL.v};
          o[t] = mfma3_hh_hl_lh_32x32(vf, pf, o[t]);
        }
      }
    }
  }
  __syncthreads();  // every wave is done with the K / V chunk before it becomes the output buffer
  if (!active) return;
  const float inv = 1.f / l_run;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) Ot[wave][col][t * 32 + (r & 3) + 8 * (r >> 2) + 4 * hb] = o[t][r] * inv;
  wave_lds_handover();
  if (SPLIT) {
    const size_t rowb = (size_t)H * 256;
    va_store_split(Ot[wave], reinterpret_cast<char *>(out) + ((size_t)b * T + q0) * rowb + h * 256, rowb, T - q0, lane);
    return;
  }
  // 32 rows x 256 B: 16 lanes per row, 16 B each
#pragma unroll
  for (int it = 0; it < 8; ++it) {
    const int row = it * 4 + (lane >> 4), seg = lane & 15;
    if (q0 + row < T) {
      const float4 v = *reinterpret_cast<const float4 *>(&Ot[wave][row][seg * 4]);
      *reinterpret_cast<float4 *>(out + ((size_t)b * T + q0 + row) * (H * 64) + h * 64 + seg * 4) = v;
    }
  }
}

}  // namespace unopose

using namespace unopose;

extern "C" {

// The eval (P null) and the training forward (P: the saved softmax) behind one launcher; `name`: the entry point, for the error texts
static int launch_token_attn_f32(const char *name, const float *q, int ldq, const float *k, int ldk, const float *vt, const float *qp,
                                 int ldqp, const float *E, int B, int n, int m, float scale, float *out, float *P,
                                 unopose_stream_t stream) {
  UNOPOSE_REQUIRE(q && k && vt && out, "%s: null pointer", name);
  UNOPOSE_REQUIRE((qp == nullptr) == (E == nullptr), "%s: qp and E go together", name);
  UNOPOSE_REQUIRE(B >= 0 && n >= 1 && m >= 1 && m <= TA_MP && B <= 65535, "%s: m=%d exceeds the %d-key tile", name, m, TA_MP);
  UNOPOSE_REQUIRE(ldq >= 256 && ldk >= 256 && ldq % 8 == 0 && ldk % 8 == 0 && (!E || (ldqp >= 1024 && ldqp % 8 == 0)),
                  "%s: row strides must be multiples of 8 elements", name);
  if (B == 0) return UNOPOSE_OK;
  auto *kernel = E ? (P ? token_attn_f32_kernel<true, true> : token_attn_f32_kernel<true, false>)
                   : (P ? token_attn_f32_kernel<false, true> : token_attn_f32_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3(cdiv(n, 16), B), dim3(256), 0, (hipStream_t)stream, q, ldq, k, ldk, vt, qp, ldqp, E, n, m, scale, out, P);
  return check_launch(name);
}

int unopose_token_attention_f32(const float *q, int ldq, const float *k, int ldk, const float *vt, const float *qp,
                                int ldqp, const float *E, int B, int n, int m, float scale, float *out,
                                unopose_stream_t stream) {
  return launch_token_attn_f32("token_attention_f32", q, ldq, k, ldk, vt, qp, ldqp, E, B, n, m, scale, out, nullptr, stream);
}

int unopose_token_attention_f32_train(const float *q, int ldq, const float *k, int ldk, const float *vt, const float *qp, int ldqp,
                                      const float *E, int B, int n, int m, float scale, float *out, float *P, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(P, "token_attention_f32_train: null pointer");
  return launch_token_attn_f32("token_attention_f32_train", q, ldq, k, ldk, vt, qp, ldqp, E, B, n, m, scale, out, P, stream);
}


int unopose_token_attention_f32_backward(const float *dout, const float *q, int ldq, const float *v, int ldv, const float *kt,
                                         const float *qp, int ldqp, const float *E, const float *P, int B, int n, int m, float scale,
                                         float *dS, float *dq, float *dk, float *dv, float *dqp, float *dE, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(dout && q && v && kt && P && dS && dq && dk && dv, "token_attention_f32_backward: null pointer");
  UNOPOSE_REQUIRE((qp == nullptr) == (E == nullptr) && (qp == nullptr) == (dqp == nullptr) && (dE == nullptr || E != nullptr),
                  "token_attention_f32_backward: qp, E and dqp go together (dE only with them)");
  UNOPOSE_REQUIRE(B >= 0 && n >= 1 && m >= 1 && m <= TA_MP && B <= 65535,
                  "token_attention_f32_backward: m=%d exceeds the %d-key tile", m, TA_MP);
  UNOPOSE_REQUIRE(ldq >= 256 && ldv >= 256 && ldq % 8 == 0 && ldv % 8 == 0 && (!qp || (ldqp >= 1024 && ldqp % 8 == 0)),
                  "token_attention_f32_backward: row strides must be multiples of 8 elements");
  if (B == 0) return UNOPOSE_OK;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(token_attn_f32_bwd_dq_kernel, dim3(cdiv(n, 16), B), dim3(256), 0, s, dout, v, ldv, P, kt, n, m, scale, dS, dq);
  int rc = check_launch("token_attention_f32_backward (dq)");
  if (rc != UNOPOSE_OK) return rc;
  hipLaunchKernelGGL(token_attn_f32_bwd_dkv_kernel, dim3(cdiv(m, AB_JT), 4, B), dim3(256), 0, s, q, ldq, dout, P, (const float *)dS, n, m,
                     scale, dk, dv);
  rc = check_launch("token_attention_f32_backward (dk, dv)");
  if (rc != UNOPOSE_OK || !qp) return rc;
  hipLaunchKernelGGL(token_attn_f32_bwd_rpe_kernel, dim3(cdiv(n, 4), B), dim3(256), 0, s, (const float *)dS, qp, ldqp, E, n, m, scale, dqp,
                     dE);
  return check_launch("token_attention_f32_backward (rpe)");
}

int unopose_vit_attention_f32(const float *qkv, int B, int T, int H, float *out, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(qkv && out, "vit_attention_f32: null pointer");
  UNOPOSE_REQUIRE(B >= 0 && T >= 1 && H >= 1 && B <= 65535 && H <= 65535, "vit_attention_f32: bad sizes");
  if (B == 0) return UNOPOSE_OK;
  dim3 grid(cdiv(T, 128), H, B);
  hipLaunchKernelGGL(vit_attn_f32_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, qkv, T, H,
                     0.125f * 1.4426950408889634f, out);
  return check_launch("vit_attention_f32");
}

int unopose_vit_attention_f32_split(const float *qkv, int B, int T, int H, void *out_split, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(qkv && out_split, "vit_attention_f32_split: null pointer");
  UNOPOSE_REQUIRE(B >= 0 && T >= 1 && H >= 1 && B <= 65535 && H <= 65535, "vit_attention_f32_split: bad sizes");
  if (B == 0) return UNOPOSE_OK;
  dim3 grid(cdiv(T, 128), H, B);
  hipLaunchKernelGGL(vit_attn_f32_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, qkv, T, H, 0.125f * 1.4426950408889634f,
                     (float *)out_split);
  return check_launch("vit_attention_f32_split");
}

}  // extern "C"