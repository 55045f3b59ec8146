// Focused linear attention under autograd for gfx950: the core of LinearAttention.forward (core/unopose/model/transformer.py:533-568) in the
// fp32 training step, forward and backward, from the projections' outputs yq (B,N,256), yk / v (B,J,256) and s = 1 / softplus(scale) (256).
// 4 heads x 64, focusing_factor 3.  Every product is an fp32 FMA on the VALU (no split operands: the gradients are held to the bound of an
// fp32 route), every sum over rows is per-workgroup partials added in a fixed order by a second launch: no atomics, the same bits every run.
//
// Layout of all row work: one wavefront per row, lane l owns channels 4 l .. 4 l + 3 (head l / 16).  A workgroup (4 waves) walks its rows
// LA_T at a time; the 64 x 64 matrices of the batch (K and K^T, or dK and dK^T) sit in LDS, a row's head vector is handed to the 16 lanes
// of its head through an LDS row, and each lane contracts it with its four columns of the matrix (float4 LDS reads).  The sums over rows of
// outer products (K = sum_j k_j (x) v_j, dK = sum_n q_n (x) dnum_n) are taken per tile: wave h accumulates head h, 16 x 4 entries per lane.
#include <algorithm>

#include "common.h"

namespace unopose {

constexpr int LA_R = 2;                         // rows per wave and step
constexpr int LA_T = 4 * LA_R;                  // rows per workgroup and step
constexpr int LA_MAT = 4 * 64 * 64;             // one (4,64,64) matrix
constexpr int LA_REC = LA_MAT + 256 + 256;      // a workgroup's partial: matrix | head vector (S or dS) | ds
constexpr int LA_MAX_WG = 64;                   // workgroups (= partials) per batch at most
constexpr int LA_DS_RUNS = 16;                  // contiguous runs the last stage cuts the ds partials into
constexpr int LA_Q_UNIT = 128, LA_K_UNIT = 32;  // rows per workgroup are a multiple of this (query rows / key rows)
// LDS image (floats): M | MT | head vector | s | tile A | tile B
constexpr int LA_M = 0, LA_MT = LA_MAT, LA_VEC = 2 * LA_MAT, LA_SC = LA_VEC + 256, LA_TA = LA_SC + 256, LA_TB = LA_TA + LA_T * 256;
constexpr int LA_LDS_FLOATS = LA_TB + LA_T * 256;
constexpr size_t LA_LDS_BYTES = (size_t)LA_LDS_FLOATS * sizeof(float);

// rows per workgroup and workgroups per batch: functions of the row count alone
static inline int la_wg_rows(int rows, int unit) { return unit * (int)(((long)rows + (long)unit * LA_MAX_WG - 1) / ((long)unit * LA_MAX_WG)); }
static inline int la_wgs(int rows, int unit) { return cdiv(rows, la_wg_rows(rows, unit)); }
static inline long la_ceil_rec(long floats) { return (floats + LA_REC - 1) / LA_REC; }
// records of the backward's workspace: query partials | key-side ds partials (256 floats each) | dK, dK^T, dS per batch
static inline long la_bwd_key_ds_at(int B, int N) { return (long)B * la_wgs(N, LA_Q_UNIT); }
static inline long la_bwd_state_at(int B, int N, int J) { return la_bwd_key_ds_at(B, N) + la_ceil_rec((long)B * la_wgs(J, LA_K_UNIT) * 256); }
static inline long la_bwd_records(int B, int N, int J) { return la_bwd_state_at(B, N, J) + la_ceil_rec((long)B * (2 * LA_MAT + 256)); }
static inline long la_fwd_records(int B, int J) { return (long)B * la_wgs(J, LA_K_UNIT); }

struct LaFocus {
  float q0[4], p[4];  // (relu(y) + 1e-6) s and its cube
  float n1, n3, r;    // |q0|, |p| over the 256 channels, n1 / n3: the focused feature is p r
};

__device__ __forceinline__ void la_focus(const float (&y)[4], const float (&sc)[4], LaFocus &f) {
  float t1 = 0.f, t3 = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    f.q0[e] = (fmaxf(y[e], 0.f) + 1e-6f) * sc[e];
    t1 = __builtin_fmaf(f.q0[e], f.q0[e], t1);
  }
  f.n1 = sqrtf(wave_sum_f32(t1));
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    f.p[e] = f.q0[e] * f.q0[e] * f.q0[e];
    t3 = __builtin_fmaf(f.p[e], f.p[e], t3);
  }
  f.n3 = sqrtf(wave_sum_f32(t3));
  f.r = f.n1 / f.n3;
}

// g = the gradient of the focused row -> dy (exactly 0 where y <= 0); a live row's share of ds is added to dsacc
__device__ __forceinline__ void la_focus_bwd(const float (&y)[4], const float (&sc)[4], const LaFocus &f, const float (&g)[4], bool live,
                                             float (&dy)[4], float (&dsacc)[4]) {
  float t = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) t = __builtin_fmaf(g[e], f.p[e], t);
  const float dr = wave_sum_f32(t);
  const float u = dr / f.n3;  // the gradient of n1
  const float a = u * f.r;    // dr n1 / n3^2: with p / n3 (a unit vector) the n3 term of dp, no n3^3 formed
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float dp = g[e] * f.r - a * (f.p[e] / f.n3);
    const float dq0 = 3.f * (f.q0[e] * f.q0[e]) * dp + u * (f.q0[e] / f.n1);
    dy[e] = y[e] > 0.f ? dq0 * sc[e] : 0.f;
    dsacc[e] = live ? __builtin_fmaf(dq0, fmaxf(y[e], 0.f) + 1e-6f, dsacc[e]) : dsacc[e];  // (a row past the end may focus to 0 / 0)
  }
}

// sum over the 16 lanes of a head; every lane gets it
__device__ __forceinline__ float la_head_sum(float v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 8);
  return v;
}

__device__ __forceinline__ void la_ld4(const float *p, float (&v)[4]) {
  const float4 t = *reinterpret_cast<const float4 *>(p);
  v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
}
__device__ __forceinline__ void la_st4(float *p, const float (&v)[4]) { *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]); }

// acc[i][e] = sum_k rows[i][64 h + k] M[h][k][4 (lane % 16) + e]: rows = the wave's LA_R rows of a tile, M a (4,64,64) matrix in LDS
__device__ __forceinline__ void la_matvec(const float *M, const float *rows, int lane, float (&acc)[LA_R][4]) {
  const int h = lane >> 4;
  const float *Mh = M + h * 4096 + (lane & 15) * 4;
#pragma unroll
  for (int i = 0; i < LA_R; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[i][e] = 0.f;
#pragma unroll 4
  for (int k4 = 0; k4 < 16; ++k4) {
    float m[4][4], x[LA_R][4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) la_ld4(Mh + (k4 * 4 + kk) * 64, m[kk]);
#pragma unroll
    for (int i = 0; i < LA_R; ++i) la_ld4(rows + i * 256 + h * 64 + k4 * 4, x[i]);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
      for (int i = 0; i < LA_R; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[i][e] = __builtin_fmaf(x[i][kk], m[kk][e], acc[i][e]);
  }
}

// acc[i][e] += sum_t A[t][64 h + cb + i] B[t][64 h + d4 + e] over the tile's LA_T rows: h = the wave, cb = 16 (lane / 16), d4 = 4 (lane % 16)
__device__ __forceinline__ void la_outer(const float *TA, const float *TB, int h, int lane, float (&acc)[16][4]) {
  const int cb = (lane >> 4) * 16, d4 = (lane & 15) * 4;
#pragma unroll 2
  for (int t = 0; t < LA_T; ++t) {
    float bv[4], av[4][4];
    la_ld4(TB + t * 256 + h * 64 + d4, bv);
#pragma unroll
    for (int i4 = 0; i4 < 4; ++i4) la_ld4(TA + t * 256 + h * 64 + cb + i4 * 4, av[i4]);
#pragma unroll
    for (int i = 0; i < 16; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[i][e] = __builtin_fmaf(av[i >> 2][i & 3], bv[e], acc[i][e]);
  }
}
__device__ __forceinline__ void la_store_outer(float *rec, int h, int lane, const float (&acc)[16][4]) {
  const int cb = (lane >> 4) * 16, d4 = (lane & 15) * 4;
#pragma unroll
  for (int i = 0; i < 16; ++i) la_st4(rec + h * 4096 + (cb + i) * 64 + d4, acc[i]);
}

// n floats (a multiple of 4, 16-byte aligned) from global memory into LDS
__device__ __forceinline__ void la_stage(float *dst, const float *__restrict__ src, int n) {
  for (int i = threadIdx.x * 4; i < n; i += 256 * 4) *reinterpret_cast<float4 *>(dst + i) = *reinterpret_cast<const float4 *>(src + i);
}

// The lanes' per-channel sums of the four waves, added in wave order through `red` (4 x 256 floats of LDS) into dst[256].  All threads call.
__device__ __forceinline__ void la_wave_reduce(float *red, const float (&acc)[4], float *dst) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  la_st4(red + wave * 256 + lane * 4, acc);
  __syncthreads();
  if (wave == 0) {
    float t[4], u[4];
    la_ld4(red + lane * 4, t);
    for (int w = 1; w < 4; ++w) {
      la_ld4(red + w * 256 + lane * 4, u);
#pragma unroll
      for (int e = 0; e < 4; ++e) t[e] += u[e];
    }
    la_st4(dst + lane * 4, t);
  }
}

// Key state, per workgroup: partial K[h][c][d] = sum_j k_jhc v_jhd and S = sum_j k_j over the workgroup's key rows (k = the focused keys).
__global__ __launch_bounds__(256) void la_key_state_kernel(const float *__restrict__ yk, const float *__restrict__ v, const float *__restrict__ s, int J,
                                                           int wg_rows, float *__restrict__ partials) {
  extern __shared__ __attribute__((aligned(16))) float la_lds[];
  float *TA = la_lds + LA_TA, *TB = la_lds + LA_TB;
  const int b = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r0 = blockIdx.x * wg_rows, r1 = min(J, r0 + wg_rows);
  float sc[4];
  la_ld4(s + lane * 4, sc);
  float acc[16][4], sacc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 16; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[i][e] = 0.f;
  for (int t0 = r0; t0 < r1; t0 += LA_T) {
#pragma unroll
    for (int i = 0; i < LA_R; ++i) {
      const int row = t0 + wave * LA_R + i;
      const bool live = row < r1;
      float y[4] = {0.f, 0.f, 0.f, 0.f}, vv[4] = {0.f, 0.f, 0.f, 0.f}, k[4];
      if (live) {
        la_ld4(yk + ((size_t)b * J + row) * 256 + lane * 4, y);
        la_ld4(v + ((size_t)b * J + row) * 256 + lane * 4, vv);
      }
      LaFocus f;
      la_focus(y, sc, f);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        k[e] = live ? f.p[e] * f.r : 0.f;
        sacc[e] += k[e];
      }
      la_st4(TA + (wave * LA_R + i) * 256 + lane * 4, k);
      la_st4(TB + (wave * LA_R + i) * 256 + lane * 4, vv);
    }
    __syncthreads();
    la_outer(TA, TB, wave, lane, acc);
    __syncthreads();
  }
  float *rec = partials + ((size_t)b * gridDim.x + blockIdx.x) * LA_REC;
  la_store_outer(rec, wave, lane, acc);
  la_wave_reduce(TA, sacc, rec + LA_MAT);
}

// M[b] = sum_g partial matrix, MT[b] = its per-head transpose, vec[b] = sum_g partial head vector; g in order.
__global__ __launch_bounds__(256) void la_reduce_state_kernel(const float *__restrict__ partials, int G, float *__restrict__ M, float *__restrict__ MT,
                                                              float *__restrict__ vec) {
  const int b = blockIdx.y, idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= LA_MAT + 256) return;
  const float *p = partials + (size_t)b * G * LA_REC + idx;
  float t = p[0];
  for (int g = 1; g < G; ++g) t += p[(size_t)g * LA_REC];
  if (idx < LA_MAT) {
    const int h = idx >> 12, c = (idx >> 6) & 63, d = idx & 63;
    M[(size_t)b * LA_MAT + idx] = t;
    MT[(size_t)b * LA_MAT + h * 4096 + d * 64 + c] = t;
  } else {
    vec[(size_t)b * 256 + idx - LA_MAT] = t;
  }
}

// ds = the query partials' ds slots (nq records) plus the key partials (nk rows of 256).  Both lists are cut into LA_DS_RUNS contiguous
// runs; 64 lanes (four channels each) add one run in order -- the loads of eight partials in flight, the additions in order -- and the
// run sums are added in run order.  (One lane per channel over all partials in turn spent 140 us of load latency at 512 + 112 partials.)
__device__ __forceinline__ void la_add_run(float (&acc)[4], const float *__restrict__ p, long n, long stride, int run) {
  const long per = (n + LA_DS_RUNS - 1) / LA_DS_RUNS;
  const long i0 = run * per < n ? run * per : n, i1 = i0 + per < n ? i0 + per : n;
  long i = i0;
  for (; i + 8 <= i1; i += 8) {
    float v[8][4];
#pragma unroll
    for (int k = 0; k < 8; ++k) la_ld4(p + (i + k) * stride, v[k]);
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] += v[k][e];
  }
  for (; i < i1; ++i) {
    float v[4];
    la_ld4(p + i * stride, v);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] += v[e];
  }
}
__global__ __launch_bounds__(64 * LA_DS_RUNS) void la_reduce_ds_kernel(const float *__restrict__ qpart, long nq, const float *__restrict__ kpart, long nk,
                                                                       float *__restrict__ ds) {
  __shared__ __attribute__((aligned(16))) float red[LA_DS_RUNS][256];
  const int lane = threadIdx.x & 63, run = threadIdx.x >> 6;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  la_add_run(acc, qpart + LA_MAT + 256 + lane * 4, nq, LA_REC, run);
  la_add_run(acc, kpart + lane * 4, nk, 256, run);
  la_st4(&red[run][lane * 4], acc);
  __syncthreads();
  if (run > 0) return;
  for (int k = 1; k < LA_DS_RUNS; ++k) {
    float v[4];
    la_ld4(&red[k][lane * 4], v);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] += v[e];
  }
  la_st4(ds + lane * 4, acc);
}

// Forward over the query rows: out_nhd = (sum_c q_nhc K_h[c][d]) / den_nh, den_nh = q_nh . S_h + 1e-6 (kept for the backward).
__global__ __launch_bounds__(256) void la_query_fwd_kernel(const float *__restrict__ yq, const float *__restrict__ s, const float *__restrict__ K,
                                                           const float *__restrict__ S, int N, int wg_rows, float *__restrict__ out,
                                                           float *__restrict__ den) {
  extern __shared__ __attribute__((aligned(16))) float la_lds[];
  float *TA = la_lds + LA_TA;
  const int b = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, h = lane >> 4;
  const int r0 = blockIdx.x * wg_rows, r1 = min(N, r0 + wg_rows);
  la_stage(la_lds + LA_M, K + (size_t)b * LA_MAT, LA_MAT);
  float sc[4], sv[4];
  la_ld4(s + lane * 4, sc);
  la_ld4(S + (size_t)b * 256 + lane * 4, sv);
  __syncthreads();
  for (int t0 = r0; t0 < r1; t0 += LA_T) {
    float dn[LA_R];
#pragma unroll
    for (int i = 0; i < LA_R; ++i) {
      const int row = t0 + wave * LA_R + i;
      float y[4] = {0.f, 0.f, 0.f, 0.f}, q[4];
      if (row < r1) la_ld4(yq + ((size_t)b * N + row) * 256 + lane * 4, y);
      LaFocus f;
      la_focus(y, sc, f);
      float t = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        q[e] = f.p[e] * f.r;
        t = __builtin_fmaf(q[e], sv[e], t);
      }
      dn[i] = la_head_sum(t) + 1e-6f;
      la_st4(TA + (wave * LA_R + i) * 256 + lane * 4, q);
    }
    __syncthreads();
    float num[LA_R][4];
    la_matvec(la_lds + LA_M, TA + wave * LA_R * 256, lane, num);
#pragma unroll
    for (int i = 0; i < LA_R; ++i) {
      const int row = t0 + wave * LA_R + i;
      if (row < r1) {
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = num[i][e] / dn[i];
        la_st4(out + ((size_t)b * N + row) * 256 + lane * 4, o);
        if ((lane & 15) == 0) den[((size_t)b * N + row) * 4 + h] = dn[i];
      }
    }
    __syncthreads();
  }
}

// Backward over the query rows: recomputes q and out, writes dyq, and (KEYS) leaves the workgroup's partial of dK, dS and ds.
template <bool KEYS>
__global__ __launch_bounds__(256) void la_query_bwd_kernel(const float *__restrict__ dout, const float *__restrict__ yq, const float *__restrict__ s,
                                                           const float *__restrict__ K, const float *__restrict__ Kt, const float *__restrict__ S,
                                                           const float *__restrict__ den, int N, int wg_rows, float *__restrict__ dyq,
                                                           float *__restrict__ partials) {
  extern __shared__ __attribute__((aligned(16))) float la_lds[];
  float *TA = la_lds + LA_TA, *TB = la_lds + LA_TB;
  const int b = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, h = lane >> 4;
  const int r0 = blockIdx.x * wg_rows, r1 = min(N, r0 + wg_rows);
  la_stage(la_lds + LA_M, K + (size_t)b * LA_MAT, LA_MAT);
  la_stage(la_lds + LA_MT, Kt + (size_t)b * LA_MAT, LA_MAT);
  float sc[4], sv[4];
  la_ld4(s + lane * 4, sc);
  la_ld4(S + (size_t)b * 256 + lane * 4, sv);
  float acc[16][4], dSacc[4] = {0.f, 0.f, 0.f, 0.f}, dsacc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 16; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[i][e] = 0.f;
  __syncthreads();
  for (int t0 = r0; t0 < r1; t0 += LA_T) {
    float y[LA_R][4], q[LA_R][4];
    LaFocus f[LA_R];
#pragma unroll
    for (int i = 0; i < LA_R; ++i) {
      const int row = t0 + wave * LA_R + i;
      const bool live = row < r1;
#pragma unroll
      for (int e = 0; e < 4; ++e) y[i][e] = 0.f;
      if (live) la_ld4(yq + ((size_t)b * N + row) * 256 + lane * 4, y[i]);
      la_focus(y[i], sc, f[i]);
#pragma unroll
      for (int e = 0; e < 4; ++e) q[i][e] = live ? f[i].p[e] * f[i].r : 0.f;  // rows past the end add nothing to dK and dS
      la_st4(TA + (wave * LA_R + i) * 256 + lane * 4, q[i]);
    }
    __syncthreads();
    float num[LA_R][4], dden[LA_R];
    la_matvec(la_lds + LA_M, TA + wave * LA_R * 256, lane, num);
#pragma unroll
    for (int i = 0; i < LA_R; ++i) {
      const int row = t0 + wave * LA_R + i;
      float d[4] = {0.f, 0.f, 0.f, 0.f}, dnum[4], dn = 1.f;
      if (row < r1) {
        la_ld4(dout + ((size_t)b * N + row) * 256 + lane * 4, d);
        dn = den[((size_t)b * N + row) * 4 + h];
      }
      float t = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        dnum[e] = d[e] / dn;
        t = __builtin_fmaf(d[e], num[i][e] / dn, t);
      }
      dden[i] = -la_head_sum(t) / dn;
      la_st4(TB + (wave * LA_R + i) * 256 + lane * 4, dnum);
    }
    __syncthreads();
    float dq[LA_R][4];
    la_matvec(la_lds + LA_MT, TB + wave * LA_R * 256, lane, dq);
#pragma unroll
    for (int i = 0; i < LA_R; ++i) {
      const int row = t0 + wave * LA_R + i;
      float dy[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        dq[i][e] = __builtin_fmaf(dden[i], sv[e], dq[i][e]);
        dSacc[e] = __builtin_fmaf(q[i][e], dden[i], dSacc[e]);
      }
      la_focus_bwd(y[i], sc, f[i], dq[i], row < r1, dy, dsacc);
      if (row < r1) la_st4(dyq + ((size_t)b * N + row) * 256 + lane * 4, dy);
    }
    if constexpr (KEYS) la_outer(TA, TB, wave, lane, acc);
    __syncthreads();
  }
  if constexpr (!KEYS) return;
  float *rec = partials + ((size_t)b * gridDim.x + blockIdx.x) * LA_REC;
  la_store_outer(rec, wave, lane, acc);
  la_wave_reduce(TA, dSacc, rec + LA_MAT);
  la_wave_reduce(TB, dsacc, rec + LA_MAT + 256);
}

// Backward over the key rows from the reduced dK (and its transpose) and dS: dk = dK v + dS through the focusing -> dyk, dv = k dK, and the
// workgroup's partial of ds.
__global__ __launch_bounds__(256) void la_key_bwd_kernel(const float *__restrict__ yk, const float *__restrict__ v, const float *__restrict__ s,
                                                         const float *__restrict__ dK, const float *__restrict__ dKt, const float *__restrict__ dS, int J,
                                                         int wg_rows, float *__restrict__ dyk, float *__restrict__ dv, float *__restrict__ ds_part) {
  extern __shared__ __attribute__((aligned(16))) float la_lds[];
  float *TA = la_lds + LA_TA, *TB = la_lds + LA_TB;
  const int b = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r0 = blockIdx.x * wg_rows, r1 = min(J, r0 + wg_rows);
  la_stage(la_lds + LA_M, dK + (size_t)b * LA_MAT, LA_MAT);
  la_stage(la_lds + LA_MT, dKt + (size_t)b * LA_MAT, LA_MAT);
  float sc[4], sv[4], dsacc[4] = {0.f, 0.f, 0.f, 0.f};
  la_ld4(s + lane * 4, sc);
  la_ld4(dS + (size_t)b * 256 + lane * 4, sv);
  __syncthreads();
  for (int t0 = r0; t0 < r1; t0 += LA_T) {
    float y[LA_R][4];
    LaFocus f[LA_R];
#pragma unroll
    for (int i = 0; i < LA_R; ++i) {
      const int row = t0 + wave * LA_R + i;
      float vv[4] = {0.f, 0.f, 0.f, 0.f}, k[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) y[i][e] = 0.f;
      if (row < r1) {
        la_ld4(yk + ((size_t)b * J + row) * 256 + lane * 4, y[i]);
        la_ld4(v + ((size_t)b * J + row) * 256 + lane * 4, vv);
      }
      la_focus(y[i], sc, f[i]);
#pragma unroll
      for (int e = 0; e < 4; ++e) k[e] = f[i].p[e] * f[i].r;
      la_st4(TA + (wave * LA_R + i) * 256 + lane * 4, k);
      la_st4(TB + (wave * LA_R + i) * 256 + lane * 4, vv);
    }
    __syncthreads();
    float dk[LA_R][4], dvv[LA_R][4];
    la_matvec(la_lds + LA_MT, TB + wave * LA_R * 256, lane, dk);   // dk_c = sum_d v_d dK[c][d]
    la_matvec(la_lds + LA_M, TA + wave * LA_R * 256, lane, dvv);   // dv_d = sum_c k_c dK[c][d]
#pragma unroll
    for (int i = 0; i < LA_R; ++i) {
      const int row = t0 + wave * LA_R + i;
      const bool live = row < r1;
      float dy[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) dk[i][e] = live ? dk[i][e] + sv[e] : 0.f;  // rows past the end add nothing to ds
      la_focus_bwd(y[i], sc, f[i], dk[i], live, dy, dsacc);
      if (live) {
        la_st4(dyk + ((size_t)b * J + row) * 256 + lane * 4, dy);
        la_st4(dv + ((size_t)b * J + row) * 256 + lane * 4, dvv[i]);
      }
    }
    __syncthreads();
  }
  la_wave_reduce(TA, dsacc, ds_part + ((size_t)b * gridDim.x + blockIdx.x) * 256);
}

}  // namespace unopose

using namespace unopose;

#define LA_LDS_OPTIN(kernel, what)                                                                            \
  do {                                                                                                        \
    static bool done[64];                                                                                     \
    const int rc_ = lds_optin(done, reinterpret_cast<const void *>(kernel), LA_LDS_BYTES, what);              \
    if (rc_ != UNOPOSE_OK) return rc_;                                                                        \
  } while (0)

extern "C" {

int unopose_linear_attention_f32_partial_floats(void) { return LA_REC; }

int unopose_linear_attention_f32_partials(int B, int N, int J) {
  if (B < 0 || B > 65535 || N < 1 || J < 1) return -1;
  const long n = std::max(la_bwd_records(B, N, J), la_fwd_records(B, J));
  return n < (1L << 31) ? (int)n : -1;
}

int unopose_linear_attention_f32_train(const float *yq, const float *yk, const float *v, const float *s, int B, int N, int J, int focus,
                                       float *out, float *K, float *Kt, float *S, float *den, float *partials, int partial_records,
                                       unopose_stream_t stream) {
  UNOPOSE_REQUIRE(yq && yk && v && s && out && K && Kt && S && den && partials, "linear_attention_f32_train: null pointer");
  UNOPOSE_REQUIRE(B >= 0 && B <= 65535 && N >= 1 && J >= 1, "linear_attention_f32_train: bad sizes");
  UNOPOSE_REQUIRE(focus == 3, "linear_attention_f32_train: built for focusing_factor = 3 (got %d)", focus);
  UNOPOSE_REQUIRE(partial_records >= la_fwd_records(B, J), "linear_attention_f32_train: the workspace holds %d partials, %ld needed",
                  partial_records, la_fwd_records(B, J));
  if (B == 0) return UNOPOSE_OK;
  hipStream_t st = (hipStream_t)stream;
  LA_LDS_OPTIN(la_key_state_kernel, "linear_attention_f32_train");
  LA_LDS_OPTIN(la_query_fwd_kernel, "linear_attention_f32_train");
  const int kr = la_wg_rows(J, LA_K_UNIT), kg = la_wgs(J, LA_K_UNIT);
  hipLaunchKernelGGL(la_key_state_kernel, dim3(kg, B), dim3(256), LA_LDS_BYTES, st, yk, v, s, J, kr, partials);
  hipLaunchKernelGGL(la_reduce_state_kernel, dim3(cdiv(LA_MAT + 256, 256), B), dim3(256), 0, st, (const float *)partials, kg, K, Kt, S);
  const int qr = la_wg_rows(N, LA_Q_UNIT), qg = la_wgs(N, LA_Q_UNIT);
  hipLaunchKernelGGL(la_query_fwd_kernel, dim3(qg, B), dim3(256), LA_LDS_BYTES, st, yq, s, (const float *)K, (const float *)S, N, qr, out, den);
  return check_launch("linear_attention_f32_train");
}

int unopose_linear_attention_f32_backward(const float *dout, const float *yq, const float *yk, const float *v, const float *s, const float *K,
                                          const float *Kt, const float *S, const float *den, int B, int N, int J, int focus, float *dyq,
                                          float *dyk, float *dv, float *ds, float *partials, int partial_records, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(dout && yq && yk && v && s && K && Kt && S && den && dyq, "linear_attention_f32_backward: null pointer");
  UNOPOSE_REQUIRE((dyk == nullptr) == (dv == nullptr) && (dyk == nullptr) == (ds == nullptr),
                  "linear_attention_f32_backward: dyk, dv and ds go together");
  UNOPOSE_REQUIRE(B >= 0 && B <= 65535 && N >= 1 && J >= 1, "linear_attention_f32_backward: bad sizes");
  UNOPOSE_REQUIRE(focus == 3, "linear_attention_f32_backward: built for focusing_factor = 3 (got %d)", focus);
  const bool keys = dyk != nullptr;
  UNOPOSE_REQUIRE(!keys || (partials && partial_records >= la_bwd_records(B, N, J)),
                  "linear_attention_f32_backward: the workspace holds %d partials, %ld needed", partial_records, la_bwd_records(B, N, J));
  hipStream_t st = (hipStream_t)stream;
  if (B == 0) {
    if (keys && hipMemsetAsync(ds, 0, 256 * sizeof(float), st) != hipSuccess) return UNOPOSE_ELAUNCH;
    return UNOPOSE_OK;
  }
  const int qr = la_wg_rows(N, LA_Q_UNIT), qg = la_wgs(N, LA_Q_UNIT);
  if (!keys) {
    LA_LDS_OPTIN(la_query_bwd_kernel<false>, "linear_attention_f32_backward");
    hipLaunchKernelGGL(la_query_bwd_kernel<false>, dim3(qg, B), dim3(256), LA_LDS_BYTES, st, dout, yq, s, K, Kt, S, den, N, qr, dyq, partials);
    return check_launch("linear_attention_f32_backward");
  }
  LA_LDS_OPTIN(la_query_bwd_kernel<true>, "linear_attention_f32_backward");
  LA_LDS_OPTIN(la_key_bwd_kernel, "linear_attention_f32_backward");
  const int kr = la_wg_rows(J, LA_K_UNIT), kg = la_wgs(J, LA_K_UNIT);
  float *kds = partials + (size_t)la_bwd_key_ds_at(B, N) * LA_REC;
  float *dK = partials + (size_t)la_bwd_state_at(B, N, J) * LA_REC, *dKt = dK + (size_t)B * LA_MAT, *dS = dKt + (size_t)B * LA_MAT;
  hipLaunchKernelGGL(la_query_bwd_kernel<true>, dim3(qg, B), dim3(256), LA_LDS_BYTES, st, dout, yq, s, K, Kt, S, den, N, qr, dyq, partials);
  hipLaunchKernelGGL(la_reduce_state_kernel, dim3(cdiv(LA_MAT + 256, 256), B), dim3(256), 0, st, (const float *)partials, qg, dK, dKt, dS);
  hipLaunchKernelGGL(la_key_bwd_kernel, dim3(kg, B), dim3(256), LA_LDS_BYTES, st, yk, v, s, (const float *)dK, (const float *)dKt, (const float *)dS, J,
                     kr, dyk, dv, kds);
  hipLaunchKernelGGL(la_reduce_ds_kernel, dim3(1), dim3(64 * LA_DS_RUNS), 0, st, (const float *)partials, (long)B * qg, (const float *)kds, (long)B * kg, ds);
  return check_launch("linear_attention_f32_backward");
}

}  // extern "C"
