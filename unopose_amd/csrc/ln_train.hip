// Residual add + LayerNorm under autograd for gfx950: the post-LN glue of the matcher's layers (core/unopose/model/transformer.py:151-193,
// norm(linear(h) + x)) in the training step.  Forward = the arithmetic of add_layernorm_vec4_kernel (fused.hip) that also keeps the sum and
// the row statistics; backward = one pass over dy and the sum that writes dx and, per slab of rows, one partial of dw / db, plus a small
// second launch that adds the partials.  fp32 arithmetic throughout, no atomics: the results depend on (rows, C) only.
#include <algorithm>

#include "common.h"

namespace unopose {

constexpr int LT_MAX_SLAB = 512;   // rows per slab at most: the lane-serial fp32 sums of dw / db stay short
constexpr int LT_MIN_SLAB = 16;    // 4 rows per wave at least: one (2, C) partial per 16 rows of dy and s read
constexpr int LT_SLABS = 2048;     // slabs aimed at for large inputs (8 workgroups of 4 waves on each of the 256 CUs)
constexpr int LT_SUM_RUNS = 128;   // contiguous runs of slabs the second stage cuts the partials into

// rows per slab: a function of rows (and of nothing that differs between cards or runs)
static inline int lt_slab_rows(long rows) {
  const long per = (rows + LT_SLABS - 1) / LT_SLABS;
  return (int)std::min<long>(LT_MAX_SLAB, std::max<long>(LT_MIN_SLAB, (per + 3) / 4 * 4));
}
static inline long lt_slabs(long rows) {
  const int L = lt_slab_rows(rows);
  return (rows + L - 1) / L;
}

template <bool BF>
__device__ __forceinline__ float4 lt_load4(const void *p, size_t i) {
  if (BF) {
    const uint2 r = *reinterpret_cast<const uint2 *>(reinterpret_cast<const u16 *>(p) + i);
    return make_float4(bf2f((u16)(r.x & 0xFFFF)), bf2f((u16)(r.x >> 16)), bf2f((u16)(r.y & 0xFFFF)), bf2f((u16)(r.y >> 16)));
  }
  return *reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(p) + i);
}

// y[r,:] = LayerNorm(s[r,:]) * w + bias with s = a (+ b); s, mean[r], rstd[r] kept for the backward.  One wavefront per row, four
// contiguous channels per lane and step (NCH steps: C <= 256 NCH).
template <int NCH, bool A_BF16, bool B_BF16, bool HAS_B>
__global__ __launch_bounds__(256) void add_layernorm_train_kernel(const void *__restrict__ a, const void *__restrict__ b,
                                                                  const float *__restrict__ w, const float *__restrict__ bias, long rows, int C,
                                                                  float eps, float *__restrict__ y, float *__restrict__ s,
                                                                  float *__restrict__ mean, float *__restrict__ rstd) {
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int lane = threadIdx.x & 63;
  float4 v[NCH];
  float t = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = (i * 64 + lane) * 4;
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < C) {
      x = lt_load4<A_BF16>(a, (size_t)r * C + c);
      if (HAS_B) {
        const float4 z = lt_load4<B_BF16>(b, (size_t)r * C + c);
        x.x += z.x;
        x.y += z.y;
        x.z += z.z;
        x.w += z.w;
      }
      *reinterpret_cast<float4 *>(s + (size_t)r * C + c) = x;
    }
    v[i] = x;
    t += (x.x + x.y) + (x.z + x.w);
  }
  const float m = wave_sum_f32(t) / (float)C;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    if ((i * 64 + lane) * 4 < C) {
      const float d0 = v[i].x - m, d1 = v[i].y - m, d2 = v[i].z - m, d3 = v[i].w - m;
      q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
    }
  }
  const float rs = rsqrtf(wave_sum_f32(q) / (float)C + eps);
  if (lane == 0) {
    mean[r] = m;
    rstd[r] = rs;
  }
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < C) {
      const float4 wv = *reinterpret_cast<const float4 *>(w + c), bv = *reinterpret_cast<const float4 *>(bias + c);
      *reinterpret_cast<float4 *>(y + (size_t)r * C + c) =
          make_float4((v[i].x - m) * rs * wv.x + bv.x, (v[i].y - m) * rs * wv.y + bv.y, (v[i].z - m) * rs * wv.z + bv.z, (v[i].w - m) * rs * wv.w + bv.w);
    }
  }
}

// Rows [blockIdx.x * slab, + slab) of dx = rstd (g - mean_c(g) - xhat mean_c(g xhat)), g = dy w, xhat = (s - mean) rstd: wave k of the
// workgroup takes rows k, k + 4, ... of the slab.  PARAMS: every lane also adds dy xhat and dy of its own channels over its rows in
// registers; waves 1..3 hand theirs to wave 0 through LDS, which adds them in wave order and writes the slab's (2, C) partial.
template <int NCH, bool PARAMS>
__global__ __launch_bounds__(256) void add_layernorm_bwd_kernel(const float *__restrict__ dy, const float *__restrict__ s, const float *__restrict__ mean,
                                                                const float *__restrict__ rstd, const float *__restrict__ w, long rows, int C, int slab,
                                                                float *__restrict__ dx, float *__restrict__ partials) {
  __shared__ float4 red[PARAMS ? 3 * 2 * NCH * 64 : 1];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long r0 = (long)blockIdx.x * slab, r1 = r0 + slab < rows ? r0 + slab : rows;
  float4 wv[NCH], aw[NCH], ab[NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = (i * 64 + lane) * 4;
    wv[i] = c < C ? *reinterpret_cast<const float4 *>(w + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    aw[i] = ab[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  for (long r = r0 + wave; r < r1; r += 4) {  // the bound is the same for every lane of the wave: the wave sums below see all 64
    const float m = mean[r], rs = rstd[r];
    float4 d[NCH], xh[NCH], g[NCH];
    float sg = 0.f, sgx = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = (i * 64 + lane) * 4;
      d[i] = xh[i] = g[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c < C) {
        d[i] = *reinterpret_cast<const float4 *>(dy + (size_t)r * C + c);
        const float4 x = *reinterpret_cast<const float4 *>(s + (size_t)r * C + c);
        xh[i] = make_float4((x.x - m) * rs, (x.y - m) * rs, (x.z - m) * rs, (x.w - m) * rs);
        g[i] = make_float4(d[i].x * wv[i].x, d[i].y * wv[i].y, d[i].z * wv[i].z, d[i].w * wv[i].w);
        sg += (g[i].x + g[i].y) + (g[i].z + g[i].w);
        sgx += (g[i].x * xh[i].x + g[i].y * xh[i].y) + (g[i].z * xh[i].z + g[i].w * xh[i].w);
      }
    }
    const float mg = wave_sum_f32(sg) / (float)C, mgx = wave_sum_f32(sgx) / (float)C;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = (i * 64 + lane) * 4;
      if (c < C) {
        *reinterpret_cast<float4 *>(dx + (size_t)r * C + c) =
            make_float4(rs * (g[i].x - mg - xh[i].x * mgx), rs * (g[i].y - mg - xh[i].y * mgx), rs * (g[i].z - mg - xh[i].z * mgx),
                        rs * (g[i].w - mg - xh[i].w * mgx));
        if (PARAMS) {
          aw[i].x += d[i].x * xh[i].x;
          aw[i].y += d[i].y * xh[i].y;
          aw[i].z += d[i].z * xh[i].z;
          aw[i].w += d[i].w * xh[i].w;
          ab[i].x += d[i].x;
          ab[i].y += d[i].y;
          ab[i].z += d[i].z;
          ab[i].w += d[i].w;
        }
      }
    }
  }
  if (!PARAMS) return;
  if (wave > 0) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      red[((wave - 1) * 2 * NCH + i) * 64 + lane] = aw[i];
      red[((wave - 1) * 2 * NCH + NCH + i) * 64 + lane] = ab[i];
    }
  }
  __syncthreads();
  if (wave > 0) return;
  float *part = partials + (size_t)blockIdx.x * 2 * C;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < C) {
      float4 tw = aw[i], tb = ab[i];
      for (int k = 0; k < 3; ++k) {
        const float4 pw = red[(k * 2 * NCH + i) * 64 + lane], pb = red[(k * 2 * NCH + NCH + i) * 64 + lane];
        tw = make_float4(tw.x + pw.x, tw.y + pw.y, tw.z + pw.z, tw.w + pw.w);
        tb = make_float4(tb.x + pb.x, tb.y + pb.y, tb.z + pb.z, tb.w + pb.w);
      }
      *reinterpret_cast<float4 *>(part + c) = tw;
      *reinterpret_cast<float4 *>(part + C + c) = tb;
    }
  }
}

// dw | db = the sum of the slabs' (2, C) partials, 32 of the 2 C columns per workgroup.  The slabs are cut into LT_SUM_RUNS contiguous
// runs; eight lanes (four columns each, one 128-byte line per slab) add one run in slab order -- the loads of eight slabs in flight, the
// additions in order -- and the run sums are added in run order.  (One lane per column over runs of 128 slabs, the first form, spent
// 300 us of load latency at 2048 slabs.)
__global__ __launch_bounds__(8 * LT_SUM_RUNS) void add_layernorm_bwd_params_kernel(const float *__restrict__ partials, int nslabs, int C,
                                                                                   float *__restrict__ dw, float *__restrict__ db) {
  __shared__ float4 red[LT_SUM_RUNS][8];
  const int tx = threadIdx.x & 7, run = threadIdx.x >> 3;
  const int col = (blockIdx.x * 8 + tx) * 4;  // this lane's columns col .. col + 3 of the 2 C (a multiple of 4)
  const int per = (nslabs + LT_SUM_RUNS - 1) / LT_SUM_RUNS;
  const int i0 = run * per < nslabs ? run * per : nslabs, i1 = i0 + per < nslabs ? i0 + per : nslabs;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (col < 2 * C) {
    const float *p = partials + col;
    int i = i0;
    for (; i + 8 <= i1; i += 8) {
      float4 v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = *reinterpret_cast<const float4 *>(p + (size_t)(i + k) * 2 * C);
#pragma unroll
      for (int k = 0; k < 8; ++k) acc = make_float4(acc.x + v[k].x, acc.y + v[k].y, acc.z + v[k].z, acc.w + v[k].w);
    }
    for (; i < i1; ++i) {
      const float4 v = *reinterpret_cast<const float4 *>(p + (size_t)i * 2 * C);
      acc = make_float4(acc.x + v.x, acc.y + v.y, acc.z + v.z, acc.w + v.w);
    }
  }
  red[run][tx] = acc;
  __syncthreads();
  const int c = blockIdx.x * 32 + threadIdx.x;
  if (threadIdx.x >= 32 || c >= 2 * C) return;
  const float *lane_red = reinterpret_cast<const float *>(&red[0][0]) + threadIdx.x;  // run k's sum of column c: lane_red[32 k]
  float t = lane_red[0];
#pragma unroll 8
  for (int k = 1; k < LT_SUM_RUNS; ++k) t += lane_red[32 * k];
  if (c < C)
    dw[c] = t;
  else
    db[c - C] = t;
}

}  // namespace unopose

using namespace unopose;

#define LT_REQUIRE_C(what) \
  UNOPOSE_REQUIRE(rows >= 0 && C >= 4 && C % 4 == 0 && C <= 1024, what ": C=%d unsupported (a multiple of 4, 4 <= C <= 1024)", C)

extern "C" {

int unopose_add_layernorm_train(const void *a, int a_bf16, const void *b, int b_bf16, const float *w, const float *bias, long rows, int C,
                                float eps, float *y, float *s, float *mean, float *rstd, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(a && w && bias && y && s && mean && rstd, "add_layernorm_train: null pointer");
  LT_REQUIRE_C("add_layernorm_train");
  UNOPOSE_REQUIRE((rows + 3) / 4 < (1L << 31), "add_layernorm_train: too many rows (%ld)", rows);
  if (rows == 0) return UNOPOSE_OK;
  const dim3 grid((unsigned)((rows + 3) / 4));
  hipStream_t st = (hipStream_t)stream;
#define LT_FWD(NCH, AB, BB, HB) \
  hipLaunchKernelGGL((add_layernorm_train_kernel<NCH, AB, BB, HB>), grid, dim3(256), 0, st, a, b, w, bias, rows, C, eps, y, s, mean, rstd)
#define LT_FWD_C(AB, BB, HB)   \
  do {                         \
    if (C <= 256)              \
      LT_FWD(1, AB, BB, HB);   \
    else if (C <= 512)         \
      LT_FWD(2, AB, BB, HB);   \
    else                       \
      LT_FWD(4, AB, BB, HB);   \
  } while (0)
  switch ((a_bf16 ? 4 : 0) | (b ? (b_bf16 ? 2 : 0) | 1 : 0)) {
    case 0: LT_FWD_C(false, false, false); break;
    case 1: LT_FWD_C(false, false, true); break;
    case 3: LT_FWD_C(false, true, true); break;
    case 4: LT_FWD_C(true, false, false); break;
    case 5: LT_FWD_C(true, false, true); break;
    case 7: LT_FWD_C(true, true, true); break;
    default: UNOPOSE_REQUIRE(false, "add_layernorm_train: bad dtype combination");
  }
#undef LT_FWD_C
#undef LT_FWD
  return check_launch("add_layernorm_train");
}

int unopose_add_layernorm_backward_slabs(long rows, int C) {
  if (rows < 0 || C < 4 || C % 4 != 0 || C > 1024 || lt_slabs(rows) >= (1L << 31)) return -1;
  return (int)lt_slabs(rows);
}

int unopose_add_layernorm_backward(const float *dy, const float *s, const float *mean, const float *rstd, const float *w, long rows, int C,
                                   float *dx, float *dw, float *db, float *partials, int partial_slabs, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(dy && s && mean && rstd && w && dx, "add_layernorm_backward: null pointer");
  UNOPOSE_REQUIRE((dw == nullptr) == (db == nullptr), "add_layernorm_backward: dw and db go together");
  LT_REQUIRE_C("add_layernorm_backward");
  const long nslabs = lt_slabs(rows);
  UNOPOSE_REQUIRE(nslabs < (1L << 31), "add_layernorm_backward: too many rows (%ld)", rows);
  const bool params = dw != nullptr;
  UNOPOSE_REQUIRE(!params || nslabs == 0 || (partials && partial_slabs >= nslabs),
                  "add_layernorm_backward: the partials workspace holds %d slabs, %ld needed", partial_slabs, nslabs);
  hipStream_t st = (hipStream_t)stream;
  const int slab = lt_slab_rows(rows);
  if (nslabs > 0) {
#define LT_BWD(NCH)                                                                                                                      \
  do {                                                                                                                                   \
    if (params)                                                                                                                          \
      hipLaunchKernelGGL((add_layernorm_bwd_kernel<NCH, true>), dim3((unsigned)nslabs), dim3(256), 0, st, dy, s, mean, rstd, w, rows, C, slab, dx, \
                         partials);                                                                                                      \
    else                                                                                                                                 \
      hipLaunchKernelGGL((add_layernorm_bwd_kernel<NCH, false>), dim3((unsigned)nslabs), dim3(256), 0, st, dy, s, mean, rstd, w, rows, C, slab, dx, \
                         partials);                                                                                                      \
  } while (0)
    if (C <= 256)
      LT_BWD(1);
    else if (C <= 512)
      LT_BWD(2);
    else
      LT_BWD(4);
#undef LT_BWD
    const int rc = check_launch("add_layernorm_backward");
    if (rc != UNOPOSE_OK) return rc;
  }
  if (!params) return UNOPOSE_OK;
  hipLaunchKernelGGL(add_layernorm_bwd_params_kernel, dim3((unsigned)cdiv(2 * C, 32)), dim3(8 * LT_SUM_RUNS), 0, st, partials, (int)nslabs, C, dw, db);
  return check_launch("add_layernorm_backward (parameters)");
}

}  // extern "C"
