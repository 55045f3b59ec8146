// Shared helpers for the gfx950 kernels of libunopose_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/unopose_hip.h"

namespace unopose {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16;

// Last error text, readable through unopose_last_error().
void set_error(const char *fmt, ...);

inline int check_launch(const char *what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return UNOPOSE_ELAUNCH;
  }
  return UNOPOSE_OK;
}

#define UNOPOSE_REQUIRE(cond, ...)        \
  do {                                    \
    if (!(cond)) {                        \
      ::unopose::set_error(__VA_ARGS__);  \
      return UNOPOSE_EINVAL;              \
    }                                     \
  } while (0)

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// Opt a kernel into more than 64 KiB of dynamic LDS, once per DEVICE (the attribute belongs to the function on the current device:
// a process that drives several GPUs must set it on each).  `done`: a static bool[64] owned by the call site.
inline int lds_optin(bool (&done)[64], const void *fn, size_t bytes, const char *what) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  if (!done[dev]) {
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) {
      set_error("%s: cannot reserve %zu bytes of LDS", what, bytes);
      return UNOPOSE_ELAUNCH;
    }
    done[dev] = true;
  }
  return UNOPOSE_OK;
}

// Packed RNE fp32 -> bf16 (low half = a, high half = b): lowers to ONE v_cvt_pk_bf16_f32 on gfx950.
// Deliberately the compiler's own vector conversion, not inline asm: the hazard recogniser does not look
// inside asm statements, and an asm VALU op next to an in-flight MFMA on overlapping registers silently
// corrupts results (found with a software-pipelined attention variant; scripts/ubench).
typedef float unopose_f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 unopose_bf16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t cvt_pk_bf16_f32(float a, float b) {
  const unopose_f32x2 v = {a, b};
  union {
    unopose_bf16x2 h;
    uint32_t u;
  } r;
  r.h = __builtin_convertvector(v, unopose_bf16x2);
  return r.u;
}

// Scalar RNE fp32 -> bf16 in software.  Unlike the hardware conversion above it does not keep NaNs: 0x7FFFFFFF becomes -0.
__device__ __forceinline__ u16 f2bf(float f) {
  uint32_t u = __float_as_uint(f);
  u += 0x7FFFu + ((u >> 16) & 1u);
  return (u16)(u >> 16);
}
__device__ __forceinline__ float bf2f(u16 h) { return __uint_as_float(((uint32_t)h) << 16); }

// ---- fp32-class operands on the bf16 matrix cores: x = hi + lo with hi = bf16(x), lo = bf16(x - hi) (x to 2^-17 relative),
// and a product a b ~ ah bh + ah bl + al bh as three bf16 MFMAs with fp32 accumulation (the dropped al bl term is 2^-18 relative).
// The lo pair of (a, b) whose packed hi pair is h = cvt_pk_bf16_f32(a, b).
__device__ __forceinline__ uint32_t cvt_pk_bf16_lo(float a, float b, uint32_t h) {
  return cvt_pk_bf16_f32(a - __uint_as_float(h << 16), b - __uint_as_float(h & 0xFFFF0000u));
}
struct bf16x8_hl {
  bf16x8 hi, lo;
};
__device__ __forceinline__ bf16x8_hl split8_bf16(const float (&v)[8]) {
  union {
    bf16x8 v;
    uint32_t w[4];
  } H, L;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const uint32_t h = cvt_pk_bf16_f32(v[2 * e], v[2 * e + 1]);
    H.w[e] = h;
    L.w[e] = cvt_pk_bf16_lo(v[2 * e], v[2 * e + 1], h);
  }
  return bf16x8_hl{H.v, L.v};
}
// The three products, named by the order they are issued in (hh = a.hi b.hi, hl = a.hi b.lo, lh = a.lo b.hi).  The order
// is part of the result: every kernel keeps the one it was validated with.
__device__ __forceinline__ f32x4 mfma3_hh_hl_lh_16x16(bf16x8_hl a, bf16x8_hl b, f32x4 acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.hi, b.hi, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.hi, b.lo, acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.lo, b.hi, acc, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mfma3_hh_hl_lh_32x32(bf16x8_hl a, bf16x8_hl b, f32x16 acc) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.hi, b.hi, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.hi, b.lo, acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.lo, b.hi, acc, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mfma3_lh_hl_hh_32x32(bf16x8_hl a, bf16x8_hl b, f32x16 acc) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.lo, b.hi, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.hi, b.lo, acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.hi, b.hi, acc, 0, 0, 0);
}

// ---- bilinear tap of a pixel of the (H, W) crop in the (hw, hw) feature map
// torch upsample_bilinear2d, align_corners=False: src = max(0, (dst + 0.5) * in/out - 0.5)  (oneref_feature_extraction.py:229)
struct BilinearTap {
  int y0, x0, y1, x1;
  float ly, lx;
};
__device__ __forceinline__ BilinearTap bilinear_tap(long long pix, int H, int W, int hw) {
  BilinearTap t;
  const int py = (int)(pix / W), px = (int)(pix - (long long)py * W);
  const float sy = fmaxf(((float)py + 0.5f) * ((float)hw / (float)H) - 0.5f, 0.f);
  const float sx = fmaxf(((float)px + 0.5f) * ((float)hw / (float)W) - 0.5f, 0.f);
  t.y0 = min((int)sy, hw - 1);
  t.x0 = min((int)sx, hw - 1);
  t.y1 = t.y0 < hw - 1 ? t.y0 + 1 : t.y0;
  t.x1 = t.x0 < hw - 1 ? t.x0 + 1 : t.x0;
  t.ly = sy - (float)t.y0;
  t.lx = sx - (float)t.x0;
  return t;
}

// ---- wave64 reductions: TWO families, and a kernel keeps the one it was validated with --------------------------------------
//  * DPP row_shr (wave_sum_f32, wave_max_f32, wave_max_u64 below): lane l of a 16-lane row accumulates lanes l-1, l-2, l-4, l-8 in
//    turn, so lane 15 holds the row's result, and the four row results are combined as (r3 + r2) + (r1 + r0) (max: any order).  The
//    result is wave-uniform (scalar registers).  The fp32 forward path uses it; block_sum_256 / block_max_256 extend it to 256 threads
//    as (w0 + w1) + (w2 + w3).
//  * xor butterfly (wave_all and its named forms below): v = op(v, v of lane ^ o) for o = 32, 16, ..., 1.  Both partners of a step
//    compute the same two-operand result, so EVERY lane ends with the same bits: the data-side kernels (scoring, ground truth, dataset
//    preparation, training items, mostly double and int) rely on that to match their host references.
//  For integers, min and max the two agree.  For floating-point sums they add in different orders and differ in the last bits, so
//  moving an existing kernel from one family to the other changes its results; new code picks the butterfly where every lane needs
//  the value or the type is not fp32, the DPP form for an fp32 value wanted once per wave.
//  Neither family, each with an order or a width of its own: row16_max / row16_sum (attn_common.h, 16-lane rows); optim.hip's
//  block_sum_256 (LDS tree over 256 doubles); bn_train.hip's block_sum2 (wave partials added one after the other); the half-wave and
//  sub-wave exchanges (__shfl_xor(., 32) in linattn.hip, attn_f32.hip, gemm_small.hip, fineassign.hip, linear_small_train.hip;
//  la_head_sum; mt_sum4, mt_xor16, mt_xor32; the upward partial butterfly of gemm_kernel.h's LayerNorm epilogue); and the (value, index)
//  arg-reductions of bn_train.hip, match_train.hip, posehead.hip, reftargets.hip and modelinfo.hip's cross-wave tie-break.
// dpp_ctrl: row_shr:n = 0x110+n, row_bcast:15 = 0x142, row_bcast:31 = 0x143.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t v, uint32_t identity) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)identity, (int)v, CTRL, ROW_MASK, 0xF, false);
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_f32(float v, float identity) {
  return __int_as_float(
      __builtin_amdgcn_update_dpp(__float_as_int(identity), __float_as_int(v), CTRL, ROW_MASK, 0xF, false));
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint64_t dpp_u64(uint64_t v) {
  uint32_t lo = dpp_u32<CTRL, ROW_MASK>((uint32_t)v, 0u);
  uint32_t hi = dpp_u32<CTRL, ROW_MASK>((uint32_t)(v >> 32), 0u);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t umax64(uint64_t a, uint64_t b) { return a > b ? a : b; }

// max over the 16 lanes of each DPP row; valid in lane 15 of the row.
__device__ __forceinline__ uint64_t row_max_u64(uint64_t v) {
  v = umax64(v, dpp_u64<0x111, 0xF>(v));
  v = umax64(v, dpp_u64<0x112, 0xF>(v));
  v = umax64(v, dpp_u64<0x114, 0xF>(v));
  v = umax64(v, dpp_u64<0x118, 0xF>(v));
  return v;
}
// max over all 64 lanes; wave-uniform result (read from lane 63).
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
  v = row_max_u64(v);
  uint64_t r[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    r[i] = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 16 * i + 15) << 32) |
           (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 16 * i + 15);
  return umax64(umax64(r[0], r[1]), umax64(r[2], r[3]));
}

__device__ __forceinline__ float wave_sum_f32(float v) {
  v += dpp_f32<0x111, 0xF>(v, 0.f);
  v += dpp_f32<0x112, 0xF>(v, 0.f);
  v += dpp_f32<0x114, 0xF>(v, 0.f);
  v += dpp_f32<0x118, 0xF>(v, 0.f);
  // the four row sums (lane 15 of every 16-lane row) combined in the order the row_bcast chain used: (r3 + r2) + (r1 + r0)
  const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 15)), r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 31));
  const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 47)), r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
  return (r3 + r2) + (r1 + r0);
}
__device__ __forceinline__ float wave_max_f32(float v) {
  const float ninf = -__builtin_inff();
  v = fmaxf(v, dpp_f32<0x111, 0xF>(v, ninf));
  v = fmaxf(v, dpp_f32<0x112, 0xF>(v, ninf));
  v = fmaxf(v, dpp_f32<0x114, 0xF>(v, ninf));
  v = fmaxf(v, dpp_f32<0x118, 0xF>(v, ninf));
  const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 15)), r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 31));
  const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 47)), r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
  return fmaxf(fmaxf(r0, r1), fmaxf(r2, r3));
}

__device__ __forceinline__ int lane_id() {
  return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
}

// Hand-over of LDS data between the lanes of ONE wavefront (a staging buffer no other wave reads): what the lanes wrote before it, every
// lane may read after it.  Release, wave barrier, acquire.
__device__ __forceinline__ void wave_lds_handover() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// sum / max over the 256 threads of a workgroup on the DPP family, `red`: 4 floats of LDS.  The barrier BEFORE the write lets calls
// follow each other on the same `red`; there is none after the read.
__device__ __forceinline__ float block_sum_256(float v, float *red /*[4]*/) {
  v = wave_sum_f32(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ __forceinline__ float block_max_256(float v, float *red) {
  v = wave_max_f32(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// ---- xor butterfly over the 64 lanes: v = op(v, partner's v), partner = lane ^ 32, 16, ..., 1; the result is in every lane, with
// the same bits.  The operand order is part of the contract (an op need not be symmetric).
template <typename T, typename Op>
__device__ __forceinline__ T wave_all(T v, Op op) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
  return v;
}
template <typename T>
__device__ __forceinline__ T wave_all_sum(T v) {
  return wave_all(v, [](T a, T b) { return a + b; });
}
__device__ __forceinline__ int wave_all_min(int v) {
  return wave_all(v, [](int a, int b) { return min(a, b); });
}
__device__ __forceinline__ int wave_all_max(int v) {
  return wave_all(v, [](int a, int b) { return max(a, b); });
}
__device__ __forceinline__ double wave_all_fmin(double v) {
  return wave_all(v, [](double a, double b) { return fmin(a, b); });
}
__device__ __forceinline__ double wave_all_fmax(double v) {
  return wave_all(v, [](double a, double b) { return fmax(a, b); });
}

// inclusive prefix sum over the 64 lanes (Hillis-Steele, __shfl_up by 1, 2, ..., 32); lane 63 holds the wave's total.
template <typename T>
__device__ __forceinline__ T wave_inclusive_sum(T v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

}  // namespace unopose
