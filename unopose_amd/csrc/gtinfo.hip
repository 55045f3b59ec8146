// Ground-truth visibility of a BOP dataset (unopose_amd/gt_info.py with `device=`): what the reference's lib/pysixd/scripts/calc_gt_info.py:97-171
// and third_party/bop_toolkit/scripts/calc_gt_masks.py:92-108 compute per ground truth with numpy, for G ground truths per launch.
// gt_info.gt_counts_host is the specification.
//
// The object is rendered on the toolkit's enlarged canvas (3H x 3W, principal point (cx + W, cy + H)) so that the part of its silhouette
// outside the image is counted; the image is the central H x W crop.  Per ground truth the kernel streams the canvas once and leaves
// GT_INTS integers:
//     px_count_all    canvas pixels with depth > 0
//     px_count_valid  crop pixels with dist_gt > 0 and dist_test > 0
//     px_count_visib  crop pixels with ((float)dist_gt - (float)dist_test <= delta || dist_test == 0) && dist_gt > 0      ("bop19")
//     min x, min y, max x, max y of the silhouette (canvas depth > 0) in image coordinates -- canvas coordinate minus (W, H), so negative
//     values are legitimate --, then the same four of the visible mask
// and, when asked for, the two masks of the crop as uint8 0 / 255 (`dist_gt > 0`, the visible mask).  dist is bopscore.hip's vsd_dist:
// float64, bop_eval.depth_to_dist's evaluation order, so the integers EQUAL numpy's.  A canvas pixel with depth 0 has dist_gt = 0, is in no
// count and no mask, and is dropped before any float64 work and before the test depth is read -- most of the canvas.
//
// The canvas is read as one flat array with 16-byte loads when 9 H W is a multiple of 4 and the map starts on a 16-byte boundary, else 4
// bytes at a time; either way every pixel finds its own row and column, so a vector may straddle a row end or an edge of the crop.  The
// test depth is read only under the silhouette.  Counters and extrema live in registers, are reduced over the wave by shuffles and over
// the block through LDS, and leave the block as integer atomicAdd / atomicMin / atomicMax -- none of which depends on the order.  Four
// crop pixels of a vector that share a mask word are stored as one 32-bit word, the others as bytes.
#include <algorithm>
#include <climits>

#include "common.h"
#include "visib.h"

namespace unopose {

constexpr int GT_INTS = 11;          // 3 counts, 4 extrema of the silhouette, 4 of the visible mask
constexpr int GT_DOUBLES = 5;        // fx, fy, cx, cy, delta
constexpr int GT_INDEX_INTS = 2;     // index of the canvas map, of the test image
constexpr int GT_PIXELS_PER_THREAD = 32;

struct GtAcc {
  int v[GT_INTS];
};

// min for the columns that hold a minimum, max for those that hold a maximum, + for the counts
__device__ __forceinline__ int gt_combine(int k, int a, int b) { return k < 3 ? a + b : ((k - 3) & 2) ? max(a, b) : min(a, b); }
__host__ __device__ __forceinline__ int gt_identity(int k) { return k < 3 ? 0 : ((k - 3) & 2) ? INT_MIN : INT_MAX; }

struct GtView {
  const float *test;  // the ground truth's test image
  double fx, fy, cx, cy, delta;
  int H, W;
};

// One canvas pixel (row y, column x of the 3H x 3W canvas, depth d) into the thread's accumulators -> bit 0: inside the crop, bit 1:
// in the object mask, bit 2: in the visible mask.
__device__ __forceinline__ int gt_pixel(int y, int x, float d, const GtView &g, GtAcc &acc) {
  const int iy = y - g.H, ix = x - g.W;
  const bool crop = iy >= 0 && iy < g.H && ix >= 0 && ix < g.W;
  if (d == 0.f) return crop ? 1 : 0;
  if (d > 0.f) {
    acc.v[0] += 1;
    acc.v[3] = min(acc.v[3], ix), acc.v[4] = min(acc.v[4], iy), acc.v[5] = max(acc.v[5], ix), acc.v[6] = max(acc.v[6], iy);
  }
  if (!crop) return 0;
  const float t = g.test[(size_t)iy * g.W + ix];
  const double pre_x = ((double)ix - g.cx) / g.fx, pre_y = ((double)iy - g.cy) / g.fy;
  const double dg = vsd_dist(pre_x, pre_y, d), dt = vsd_dist(pre_x, pre_y, t);
  const bool obj = dg > 0.0;
  const bool visib = ((double)((float)dg - (float)dt) <= g.delta || dt == 0.0) && obj;
  acc.v[1] += (obj && dt > 0.0) ? 1 : 0;
  if (visib) {
    acc.v[2] += 1;
    acc.v[7] = min(acc.v[7], ix), acc.v[8] = min(acc.v[8], iy), acc.v[9] = max(acc.v[9], ix), acc.v[10] = max(acc.v[10], iy);
  }
  return 1 | (obj ? 2 : 0) | (visib ? 4 : 0);
}

// The pixels of one thread: vectors (or, without `wide`, pixels) first, first + stride, ... of the canvas map `cv` into `acc` and, when
// `mo` / `mv` are given, into the ground truth's two masks.
__device__ __forceinline__ void gt_stream(const float *__restrict__ cv, const GtView &g, int wide, int first, int stride, uint8_t *__restrict__ mo,
                                          uint8_t *__restrict__ mv, GtAcc &acc) {
  const int H = g.H, W = g.W, W3 = 3 * W, N = 9 * H * W;
  if (wide) {  // the map starts on a 16-byte boundary and holds a whole number of vectors: the host checked
    const f32x4 *vc = (const f32x4 *)cv;
    for (int i = first; i < (N >> 2); i += stride) {
      const f32x4 d = vc[i];
      if (!mo && d[0] == 0.f && d[1] == 0.f && d[2] == 0.f && d[3] == 0.f) continue;  // most of the canvas; with masks its crop pixels are still written
      int y = (4 * i) / W3, x = 4 * i - y * W3, bits[4];
      const int y0 = y, x0 = x;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        bits[j] = gt_pixel(y, x, d[j], g, acc);
        if (++x == W3) x = 0, ++y;
      }
      if (mo) {
        const size_t at = (size_t)(y0 - H) * W + (x0 - W);  // of the first pixel; meaningful when that one is in the crop
        // the four pixels lie in one row of the crop (the first and the last do, and the row did not end between them)
        if ((bits[0] & bits[3] & 1) && x0 + 3 < W3 && (((uintptr_t)(mo + at) | (uintptr_t)(mv + at)) & 3) == 0) {
          uint32_t wo = 0, wv = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) wo |= (bits[j] & 2 ? 0xFFu : 0u) << (8 * j), wv |= (bits[j] & 4 ? 0xFFu : 0u) << (8 * j);
          *(uint32_t *)(mo + at) = wo, *(uint32_t *)(mv + at) = wv;
        } else {
          y = y0, x = x0;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (bits[j] & 1) {
              const size_t a = (size_t)(y - H) * W + (x - W);
              mo[a] = bits[j] & 2 ? 255 : 0, mv[a] = bits[j] & 4 ? 255 : 0;
            }
            if (++x == W3) x = 0, ++y;
          }
        }
      }
    }
  } else {
    for (int i = first; i < N; i += stride) {
      const int y = i / W3, x = i - y * W3;
      const int bits = gt_pixel(y, x, cv[i], g, acc);
      if (mo && (bits & 1)) {
        const size_t a = (size_t)(y - H) * W + (x - W);
        mo[a] = bits & 2 ? 255 : 0, mv[a] = bits & 4 ? 255 : 0;
      }
    }
  }
}

__global__ __launch_bounds__(256) void gt_init_kernel(int *__restrict__ out, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = gt_identity(i % GT_INTS);
}

__global__ __launch_bounds__(256) void gt_visibility_kernel(const float *__restrict__ canvas, const float *__restrict__ test,
                                                           const int *__restrict__ index, const double *__restrict__ params, int H, int W,
                                                           int wide, int *__restrict__ out, uint8_t *__restrict__ mask,
                                                           uint8_t *__restrict__ mask_visib) {
  __shared__ int part[4][GT_INTS];
  const int p = blockIdx.y;
  const size_t HW = (size_t)H * W;
  const int *ix = index + (size_t)p * GT_INDEX_INTS;
  const double *q = params + (size_t)p * GT_DOUBLES;
  const GtView g = {test + (size_t)ix[1] * HW, q[0], q[1], q[2], q[3], q[4], H, W};
  GtAcc acc;
#pragma unroll
  for (int k = 0; k < GT_INTS; ++k) acc.v[k] = gt_identity(k);
  gt_stream(canvas + (size_t)ix[0] * 9 * HW, g, wide, blockIdx.x * 256 + threadIdx.x, gridDim.x * 256, mask ? mask + (size_t)p * HW : nullptr,
            mask ? mask_visib + (size_t)p * HW : nullptr, acc);
#pragma unroll
  for (int k = 0; k < GT_INTS; ++k) acc.v[k] = wave_all(acc.v[k], [k](int a, int b) { return gt_combine(k, a, b); });
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < GT_INTS; ++k) part[wave][k] = acc.v[k];
  }
  __syncthreads();
  if (threadIdx.x < GT_INTS) {
    const int k = threadIdx.x;
    const int v = gt_combine(k, gt_combine(k, part[0][k], part[1][k]), gt_combine(k, part[2][k], part[3][k]));
    int *dst = out + (size_t)p * GT_INTS + k;
    if (v != gt_identity(k)) {
      if (k < 3)
        atomicAdd(dst, v);
      else if ((k - 3) & 2)
        atomicMax(dst, v);
      else
        atomicMin(dst, v);
    }
  }
}

}  // namespace unopose

using namespace unopose;

extern "C" {

int unopose_gt_visibility_ints(void) { return GT_INTS; }

int unopose_gt_visibility(const float *canvas, int n_canvas, const float *test, int n_test, const int *index, const double *params, int G,
                          int H, int W, int *out, void *mask, void *mask_visib, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(canvas && test && index && params && out, "gt_visibility: null pointer");
  UNOPOSE_REQUIRE((mask == nullptr) == (mask_visib == nullptr), "gt_visibility: one mask pointer without the other");
  UNOPOSE_REQUIRE(n_canvas >= 1 && n_test >= 1 && G >= 1 && G <= 65535 && H >= 1 && W >= 1 && 9L * H * W <= (1L << 30),
                  "gt_visibility: bad sizes (maps %d / %d, G=%d H=%d W=%d)", n_canvas, n_test, G, H, W);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(gt_init_kernel, dim3(cdiv((long)G * GT_INTS, 256)), dim3(256), 0, s, out, G * GT_INTS);
  const long N = 9L * H * W;
  const int blocks = std::min(std::max(cdiv(N, 256L * GT_PIXELS_PER_THREAD), 1), 512);
  // 16-byte loads need every canvas map on a 16-byte boundary and a whole number of vectors in it; anything else takes the scalar loop
  const int wide = N % 4 == 0 && ((uintptr_t)canvas & 15) == 0;
  hipLaunchKernelGGL(gt_visibility_kernel, dim3(blocks, G), dim3(256), 0, s, canvas, test, index, params, H, W, wide, out, (uint8_t *)mask,
                     (uint8_t *)mask_visib);
  return check_launch("gt_visibility");
}

}  // extern "C"
