// Per-image composition of the pose visualisation (C ABI part 3; unopose_amd/ops/vis.py): bop_toolkit_lib/visualization.py:93-235
// `vis_object_poses` restated for renders that are already on the device (csrc/raster_color.hip), every cast and evaluation order kept.
//   boxes     misc.calc_2d_bbox of the pixels of each pose where ANY colour channel is > 0 (visualization.py:178-187: not the depth mask);
//   compose   a thread per pixel walks the poses in order: the rendered layer takes the colour of the nearest pose, the earliest at
//             equal depth (`m_depth < ren_depth`, :163-171), or without resolve_visib the saturating sum of all renders (:173-175); the
//             info layer holds the 1-pixel outline of every box, both corners inclusive as ImageDraw.rectangle draws it, value
//             int(0.3 * 255) = 76 (:16-36, :183); blend = 0.5 photo + 0.5 ren + info in float32, above 255 -> 255, truncated (:201-205);
//   depth difference (:211-227): valid = depth > 0 and ren_depth > 0, diff = valid * (ren_depth - depth), red = 255 where valid and
//             diff < delta, green = blue = 255 * depth_for_vis(diff - min(diff)) truncated, where depth_for_vis (:77-90) works in float64
//             on the pixels with a positive value: (v - min) / (range / 0.8) + 0.2; invalid pixels 0.  Three reduction passes feed it: the
//             image-wide minimum of diff (the zeros of invalid pixels included), then minimum and maximum over the positive shifted values.
// Where the toolkit is undefined: without a valid pixel the image is 0 and there are no statistics; with no positive shifted value, or
// with all of them equal (range 0), green = blue = 51 (= 255 * 0.2) at every valid pixel.
#include <limits.h>

#include "common.h"

namespace unopose {

static constexpr int VIS_WORKSPACE_INTS = 8;  // 0 min diff, 1 min valid diff, 2 max valid diff, 3 valid pixels, 4 min shifted, 5 max shifted, 6-7 sum (double)

// float <-> unsigned key with the same order (for integer atomicMin / atomicMax)
__device__ __forceinline__ uint32_t f2key(float f) {
  const uint32_t b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

__global__ __launch_bounds__(256) void vis_box_init_kernel(int *__restrict__ boxes, int P) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  boxes[p * 4 + 0] = INT_MAX;
  boxes[p * 4 + 1] = INT_MAX;
  boxes[p * 4 + 2] = INT_MIN;
  boxes[p * 4 + 3] = INT_MIN;
}

__global__ __launch_bounds__(256) void vis_box_kernel(const unsigned char *__restrict__ rgbs, int H, int W, int *__restrict__ boxes) {
  __shared__ int box[4];
  const long hw = (long)H * W, i = (long)blockIdx.x * 256 + threadIdx.x;
  const int p = blockIdx.y;
  if (threadIdx.x == 0) {
    box[0] = box[1] = INT_MAX;
    box[2] = box[3] = INT_MIN;
  }
  __syncthreads();
  if (i < hw) {
    const unsigned char *c = rgbs + ((size_t)p * hw + i) * 3;
    if (c[0] > 0 || c[1] > 0 || c[2] > 0) {
      const int y = (int)(i / W), x = (int)(i - (long)y * W);
      atomicMin(&box[0], x);
      atomicMin(&box[1], y);
      atomicMax(&box[2], x);
      atomicMax(&box[3], y);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && box[2] >= 0) {
    atomicMin(boxes + p * 4 + 0, box[0]);
    atomicMin(boxes + p * 4 + 1, box[1]);
    atomicMax(boxes + p * 4 + 2, box[2]);
    atomicMax(boxes + p * 4 + 3, box[3]);
  }
}

__global__ __launch_bounds__(256) void vis_compose_kernel(const unsigned char *__restrict__ rgbs, const float *__restrict__ depths, int P, int H,
                                                         int W, const unsigned char *__restrict__ photo, int resolve_visib,
                                                         const int *__restrict__ boxes, unsigned char *__restrict__ ren_rgb,
                                                         float *__restrict__ ren_depth, unsigned char *__restrict__ vis_rgb) {
  const long hw = (long)H * W, i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  const int y = (int)(i / W), x = (int)(i - (long)y * W);
  float rd = 0.f;
  unsigned char ren[3] = {0, 0, 0};
  bool outline = false;
  for (int p = 0; p < P; ++p) {
    const float m = depths[(size_t)p * hw + i];
    const unsigned char *c = rgbs + ((size_t)p * hw + i) * 3;
    const bool take = m != 0.f && (rd == 0.f || m < rd);
    if (take) rd = m;
    if (resolve_visib) {
      if (take) {
        ren[0] = c[0];
        ren[1] = c[1];
        ren[2] = c[2];
      }
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        float s = (float)ren[k] + (float)c[k];
        if (s > 255.f) s = 255.f;
        ren[k] = (unsigned char)s;
      }
    }
    const int bx0 = boxes[p * 4 + 0], by0 = boxes[p * 4 + 1], bx1 = boxes[p * 4 + 2], by1 = boxes[p * 4 + 3];
    if (bx1 >= bx0 && x >= bx0 && x <= bx1 && y >= by0 && y <= by1 && (x == bx0 || x == bx1 || y == by0 || y == by1)) outline = true;
  }
  ren_depth[i] = rd;
  const float info = outline ? 76.f : 0.f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    ren_rgb[i * 3 + k] = ren[k];
    float b = 0.5f * (float)photo[i * 3 + k] + 0.5f * (float)ren[k] + 1.0f * info;
    if (b > 255.f) b = 255.f;
    vis_rgb[i * 3 + k] = (unsigned char)b;
  }
}

__global__ void vis_diff_init_kernel(uint32_t *__restrict__ ws) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  ws[0] = ws[1] = ws[4] = 0xFFFFFFFFu;
  ws[2] = ws[5] = 0u;
  ws[3] = 0u;
  ws[6] = ws[7] = 0u;
}

__device__ __forceinline__ float vis_diff_at(const float *__restrict__ ren_depth, const float *__restrict__ depth, long i, bool &valid) {
  const float d = depth[i], r = ren_depth[i];
  valid = (d > 0.f) && (r > 0.f);
  return (valid ? 1.f : 0.f) * (r - d);
}

// pass 1: minimum of diff over the image; minimum, maximum, sum and count over the valid pixels
__global__ __launch_bounds__(256) void vis_diff_reduce1_kernel(const float *__restrict__ ren_depth, const float *__restrict__ depth, long hw,
                                                              uint32_t *__restrict__ ws) {
  __shared__ uint32_t s_min, s_vmin, s_vmax, s_cnt;
  __shared__ double s_sum[256];
  if (threadIdx.x == 0) {
    s_min = s_vmin = 0xFFFFFFFFu;
    s_vmax = 0u;
    s_cnt = 0u;
  }
  __syncthreads();
  double sum = 0.0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < hw; i += (long)gridDim.x * 256) {
    bool valid;
    const float diff = vis_diff_at(ren_depth, depth, i, valid);
    const uint32_t k = f2key(diff);
    atomicMin(&s_min, k);
    if (valid) {
      atomicMin(&s_vmin, k);
      atomicMax(&s_vmax, k);
      atomicAdd(&s_cnt, 1u);
      sum += (double)diff;
    }
  }
  s_sum[threadIdx.x] = sum;
  __syncthreads();
  for (int step = 128; step > 0; step >>= 1) {
    if ((int)threadIdx.x < step) s_sum[threadIdx.x] += s_sum[threadIdx.x + step];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    atomicMin(ws + 0, s_min);
    if (s_cnt) {
      atomicMin(ws + 1, s_vmin);
      atomicMax(ws + 2, s_vmax);
      atomicAdd(ws + 3, s_cnt);
      atomicAdd((double *)(ws + 6), s_sum[0]);
    }
  }
}

// pass 2: minimum and maximum of the positive shifted values (diff - min diff), over every pixel as the toolkit's mask is
__global__ __launch_bounds__(256) void vis_diff_reduce2_kernel(const float *__restrict__ ren_depth, const float *__restrict__ depth, long hw,
                                                              uint32_t *__restrict__ ws) {
  __shared__ uint32_t s_min, s_max;
  if (threadIdx.x == 0) {
    s_min = 0xFFFFFFFFu;
    s_max = 0u;
  }
  __syncthreads();
  const float dmin = key2f(ws[0]);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < hw; i += (long)gridDim.x * 256) {
    bool valid;
    const float shifted = vis_diff_at(ren_depth, depth, i, valid) - dmin;
    if (shifted > 0.f) {
      atomicMin(&s_min, f2key(shifted));
      atomicMax(&s_max, f2key(shifted));
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_max != 0u) {
    atomicMin(ws + 4, s_min);
    atomicMax(ws + 5, s_max);
  }
}

__global__ __launch_bounds__(256) void vis_diff_image_kernel(const float *__restrict__ ren_depth, const float *__restrict__ depth, long hw,
                                                            float delta, const uint32_t *__restrict__ ws, unsigned char *__restrict__ image,
                                                            double *__restrict__ stats) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const uint32_t count = ws[3];
  if (i == 0) {  // minimum, maximum, mean of diff over the valid pixels, their number
    const double sum = *(const double *)(ws + 6);
    stats[0] = count ? (double)key2f(ws[1]) : 0.0;
    stats[1] = count ? (double)key2f(ws[2]) : 0.0;
    stats[2] = count ? sum / (double)count : 0.0;
    stats[3] = (double)count;
  }
  if (i >= hw) return;
  bool valid;
  const float diff = vis_diff_at(ren_depth, depth, i, valid);
  unsigned char r = 0, g = 0;
  if (valid) {
    r = diff < delta ? 255 : 0;
    const float shifted = diff - key2f(ws[0]);
    const bool any = ws[5] != 0u;
    const double lo = any ? (double)key2f(ws[4]) : 0.0, range = any ? (double)key2f(ws[5]) - lo : 0.0;
    if (!(range > 0.0)) {
      g = 51;  // the toolkit divides by zero or takes the minimum of nothing here: 255 * valid_start
    } else if (shifted > 0.f) {
      double v = (double)shifted;
      v -= lo;
      v /= range / (1.0 - 0.2);
      v += 0.2;
      g = (unsigned char)(255.0 * v);
    }
  }
  image[i * 3 + 0] = r;
  image[i * 3 + 1] = g;
  image[i * 3 + 2] = g;
}

}  // namespace unopose

using namespace unopose;

extern "C" int unopose_vis_workspace_ints(void) { return VIS_WORKSPACE_INTS; }

extern "C" int unopose_vis_compose(const void *rgbs, const float *depths, int P, int H, int W, const void *photo, int resolve_visib, int *boxes,
                                   void *ren_rgb, float *ren_depth, void *vis_rgb, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(rgbs && depths && photo && boxes && ren_rgb && ren_depth && vis_rgb, "vis_compose: null pointer");
  UNOPOSE_REQUIRE(P >= 1 && P <= 65535 && H >= 1 && W >= 1 && (long)H * W <= (1L << 30), "vis_compose: bad sizes (P=%d H=%d W=%d)", P, H, W);
  hipStream_t s = (hipStream_t)stream;
  const long hw = (long)H * W;
  hipLaunchKernelGGL(vis_box_init_kernel, dim3(cdiv(P, 256)), dim3(256), 0, s, boxes, P);
  hipLaunchKernelGGL(vis_box_kernel, dim3(cdiv(hw, 256), P), dim3(256), 0, s, (const unsigned char *)rgbs, H, W, boxes);
  hipLaunchKernelGGL(vis_compose_kernel, dim3(cdiv(hw, 256)), dim3(256), 0, s, (const unsigned char *)rgbs, depths, P, H, W,
                     (const unsigned char *)photo, resolve_visib, boxes, (unsigned char *)ren_rgb, ren_depth, (unsigned char *)vis_rgb);
  return check_launch("vis_compose");
}

extern "C" int unopose_vis_depth_diff(const float *ren_depth, const float *depth, int H, int W, float delta, void *workspace, void *image,
                                      double *stats, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(ren_depth && depth && workspace && image && stats, "vis_depth_diff: null pointer");
  UNOPOSE_REQUIRE(H >= 1 && W >= 1 && (long)H * W <= (1L << 30), "vis_depth_diff: bad sizes (H=%d W=%d)", H, W);
  UNOPOSE_REQUIRE(((uintptr_t)workspace & 7) == 0, "vis_depth_diff: workspace must lie on an 8-byte boundary");
  hipStream_t s = (hipStream_t)stream;
  const long hw = (long)H * W;
  const int g = (int)(cdiv(hw, 256) < 1024 ? cdiv(hw, 256) : 1024);
  uint32_t *ws = (uint32_t *)workspace;
  hipLaunchKernelGGL(vis_diff_init_kernel, dim3(1), dim3(64), 0, s, ws);
  hipLaunchKernelGGL(vis_diff_reduce1_kernel, dim3(g), dim3(256), 0, s, ren_depth, depth, hw, ws);
  hipLaunchKernelGGL(vis_diff_reduce2_kernel, dim3(g), dim3(256), 0, s, ren_depth, depth, hw, ws);
  hipLaunchKernelGGL(vis_diff_image_kernel, dim3(cdiv(hw, 256)), dim3(256), 0, s, ren_depth, depth, hw, delta, (const uint32_t *)ws,
                     (unsigned char *)image, stats);
  return check_launch("vis_depth_diff");
}
