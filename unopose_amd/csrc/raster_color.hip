// Colour rasteriser for the pose visualisation (C ABI part 3; unopose_amd/vis_poses.py, the toolkit's vis_gt_poses.py / vis_est_poses.py).
// bop_toolkit_lib/visualization.py:93-235 asks its renderer for {"rgb", "depth"} of the object model in each pose; the reference delegates
// that to an OpenGL renderer.  Here, in three passes:
//   keys     a thread per (pose, triangle), as csrc/raster.hip's depth kernel and with its z expression and inside test operation for
//            operation, but the z-buffer entry is the 64-bit key (depth bits << 32) | face index under a 64-bit atomicMin: the nearest
//            face wins a pixel and, at equal depth, the face of the lowest index -- whatever order the threads arrive in;
//   resolve  a thread per (pose, pixel) reads the winner, recomputes its barycentrics with the same expressions and shades the pixel;
//            the depth written is the key's upper half, so it carries the bits unopose_render_depth writes.
// Shading is the toolkit's flat shader restated: the face normal n is the cross product of the camera-space
// edges, the fragment position is Pc = ((x - cx) / fx z, (y - cy) / fy z, z), the light sits at the camera origin and the weight is
// w = min(1, ambient + |n . Pc| / (|n| |Pc|)); |.| because the toolkit's normal comes from screen derivatives and always faces the viewer.
// A face whose |n| |Pc| is not positive takes the cosine 0.  The colour is one surface colour used as is, or per-vertex colours
// interpolated perspective-correctly ((sum b_i / z_i c_i) z); byte = (int)(clamp(w c, 0, 1) 255 + 0.5); background 0.
// tests/raster_rgb_np.py is the same arithmetic in numpy float32; the two agree bit for bit.
#include <algorithm>

#include "common.h"

namespace unopose {

static constexpr unsigned long long RASTER_EMPTY_KEY = 0x7F800000FFFFFFFFull;  // +inf, no face

__global__ __launch_bounds__(256) void raster_key_fill_kernel(unsigned long long *__restrict__ buf, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) buf[i] = RASTER_EMPTY_KEY;
}

__global__ __launch_bounds__(256) void raster_key_kernel(const float *__restrict__ verts, const int *__restrict__ faces, int F,
                                                        const float *__restrict__ Rt, const float *__restrict__ K4, int H, int W,
                                                        unsigned long long *__restrict__ keys) {
  const int f = blockIdx.x * 256 + threadIdx.x, p = blockIdx.y;
  if (f >= F) return;
  const float *R = Rt + (size_t)p * 12, *t = R + 9, *K = K4 + (size_t)p * 4;
  float X[3], Y[3], Z[3], u[3], v[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float *q = verts + (size_t)faces[f * 3 + i] * 3;
    X[i] = R[0] * q[0] + R[1] * q[1] + R[2] * q[2] + t[0];
    Y[i] = R[3] * q[0] + R[4] * q[1] + R[5] * q[2] + t[1];
    Z[i] = R[6] * q[0] + R[7] * q[1] + R[8] * q[2] + t[2];
    if (!(Z[i] > 1e-6f)) return;
    u[i] = K[0] * X[i] / Z[i] + K[2];
    v[i] = K[1] * Y[i] / Z[i] + K[3];
  }
  const float area = (u[1] - u[0]) * (v[2] - v[0]) - (u[2] - u[0]) * (v[1] - v[0]);
  if (fabsf(area) < 1e-12f) return;
  const int x0 = max(0, (int)ceilf(fminf(fminf(u[0], u[1]), u[2]))), x1 = min(W - 1, (int)floorf(fmaxf(fmaxf(u[0], u[1]), u[2])));
  const int y0 = max(0, (int)ceilf(fminf(fminf(v[0], v[1]), v[2]))), y1 = min(H - 1, (int)floorf(fmaxf(fmaxf(v[0], v[1]), v[2])));
  const float inv = 1.f / area, iz0 = 1.f / Z[0], iz1 = 1.f / Z[1], iz2 = 1.f / Z[2];
  unsigned long long *kb = keys + (size_t)p * H * W;
  for (int y = y0; y <= y1; ++y)
    for (int x = x0; x <= x1; ++x) {
      const float px = (float)x, py = (float)y;
      const float b0 = ((u[1] - px) * (v[2] - py) - (u[2] - px) * (v[1] - py)) * inv;
      const float b1 = ((u[2] - px) * (v[0] - py) - (u[0] - px) * (v[2] - py)) * inv;
      const float b2 = 1.f - b0 - b1;
      if (b0 < 0.f || b1 < 0.f || b2 < 0.f) continue;
      const float z = 1.f / (b0 * iz0 + b1 * iz1 + b2 * iz2);
      if (z > 0.f) atomicMin(kb + (size_t)y * W + x, ((unsigned long long)__float_as_uint(z) << 32) | (unsigned long long)(uint32_t)f);
    }
}

__device__ __forceinline__ unsigned char shade_byte(float w, float c) {
  const float s = fminf(fmaxf(w * c, 0.f), 1.f);
  return (unsigned char)(int)(s * 255.f + 0.5f);
}

__global__ __launch_bounds__(256) void raster_resolve_kernel(const float *__restrict__ verts, const int *__restrict__ faces, int F,
                                                            const float *__restrict__ colors, float sr, float sg, float sb, float ambient,
                                                            const float *__restrict__ Rt, const float *__restrict__ K4, int H, int W,
                                                            const unsigned long long *__restrict__ keys, float *__restrict__ depth,
                                                            unsigned char *__restrict__ rgb) {
  const long hw = (long)H * W, i = (long)blockIdx.x * 256 + threadIdx.x;
  const int p = blockIdx.y;
  if (i >= hw) return;
  const size_t at = (size_t)p * hw + i;
  const unsigned long long key = keys[at];
  const uint32_t zbits = (uint32_t)(key >> 32), f = (uint32_t)key;
  unsigned char *o = rgb + at * 3;
  if (zbits >= 0x7F800000u || f >= (uint32_t)F) {  // untouched pixel: depth 0, black
    depth[at] = 0.f;
    o[0] = o[1] = o[2] = 0;
    return;
  }
  depth[at] = __uint_as_float(zbits);
  const float *R = Rt + (size_t)p * 12, *t = R + 9, *K = K4 + (size_t)p * 4;
  int vi[3];
  float X[3], Y[3], Z[3], u[3], v[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    vi[k] = faces[(size_t)f * 3 + k];
    const float *q = verts + (size_t)vi[k] * 3;
    X[k] = R[0] * q[0] + R[1] * q[1] + R[2] * q[2] + t[0];
    Y[k] = R[3] * q[0] + R[4] * q[1] + R[5] * q[2] + t[1];
    Z[k] = R[6] * q[0] + R[7] * q[1] + R[8] * q[2] + t[2];
    u[k] = K[0] * X[k] / Z[k] + K[2];
    v[k] = K[1] * Y[k] / Z[k] + K[3];
  }
  const float area = (u[1] - u[0]) * (v[2] - v[0]) - (u[2] - u[0]) * (v[1] - v[0]);
  const float inv = 1.f / area, iz0 = 1.f / Z[0], iz1 = 1.f / Z[1], iz2 = 1.f / Z[2];
  const int y = (int)(i / W), x = (int)(i - (long)y * W);
  const float px = (float)x, py = (float)y;
  const float b0 = ((u[1] - px) * (v[2] - py) - (u[2] - px) * (v[1] - py)) * inv;
  const float b1 = ((u[2] - px) * (v[0] - py) - (u[0] - px) * (v[2] - py)) * inv;
  const float b2 = 1.f - b0 - b1;
  const float z = 1.f / (b0 * iz0 + b1 * iz1 + b2 * iz2);
  // flat shading: light at the camera origin, the normal of the face from its camera-space edges
  const float e1x = X[1] - X[0], e1y = Y[1] - Y[0], e1z = Z[1] - Z[0];
  const float e2x = X[2] - X[0], e2y = Y[2] - Y[0], e2z = Z[2] - Z[0];
  const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
  const float pcx = (px - K[2]) / K[0] * z, pcy = (py - K[3]) / K[1] * z;
  const float dot = nx * pcx + ny * pcy + nz * z;
  const float len = sqrtf(nx * nx + ny * ny + nz * nz) * sqrtf(pcx * pcx + pcy * pcy + z * z);
  const float cosine = len > 0.f ? fabsf(dot) / len : 0.f;
  const float w = fminf(1.f, ambient + cosine);
  float cr = sr, cg = sg, cb = sb;
  if (colors) {  // perspective-correct: colour / z is linear on the screen
    const float w0 = b0 * iz0, w1 = b1 * iz1, w2 = b2 * iz2;
    const float *c0 = colors + (size_t)vi[0] * 3, *c1 = colors + (size_t)vi[1] * 3, *c2 = colors + (size_t)vi[2] * 3;
    cr = (w0 * c0[0] + w1 * c1[0] + w2 * c2[0]) * z;
    cg = (w0 * c0[1] + w1 * c1[1] + w2 * c2[1]) * z;
    cb = (w0 * c0[2] + w1 * c1[2] + w2 * c2[2]) * z;
  }
  o[0] = shade_byte(w, cr);
  o[1] = shade_byte(w, cg);
  o[2] = shade_byte(w, cb);
}

}  // namespace unopose

using namespace unopose;

extern "C" int unopose_render_color(const float *verts, int V, const int *faces, int F, const float *colors, float surf_r, float surf_g,
                                    float surf_b, float ambient, const float *Rt, const float *K4, int P, int H, int W, void *keys,
                                    float *depth, void *rgb, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(verts && faces && Rt && K4 && keys && depth && rgb, "render_color: null pointer");
  UNOPOSE_REQUIRE(V >= 3 && F >= 1 && P >= 1 && P <= 65535 && H >= 1 && W >= 1, "render_color: bad sizes (V=%d F=%d P=%d H=%d W=%d)", V, F, P, H, W);
  UNOPOSE_REQUIRE((long)H * W <= (1L << 30), "render_color: H * W = %ld (at most 2^30)", (long)H * W);
  UNOPOSE_REQUIRE(((uintptr_t)keys & 7) == 0, "render_color: keys must lie on an 8-byte boundary");
  hipStream_t s = (hipStream_t)stream;
  const long hw = (long)H * W, n = (long)P * hw;
  const int g = (int)std::min<long>((n + 255) / 256, 8192);
  hipLaunchKernelGGL(raster_key_fill_kernel, dim3(g), dim3(256), 0, s, (unsigned long long *)keys, n);
  hipLaunchKernelGGL(raster_key_kernel, dim3(cdiv(F, 256), P), dim3(256), 0, s, verts, faces, F, Rt, K4, H, W, (unsigned long long *)keys);
  hipLaunchKernelGGL(raster_resolve_kernel, dim3(cdiv(hw, 256), P), dim3(256), 0, s, verts, faces, F, colors, surf_r, surf_g, surf_b, ambient,
                     Rt, K4, H, W, (const unsigned long long *)keys, depth, (unsigned char *)rgb);
  return check_launch("render_color");
}
