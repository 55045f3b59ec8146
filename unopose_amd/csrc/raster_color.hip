// Colour rasteriser for the pose visualisation (C ABI part 3; unopose_amd/vis_poses.py, the toolkit's vis_gt_poses.py / vis_est_poses.py).
// bop_toolkit_lib/visualization.py:93-235 asks its renderer for {"rgb", "depth"} of the object model in each pose; the reference delegates
// that to an OpenGL renderer.  Here, in three passes:
//   keys     a thread per (pose, triangle), as csrc/raster.hip's depth kernel and with its z expression and inside test operation for
//            operation, but the z-buffer entry is the 64-bit key (depth bits << 32) | face index under a 64-bit atomicMin: the nearest
//            face wins a pixel and, at equal depth, the face of the lowest index -- whatever order the threads arrive in;
//   resolve  a thread per (pose, pixel) reads the winner, recomputes its barycentrics with the same expressions and shades the pixel;
//            the depth written is the key's upper half, so it carries the bits unopose_render_depth writes.
// The triangle setup, the key pass and the shading expressions live in csrc/raster_keys.h, which csrc/raster_shade.hip shares.
// Shading is the toolkit's flat shader restated: the face normal n is the cross product of the camera-space
// edges, the fragment position is Pc = ((x - cx) / fx z, (y - cy) / fy z, z), the light sits at the camera origin and the weight is
// w = min(1, ambient + |n . Pc| / (|n| |Pc|)); |.| because the toolkit's normal comes from screen derivatives and always faces the viewer.
// A face whose |n| |Pc| is not positive takes the cosine 0.  The colour is one surface colour used as is, or per-vertex colours
// interpolated perspective-correctly ((sum b_i / z_i c_i) z); byte = (int)(clamp(w c, 0, 1) 255 + 0.5); background 0.
// tests/raster_rgb_np.py is the same arithmetic in numpy float32; the two agree bit for bit.
#include <algorithm>

#include "raster_keys.h"

namespace unopose {

__global__ __launch_bounds__(256) void raster_key_fill_kernel(unsigned long long *__restrict__ buf, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) buf[i] = RASTER_EMPTY_KEY;
}

__global__ __launch_bounds__(256) void raster_key_kernel(const float *__restrict__ verts, const int *__restrict__ faces, int F,
                                                        const float *__restrict__ Rt, const float *__restrict__ K4, int H, int W,
                                                        unsigned long long *__restrict__ keys) {
  const int f = blockIdx.x * 256 + threadIdx.x, p = blockIdx.y;
  if (f >= F) return;
  const float *R = Rt + (size_t)p * 12, *K = K4 + (size_t)p * 4;
  raster_face_keys(verts, faces, f, R, R + 9, K[0], K[1], K[2], K[3], H, W, keys + (size_t)p * H * W);  // csrc/raster_keys.h
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
  const float *R = Rt + (size_t)p * 12, *K = K4 + (size_t)p * 4;
  RasterFace T;
  raster_face_setup(verts, faces, (size_t)f, R, R + 9, K[0], K[1], K[2], K[3], T);
  const float inv = 1.f / raster_face_area(T), iz0 = 1.f / T.Z[0], iz1 = 1.f / T.Z[1], iz2 = 1.f / T.Z[2];
  const int y = (int)(i / W), x = (int)(i - (long)y * W);
  const float px = (float)x, py = (float)y;
  float b0, b1, b2;
  raster_barycentrics(T, inv, px, py, b0, b1, b2);
  const float z = 1.f / (b0 * iz0 + b1 * iz1 + b2 * iz2);
  const float w = raster_flat_weight(T, K[0], K[1], K[2], K[3], px, py, z, ambient);
  float cr = sr, cg = sg, cb = sb;
  if (colors) {  // perspective-correct: colour / z is linear on the screen
    const float w0 = b0 * iz0, w1 = b1 * iz1, w2 = b2 * iz2;
    const float *c0 = colors + (size_t)T.vi[0] * 3, *c1 = colors + (size_t)T.vi[1] * 3, *c2 = colors + (size_t)T.vi[2] * 3;
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
