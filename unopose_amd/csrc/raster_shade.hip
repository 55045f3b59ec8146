// Shaded, textured, supersampled renders of one object model in P views (C ABI part 3; unopose_amd/render_train.py, the toolkit's
// scripts/render_train_imgs.py, which asks an OpenGL renderer for a Phong-shaded image at ssaa x the resolution and lets cv2 shrink it).
// Two passes over a grid of sH x sW samples per view (s = ssaa, 1 .. 4), of which only the 64-bit keys are ever stored:
//   keys     csrc/raster_keys.h's visibility pass, a thread per (view, triangle), with the intrinsics K s -- the script multiplies the
//            whole matrix, cx and cy included, and so does this (in float32: fx s, fy s, cx s, cy s);
//   resolve  a thread per (view, OUTPUT pixel) walks its s x s samples, shades the covered ones to bytes exactly as csrc/raster_color.hip
//            shades a pixel, adds the bytes up as integers and writes the area mean; the sH x sW colour image never exists.
// Shading of a covered sample, with a_i = b_i / z_i z the perspective-correct weights of the winner's vertices ("Training views of an object model"):
//   phong    N = normalize(sum a_i normalize(R n_i)), L = normalize(sum a_i normalize(-P_i)), P_i the camera-space vertex (the light sits
//            at the camera), w = min(1, ambient + max(0, N . L)); normalize(0) = 0, so a zero normal leaves the ambient term;
//   flat     csrc/raster_color.hip's weight, w = min(1, ambient + |n . Pc| / (|n| |Pc|)).
// Colour c: the texel of (sum a_i uv_i), the interpolated vertex colours, or one surface colour.  The texture rule restates vispy's
// defaults -- nearest, clamp to edge, the image flipped so that v = 0 is its bottom row: column min(max(floor(u Wt), 0), Wt - 1), row
// Ht - 1 - min(max(floor(v Ht), 0), Ht - 1).  PARITY UNPINNED: no OpenGL here to compare the rasterisation and the texture rule with.
// sample byte = (int)(clamp(w c, 0, 1) 255 + 0.5), 0 where nothing projects.
// Output byte = rint((float)(sum of the s^2 sample bytes) * (1.f / s^2)), ties to even: cv2.resize(..., INTER_AREA) for an integer factor
// restated.  PARITY UNPINNED: cv2 is not available to the tests.
// All float32, no contraction; unopose_amd/shade_host.py is the same arithmetic in numpy and the two agree bit for bit (tests/test_render_train_gpu.py).
#include <algorithm>

#include "raster_keys.h"

namespace unopose {

__global__ __launch_bounds__(256) void shade_key_fill_kernel(unsigned long long *__restrict__ buf, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) buf[i] = RASTER_EMPTY_KEY;
}

__global__ __launch_bounds__(256) void shade_key_kernel(const float *__restrict__ verts, const int *__restrict__ faces, int F,
                                                       const float *__restrict__ Rt, const float *__restrict__ K4, float s, int sH, int sW,
                                                       unsigned long long *__restrict__ keys) {
  const int f = blockIdx.x * 256 + threadIdx.x, p = blockIdx.y;
  if (f >= F) return;
  const float *R = Rt + (size_t)p * 12, *K = K4 + (size_t)p * 4;
  raster_face_keys(verts, faces, f, R, R + 9, K[0] * s, K[1] * s, K[2] * s, K[3] * s, sH, sW, keys + (size_t)p * sH * sW);
}

// v / |v|, the zero vector where |v| is not positive
__device__ __forceinline__ void unit3(float x, float y, float z, float &ox, float &oy, float &oz) {
  const float len = sqrtf(x * x + y * y + z * z);
  const bool ok = len > 0.f;
  ox = ok ? x / len : 0.f;
  oy = ok ? y / len : 0.f;
  oz = ok ? z / len : 0.f;
}

struct ShadeModel {
  const float *verts;
  const int *faces;
  const float *normals;  // (V,3), read when phong
  const float *colors;   // (V,3) or null
  const float *uv;       // (V,2), read when texture
  const float *texture;  // (Ht,Wt,3) in [0,1] or null
  int F, Ht, Wt;
  float sr, sg, sb, ambient;
  int phong;
};

__global__ __launch_bounds__(256) void shade_resolve_kernel(ShadeModel m, const float *__restrict__ Rt, const float *__restrict__ K4, int ssaa,
                                                           int H, int W, const unsigned long long *__restrict__ keys,
                                                           unsigned char *__restrict__ rgb) {
  const long hw = (long)H * W, i = (long)blockIdx.x * 256 + threadIdx.x;
  const int p = blockIdx.y;
  if (i >= hw) return;
  const int oy = (int)(i / W), ox = (int)(i - (long)oy * W);
  const int sH = H * ssaa, sW = W * ssaa;
  const float s = (float)ssaa;
  const float *R = Rt + (size_t)p * 12, *K = K4 + (size_t)p * 4;
  const float fx = K[0] * s, fy = K[1] * s, cx = K[2] * s, cy = K[3] * s;
  const unsigned long long *kb = keys + (size_t)p * sH * sW;
  // the winner of the previous sample: neighbouring samples mostly share it, and everything below depends on the face and the view only
  uint32_t held = 0xFFFFFFFFu;
  RasterFace T;
  float inv = 0.f, iz0 = 0.f, iz1 = 0.f, iz2 = 0.f;
  float nh[3][3], lh[3][3];
  int sum_r = 0, sum_g = 0, sum_b = 0;
  for (int sy = 0; sy < ssaa; ++sy)
    for (int sx = 0; sx < ssaa; ++sx) {
      const int y = oy * ssaa + sy, x = ox * ssaa + sx;
      const unsigned long long key = kb[(size_t)y * sW + x];
      const uint32_t zbits = (uint32_t)(key >> 32), f = (uint32_t)key;
      if (zbits >= 0x7F800000u || f >= (uint32_t)m.F) continue;  // uncovered sample: 0
      if (f != held) {
        held = f;
        raster_face_setup(m.verts, m.faces, (size_t)f, R, R + 9, fx, fy, cx, cy, T);
        inv = 1.f / raster_face_area(T);
        iz0 = 1.f / T.Z[0];
        iz1 = 1.f / T.Z[1];
        iz2 = 1.f / T.Z[2];
        if (m.phong) {
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const float *n = m.normals + (size_t)T.vi[k] * 3;
            unit3(R[0] * n[0] + R[1] * n[1] + R[2] * n[2], R[3] * n[0] + R[4] * n[1] + R[5] * n[2], R[6] * n[0] + R[7] * n[1] + R[8] * n[2],
                  nh[k][0], nh[k][1], nh[k][2]);
            unit3(-T.X[k], -T.Y[k], -T.Z[k], lh[k][0], lh[k][1], lh[k][2]);
          }
        }
      }
      const float px = (float)x, py = (float)y;
      float b0, b1, b2;
      raster_barycentrics(T, inv, px, py, b0, b1, b2);
      const float z = 1.f / (b0 * iz0 + b1 * iz1 + b2 * iz2);
      const float w0 = b0 * iz0, w1 = b1 * iz1, w2 = b2 * iz2;
      float w;
      if (m.phong) {
        const float a0 = w0 * z, a1 = w1 * z, a2 = w2 * z;
        float Nx, Ny, Nz, Lx, Ly, Lz;
        unit3(a0 * nh[0][0] + a1 * nh[1][0] + a2 * nh[2][0], a0 * nh[0][1] + a1 * nh[1][1] + a2 * nh[2][1],
              a0 * nh[0][2] + a1 * nh[1][2] + a2 * nh[2][2], Nx, Ny, Nz);
        unit3(a0 * lh[0][0] + a1 * lh[1][0] + a2 * lh[2][0], a0 * lh[0][1] + a1 * lh[1][1] + a2 * lh[2][1],
              a0 * lh[0][2] + a1 * lh[1][2] + a2 * lh[2][2], Lx, Ly, Lz);
        w = fminf(1.f, m.ambient + fmaxf(0.f, Nx * Lx + Ny * Ly + Nz * Lz));
      } else {
        w = raster_flat_weight(T, fx, fy, cx, cy, px, py, z, m.ambient);
      }
      float cr = m.sr, cg = m.sg, cb = m.sb;
      if (m.texture) {
        const float *t0 = m.uv + (size_t)T.vi[0] * 2, *t1 = m.uv + (size_t)T.vi[1] * 2, *t2 = m.uv + (size_t)T.vi[2] * 2;
        const float tu = (w0 * t0[0] + w1 * t1[0] + w2 * t2[0]) * z, tv = (w0 * t0[1] + w1 * t1[1] + w2 * t2[1]) * z;
        // clamped as floats, so that no value, however large, reaches the conversion: the index stays inside the image
        const int col = (int)fminf(fmaxf(floorf(tu * (float)m.Wt), 0.f), (float)(m.Wt - 1));
        const int row = m.Ht - 1 - (int)fminf(fmaxf(floorf(tv * (float)m.Ht), 0.f), (float)(m.Ht - 1));
        const float *texel = m.texture + ((size_t)row * m.Wt + col) * 3;
        cr = texel[0];
        cg = texel[1];
        cb = texel[2];
      } else if (m.colors) {  // perspective-correct: colour / z is linear on the screen
        const float *c0 = m.colors + (size_t)T.vi[0] * 3, *c1 = m.colors + (size_t)T.vi[1] * 3, *c2 = m.colors + (size_t)T.vi[2] * 3;
        cr = (w0 * c0[0] + w1 * c1[0] + w2 * c2[0]) * z;
        cg = (w0 * c0[1] + w1 * c1[1] + w2 * c2[1]) * z;
        cb = (w0 * c0[2] + w1 * c1[2] + w2 * c2[2]) * z;
      }
      sum_r += shade_byte(w, cr);
      sum_g += shade_byte(w, cg);
      sum_b += shade_byte(w, cb);
    }
  const float area = 1.f / (float)(ssaa * ssaa);
  unsigned char *o = rgb + ((size_t)p * hw + i) * 3;
  o[0] = (unsigned char)(int)rintf((float)sum_r * area);
  o[1] = (unsigned char)(int)rintf((float)sum_g * area);
  o[2] = (unsigned char)(int)rintf((float)sum_b * area);
}

}  // namespace unopose

using namespace unopose;

extern "C" int unopose_render_shaded(const float *verts, int V, const int *faces, int F, const float *normals, const float *colors,
                                     const float *uv, const float *texture, int Ht, int Wt, float surf_r, float surf_g, float surf_b,
                                     float ambient, int phong, int ssaa, const float *Rt, const float *K4, int P, int H, int W, void *keys,
                                     void *rgb, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(verts && faces && Rt && K4 && keys && rgb, "render_shaded: null pointer");
  UNOPOSE_REQUIRE(V >= 3 && F >= 1 && P >= 1 && P <= 65535 && H >= 1 && W >= 1, "render_shaded: bad sizes (V=%d F=%d P=%d H=%d W=%d)", V, F, P, H, W);
  UNOPOSE_REQUIRE(ssaa >= 1 && ssaa <= 4, "render_shaded: ssaa = %d (1 to 4)", ssaa);
  UNOPOSE_REQUIRE((long)H * ssaa * W * ssaa <= (1L << 30), "render_shaded: ssaa^2 * H * W = %ld (at most 2^30)", (long)H * ssaa * W * ssaa);
  UNOPOSE_REQUIRE(!phong || normals, "render_shaded: phong shading needs normals");
  UNOPOSE_REQUIRE(!texture || (uv && Ht >= 1 && Wt >= 1 && Ht <= (1 << 20) && Wt <= (1 << 20)), "render_shaded: a texture needs uv and a size of 1 .. 2^20 (Ht=%d Wt=%d)", Ht, Wt);
  UNOPOSE_REQUIRE(!(texture && colors), "render_shaded: texture or colors, not both");
  UNOPOSE_REQUIRE(((uintptr_t)keys & 7) == 0, "render_shaded: keys must lie on an 8-byte boundary");
  hipStream_t st = (hipStream_t)stream;
  const int sH = H * ssaa, sW = W * ssaa;
  const long hw = (long)H * W, n = (long)P * sH * sW;
  const int g = (int)std::min<long>((n + 255) / 256, 8192);
  ShadeModel m{verts, faces, normals, colors, uv, texture, F, Ht, Wt, surf_r, surf_g, surf_b, ambient, phong ? 1 : 0};
  hipLaunchKernelGGL(shade_key_fill_kernel, dim3(g), dim3(256), 0, st, (unsigned long long *)keys, n);
  hipLaunchKernelGGL(shade_key_kernel, dim3(cdiv(F, 256), P), dim3(256), 0, st, verts, faces, F, Rt, K4, (float)ssaa, sH, sW,
                     (unsigned long long *)keys);
  hipLaunchKernelGGL(shade_resolve_kernel, dim3(cdiv(hw, 256), P), dim3(256), 0, st, m, Rt, K4, ssaa, H, W, (const unsigned long long *)keys,
                     (unsigned char *)rgb);
  return check_launch("render_shaded");
}
