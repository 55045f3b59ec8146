// The triangle setup and the visibility pass shared by the colour rasterisers (csrc/raster_color.hip, csrc/raster_shade.hip): one
// expression order for the camera-space vertices, their projections, the barycentrics and the perspective-correct depth, and the
// 64-bit key (depth bits << 32) | face index that a 64-bit atomicMin keeps per pixel -- the nearest face wins and, at equal depth,
// the face of the lowest index, whatever order the threads arrive in.  Everything here is inlined into the kernels that use it.
#pragma once
#include "common.h"

namespace unopose {

static constexpr unsigned long long RASTER_EMPTY_KEY = 0x7F800000FFFFFFFFull;  // +inf, no face

// One face in one pose: vertex indices, camera-space vertices and their projections under the intrinsics (fx, fy, cx, cy).
struct RasterFace {
  int vi[3];
  float X[3], Y[3], Z[3], u[3], v[3];
};

__device__ __forceinline__ void raster_face_setup(const float *__restrict__ verts, const int *__restrict__ faces, size_t f, const float *R,
                                                  const float *t, float fx, float fy, float cx, float cy, RasterFace &T) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    T.vi[i] = faces[f * 3 + i];
    const float *q = verts + (size_t)T.vi[i] * 3;
    T.X[i] = R[0] * q[0] + R[1] * q[1] + R[2] * q[2] + t[0];
    T.Y[i] = R[3] * q[0] + R[4] * q[1] + R[5] * q[2] + t[1];
    T.Z[i] = R[6] * q[0] + R[7] * q[1] + R[8] * q[2] + t[2];
    T.u[i] = fx * T.X[i] / T.Z[i] + cx;
    T.v[i] = fy * T.Y[i] / T.Z[i] + cy;
  }
}

__device__ __forceinline__ float raster_face_area(const RasterFace &T) {
  return (T.u[1] - T.u[0]) * (T.v[2] - T.v[0]) - (T.u[2] - T.u[0]) * (T.v[1] - T.v[0]);
}

// barycentrics of the pixel centre (px, py); inv = 1 / raster_face_area
__device__ __forceinline__ void raster_barycentrics(const RasterFace &T, float inv, float px, float py, float &b0, float &b1, float &b2) {
  b0 = ((T.u[1] - px) * (T.v[2] - py) - (T.u[2] - px) * (T.v[1] - py)) * inv;
  b1 = ((T.u[2] - px) * (T.v[0] - py) - (T.u[0] - px) * (T.v[2] - py)) * inv;
  b2 = 1.f - b0 - b1;
}

// The visibility pass for face f of one pose on an H x W grid: kb, the pose's H * W keys, takes the face's key wherever it covers a pixel centre.
// No clipping: a face with a vertex at z <= 1e-6 is dropped, and so is one whose projected area is below 1e-12.
__device__ __forceinline__ void raster_face_keys(const float *__restrict__ verts, const int *__restrict__ faces, int f, const float *R,
                                                 const float *t, float fx, float fy, float cx, float cy, int H, int W,
                                                 unsigned long long *__restrict__ kb) {
  RasterFace T;
  raster_face_setup(verts, faces, (size_t)f, R, t, fx, fy, cx, cy, T);
  if (!(T.Z[0] > 1e-6f) || !(T.Z[1] > 1e-6f) || !(T.Z[2] > 1e-6f)) return;
  const float area = raster_face_area(T);
  if (fabsf(area) < 1e-12f) return;
  const int x0 = max(0, (int)ceilf(fminf(fminf(T.u[0], T.u[1]), T.u[2]))), x1 = min(W - 1, (int)floorf(fmaxf(fmaxf(T.u[0], T.u[1]), T.u[2])));
  const int y0 = max(0, (int)ceilf(fminf(fminf(T.v[0], T.v[1]), T.v[2]))), y1 = min(H - 1, (int)floorf(fmaxf(fmaxf(T.v[0], T.v[1]), T.v[2])));
  const float inv = 1.f / area, iz0 = 1.f / T.Z[0], iz1 = 1.f / T.Z[1], iz2 = 1.f / T.Z[2];
  for (int y = y0; y <= y1; ++y)
    for (int x = x0; x <= x1; ++x) {
      float b0, b1, b2;
      raster_barycentrics(T, inv, (float)x, (float)y, b0, b1, b2);
      if (b0 < 0.f || b1 < 0.f || b2 < 0.f) continue;
      const float z = 1.f / (b0 * iz0 + b1 * iz1 + b2 * iz2);
      if (z > 0.f) atomicMin(kb + (size_t)y * W + x, ((unsigned long long)__float_as_uint(z) << 32) | (unsigned long long)(uint32_t)f);
    }
}

// The flat shading weight of csrc/raster_color.hip: the light at the camera origin, the normal of the face from its camera-space edges,
// the fragment at Pc = ((px - cx) / fx z, (py - cy) / fy z, z); w = min(1, ambient + |n . Pc| / (|n| |Pc|)), the cosine 0 where |n| |Pc| is not positive.
__device__ __forceinline__ float raster_flat_weight(const RasterFace &T, float fx, float fy, float cx, float cy, float px, float py, float z,
                                                    float ambient) {
  const float e1x = T.X[1] - T.X[0], e1y = T.Y[1] - T.Y[0], e1z = T.Z[1] - T.Z[0];
  const float e2x = T.X[2] - T.X[0], e2y = T.Y[2] - T.Y[0], e2z = T.Z[2] - T.Z[0];
  const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
  const float pcx = (px - cx) / fx * z, pcy = (py - cy) / fy * z;
  const float dot = nx * pcx + ny * pcy + nz * z;
  const float len = sqrtf(nx * nx + ny * ny + nz * nz) * sqrtf(pcx * pcx + pcy * pcy + z * z);
  const float cosine = len > 0.f ? fabsf(dot) / len : 0.f;
  return fminf(1.f, ambient + cosine);
}

__device__ __forceinline__ unsigned char shade_byte(float w, float c) {
  const float s = fminf(fmaxf(w * c, 0.f), 1.f);
  return (unsigned char)(int)(s * 255.f + 0.5f);
}

}  // namespace unopose
