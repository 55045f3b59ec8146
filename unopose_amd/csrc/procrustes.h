// The per-point and per-problem steps of weighted Procrustes (model_utils.py:667-743) that geom.hip's three kernels and icp.hip's
// refinement loop share; the 3x3 solve itself is jacobi3.h's kabsch_from_H.
#pragma once
#include "common.h"
#include "jacobi3.h"

namespace unopose {

// H += a b^T (a = centred source point, b = weighted centred reference point)
__device__ __forceinline__ void procrustes_accumulate(float (&h)[9], float a0, float a1, float a2, float b0, float b1, float b2) {
  h[0] += a0 * b0; h[1] += a0 * b1; h[2] += a0 * b2;
  h[3] += a1 * b0; h[4] += a1 * b1; h[5] += a1 * b2;
  h[6] += a2 * b0; h[7] += a2 * b1; h[8] += a2 * b2;
}
// t = c_ref - R c_src (s = c_src, r = c_ref).  (The nine stores of R stay in the kernels: inside this function they reorder the
// instruction streams of the wave and thread kernels.)
__device__ __forceinline__ void procrustes_translation(const float (&R)[9], float s0, float s1, float s2, float r0, float r1, float r2,
                                                       float *to) {
  to[0] = r0 - (R[0] * s0 + R[1] * s1 + R[2] * s2);
  to[1] = r1 - (R[3] * s0 + R[4] * s1 + R[5] * s2);
  to[2] = r2 - (R[6] * s0 + R[7] * s1 + R[8] * s2);
}

}  // namespace unopose
