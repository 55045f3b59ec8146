// The float64 distance of bop_eval.depth_to_dist, shared by the kernels that are held to equality with numpy (bopscore.hip, gtinfo.hip).
#pragma once
#include "common.h"

namespace unopose {

// pre_x = (x - cx) / fx, pre_y = (y - cy) / fy in float64; the build's -ffp-contract=off keeps the sum as written
__device__ __forceinline__ double vsd_dist(double pre_x, double pre_y, float depth) {
  const double d = (double)depth, a = pre_x * d, b = pre_y * d;
  return sqrt(a * a + b * b + d * d);
}

}  // namespace unopose
