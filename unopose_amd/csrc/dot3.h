// The 3 x 3 float64 product element that the host specification fixes (bop_eval._dot3), shared by posemetrics.hip and reftargets.hip.
#pragma once
#include "common.h"

namespace unopose {

// One element of a 3 x 3 float64 product as bop_eval._dot3 forms it (the rounding of the BLAS product behind the recorded reference values):
// a0 b0 rounded, then two fused multiply-adds in k order.  The explicit fma keeps that under -ffp-contract=off.
__device__ __forceinline__ double dot3_blas(double a0, double b0, double a1, double b1, double a2, double b2) {
  return __builtin_fma(a2, b2, __builtin_fma(a1, b1, a0 * b0));
}

}  // namespace unopose
