// Pose-error kernels of the BOP'19 scorer (unopose_amd/bop_eval.py with `device=`): everything between the rasteriser's depth maps and
// the host's greedy matching, for many (estimate, ground truth) pairs per launch.  bop_eval's own functions are the specification.
//
//   * vsd_counts: the 2 + T integer counts inside bop_eval.vsd -- |union|, |intersection| of the two visibility masks and, for each of the
//     T misalignment tolerances tau, the intersection pixels with |dist_gt - dist_est| / diameter >= tau -- held to EQUALITY with numpy,
//     so every expression keeps bop_eval.depth_to_dist / _visib_mask / vsd's casts and evaluation order (the build's
//     -ffp-contract=off keeps the float64 ones as written; float64 sqrt and division are correctly rounded on both sides):
//         pre_x = (x - cx) / fx, pre_y = (y - cy) / fy                                   float64
//         dist  = sqrt((pre_x * d) * (pre_x * d) + (pre_y * d) * (pre_y * d) + d * d)    float64, d = (double)depth
//         visible(model) = ((float)dist_model - (float)dist_test <= delta  ||  dist_test == 0)  &&  dist_model > 0
//     A pixel whose two rendered depths are both exactly 0 has dist_gt = dist_est = 0 and is in neither mask: it is skipped before
//     any float64 work, which is most of the image.  The kernel is a stream of 12 bytes per pixel read as 16-byte loads; counters
//     live in registers, are reduced over the wave and through LDS, and leave the block as one integer atomic add per non-zero
//     counter -- integer sums do not depend on the order.
//   * pose_errors: bop_eval.mssd / mspd -- min over the object's symmetries of the max over model points of the 3-D and of the
//     projected displacement.  One workgroup per pair; the ground-truth pose composed with each symmetry sits in LDS (tiles of
//     POSE_SYM_TILE symmetries), a wave takes POSE_SYM_BLOCK symmetries at a time so that the estimate's point and projection are
//     computed once per block, points are strided over its lanes.  max is taken on the squared distance (sqrt is monotonic) and
//     NaNs propagate as in numpy's max / min.  The host side goes through BLAS, so this one is held to a bound, not to equality.
#include <algorithm>

#include "common.h"
#include "visib.h"

namespace unopose {

constexpr int VSD_MAX_TAUS = 16;
constexpr int VSD_COUNTS = 2 + VSD_MAX_TAUS;  // n_union, n_inter, one count per tau
constexpr int VSD_PAIR_DOUBLES = 6;           // fx, fy, cx, cy, delta, diameter
constexpr int VSD_PAIR_INTS = 3;              // index of the test image, of the ground-truth map, of the estimate map
constexpr int VSD_PIXELS_PER_THREAD = 16;
constexpr int POSE_SYM_TILE = 256;
constexpr int POSE_SYM_BLOCK = 4;

struct VsdTaus {
  double v[VSD_MAX_TAUS];  // unused entries hold +inf: their counts stay 0
};

// one pixel into the thread's counters
__device__ __forceinline__ void vsd_pixel(int idx, int W, float d_test, float d_gt, float d_est, double fx, double fy, double cx, double cy,
                                          double delta, double diameter, const VsdTaus &taus, int (&cnt)[VSD_COUNTS]) {
  if (d_gt == 0.f && d_est == 0.f) return;
  const int y = idx / W, x = idx - y * W;
  const double pre_x = ((double)x - cx) / fx, pre_y = ((double)y - cy) / fy;
  const double t = vsd_dist(pre_x, pre_y, d_test), g = vsd_dist(pre_x, pre_y, d_gt), e = vsd_dist(pre_x, pre_y, d_est);
  const bool no_test = t == 0.0;
  const bool visib_gt = ((double)((float)g - (float)t) <= delta || no_test) && g > 0.0;
  const bool visib_est = (((double)((float)e - (float)t) <= delta || no_test) && e > 0.0) || (visib_gt && e > 0.0);
  cnt[0] += (visib_gt || visib_est) ? 1 : 0;
  if (visib_gt && visib_est) {
    cnt[1] += 1;
    const double err = fabs(g - e) / diameter;
#pragma unroll
    for (int k = 0; k < VSD_MAX_TAUS; ++k) cnt[2 + k] += err >= taus.v[k] ? 1 : 0;
  }
}

__global__ __launch_bounds__(256) void vsd_counts_kernel(const float *__restrict__ test, const float *__restrict__ gt, const float *__restrict__ est,
                                                        const int *__restrict__ index, const double *__restrict__ pairs, VsdTaus taus, int H, int W,
                                                        int wide, int *__restrict__ counts) {
  __shared__ int part[4][VSD_COUNTS];
  const int p = blockIdx.y, HW = H * W;
  const int *ix = index + (size_t)p * VSD_PAIR_INTS;
  const double *q = pairs + (size_t)p * VSD_PAIR_DOUBLES;
  const double fx = q[0], fy = q[1], cx = q[2], cy = q[3], delta = q[4], diameter = q[5];
  const float *mt = test + (size_t)ix[0] * HW, *mg = gt + (size_t)ix[1] * HW, *me = est + (size_t)ix[2] * HW;
  int cnt[VSD_COUNTS];
#pragma unroll
  for (int k = 0; k < VSD_COUNTS; ++k) cnt[k] = 0;
  if (wide) {  // every map starts on a 16-byte boundary: the host checked the three base pointers and H * W % 4 == 0
    const f32x4 *vt = (const f32x4 *)mt, *vg = (const f32x4 *)mg, *ve = (const f32x4 *)me;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < (HW >> 2); i += gridDim.x * 256) {
      const f32x4 a = vt[i], b = vg[i], c = ve[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) vsd_pixel(4 * i + j, W, a[j], b[j], c[j], fx, fy, cx, cy, delta, diameter, taus, cnt);
    }
  } else {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += gridDim.x * 256)
      vsd_pixel(i, W, mt[i], mg[i], me[i], fx, fy, cx, cy, delta, diameter, taus, cnt);
  }
#pragma unroll
  for (int k = 0; k < VSD_COUNTS; ++k) cnt[k] = wave_all_sum(cnt[k]);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < VSD_COUNTS; ++k) part[wave][k] = cnt[k];
  }
  __syncthreads();
  if (threadIdx.x < VSD_COUNTS) {
    const int k = threadIdx.x, v = part[0][k] + part[1][k] + part[2][k] + part[3][k];
    if (v) atomicAdd(counts + (size_t)p * VSD_COUNTS + k, v);
  }
}

// numpy's max / min: a NaN wins
__device__ __forceinline__ double nan_max(double m, double v) { return (v > m || v != v) ? v : m; }
__device__ __forceinline__ double nan_min(double m, double v) { return (v < m || v != v) ? v : m; }

__global__ __launch_bounds__(256) void pose_errors_kernel(const double *__restrict__ pts, int n, const double *__restrict__ syms, int S,
                                                         const double *__restrict__ est, const double *__restrict__ gt,
                                                         const double *__restrict__ Ks, double *__restrict__ mssd, double *__restrict__ mspd) {
  __shared__ double pose[POSE_SYM_TILE][12];  // ground truth o symmetry: R row-major, then t
  __shared__ double best[4][2];
  const int p = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double *E = est + (size_t)p * 12, *G = gt + (size_t)p * 12, *K = Ks + (size_t)p * 9;
  double Re[12], Kp[9];
#pragma unroll
  for (int k = 0; k < 12; ++k) Re[k] = E[k];
#pragma unroll
  for (int k = 0; k < 9; ++k) Kp[k] = K[k];
  const double inf = __builtin_inf();
  const auto nmax = [](double m, double v) { return nan_max(m, v); };  // not symmetric: the wave's own value is the first operand
  double min_s = inf, min_p = inf;
  for (int s0 = 0; s0 < S; s0 += POSE_SYM_TILE) {
    const int tile = min(POSE_SYM_TILE, S - s0);
    __syncthreads();  // the previous tile has been read
    for (int s = threadIdx.x; s < tile; s += 256) {
      const double *Q = syms + (size_t)(s0 + s) * 12;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) pose[s][3 * r + c] = G[3 * r] * Q[c] + G[3 * r + 1] * Q[3 + c] + G[3 * r + 2] * Q[6 + c];
        pose[s][9 + r] = G[3 * r] * Q[9] + G[3 * r + 1] * Q[10] + G[3 * r + 2] * Q[11] + G[9 + r];
      }
    }
    __syncthreads();
    for (int b = wave * POSE_SYM_BLOCK; b < tile; b += 4 * POSE_SYM_BLOCK) {  // wave-uniform
      double ms[POSE_SYM_BLOCK], mp[POSE_SYM_BLOCK];
#pragma unroll
      for (int j = 0; j < POSE_SYM_BLOCK; ++j) ms[j] = mp[j] = 0.0;  // distances are >= 0
      for (int i = lane; i < n; i += 64) {
        const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
        const double ex = Re[0] * x + Re[1] * y + Re[2] * z + Re[9], ey = Re[3] * x + Re[4] * y + Re[5] * z + Re[10];
        const double ez = Re[6] * x + Re[7] * y + Re[8] * z + Re[11];
        const double ew = Kp[6] * ex + Kp[7] * ey + Kp[8] * ez;
        const double eu = (Kp[0] * ex + Kp[1] * ey + Kp[2] * ez) / ew, ev = (Kp[3] * ex + Kp[4] * ey + Kp[5] * ez) / ew;
#pragma unroll
        for (int j = 0; j < POSE_SYM_BLOCK; ++j) {
          const double *T = pose[min(b + j, tile - 1)];  // a short last block repeats its last symmetry: the minimum does not change
          const double gx = T[0] * x + T[1] * y + T[2] * z + T[9], gy = T[3] * x + T[4] * y + T[5] * z + T[10];
          const double gz = T[6] * x + T[7] * y + T[8] * z + T[11];
          const double dx = gx - ex, dy = gy - ey, dz = gz - ez;
          ms[j] = nan_max(ms[j], dx * dx + dy * dy + dz * dz);
          const double gw = Kp[6] * gx + Kp[7] * gy + Kp[8] * gz;
          const double du = (Kp[0] * gx + Kp[1] * gy + Kp[2] * gz) / gw - eu, dv = (Kp[3] * gx + Kp[4] * gy + Kp[5] * gz) / gw - ev;
          mp[j] = nan_max(mp[j], du * du + dv * dv);
        }
      }
#pragma unroll
      for (int j = 0; j < POSE_SYM_BLOCK; ++j) {
        min_s = nan_min(min_s, wave_all(ms[j], nmax));
        min_p = nan_min(min_p, wave_all(mp[j], nmax));
      }
    }
  }
  if (lane == 0) best[wave][0] = min_s, best[wave][1] = min_p;
  __syncthreads();
  if (threadIdx.x == 0) {
    // a wave without a symmetry block of its own still holds +inf
    mssd[p] = sqrt(nan_min(nan_min(best[0][0], best[1][0]), nan_min(best[2][0], best[3][0])));
    mspd[p] = sqrt(nan_min(nan_min(best[0][1], best[1][1]), nan_min(best[2][1], best[3][1])));
  }
}

}  // namespace unopose

using namespace unopose;

extern "C" {

int unopose_vsd_count_ints(void) { return VSD_COUNTS; }

int unopose_vsd_counts(const float *test, int n_test, const float *gt, int n_gt, const float *est, int n_est, const int *index,
                       const double *pairs, const double *taus, int T, int P, int H, int W, int *counts, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(test && gt && est && index && pairs && taus && counts, "vsd_counts: null pointer");
  UNOPOSE_REQUIRE(n_test >= 1 && n_gt >= 1 && n_est >= 1 && T >= 1 && T <= VSD_MAX_TAUS && P >= 1 && P <= 65535 && H >= 1 && W >= 1 &&
                      (long)H * W <= (1L << 30),
                  "vsd_counts: bad sizes (maps %d / %d / %d, T=%d P=%d H=%d W=%d)", n_test, n_gt, n_est, T, P, H, W);
  VsdTaus t;
  for (int k = 0; k < VSD_MAX_TAUS; ++k) t.v[k] = k < T ? taus[k] : __builtin_inf();
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(counts, 0, (size_t)P * VSD_COUNTS * sizeof(int), s) != hipSuccess) return check_launch("vsd_counts: memset");
  const int blocks = std::min(std::max(cdiv((long)H * W, 256L * VSD_PIXELS_PER_THREAD), 1), 256);
  // 16-byte loads need every map on a 16-byte boundary; a view that starts elsewhere takes the scalar loop
  const int wide = ((long)H * W) % 4 == 0 && (((uintptr_t)test | (uintptr_t)gt | (uintptr_t)est) & 15) == 0;
  hipLaunchKernelGGL(vsd_counts_kernel, dim3(blocks, P), dim3(256), 0, s, test, gt, est, index, pairs, t, H, W, wide, counts);
  return check_launch("vsd_counts");
}

int unopose_pose_errors(const double *pts, int n, const double *syms, int S, const double *est, const double *gt, const double *K, int P,
                        double *mssd, double *mspd, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(pts && syms && est && gt && K && mssd && mspd, "pose_errors: null pointer");
  UNOPOSE_REQUIRE(n >= 1 && S >= 1 && P >= 1, "pose_errors: bad sizes (n=%d S=%d P=%d)", n, S, P);
  hipLaunchKernelGGL(pose_errors_kernel, dim3(P), dim3(256), 0, (hipStream_t)stream, pts, n, syms, S, est, gt, K, mssd, mspd);
  return check_launch("pose_errors");
}

}  // extern "C"
