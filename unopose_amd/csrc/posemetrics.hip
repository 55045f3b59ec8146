// The further pose errors of the evaluation (unopose_amd/bop_eval.py with `error_types=` and `device=`): ADD, ADI, the mean projection
// error and the rotation / translation errors with their symmetry-aware forms, for many (estimate, ground truth) pairs of one object
// per launch.  bop_eval's host functions `add, adi, proj, re, te, proj_sym, re_sym, te_sym` are the specification; everything is float64.
//
//   * pose_metrics: one workgroup of 256 threads per pair.  add / proj: threads stride over the model points, each point's 3-D and
//     projected displacement (one sqrt each) is added to the thread's partial in index order.  projS: as pose_errors_kernel walks the
//     symmetries -- ground truth o symmetry in LDS tiles, a wave takes METRIC_SYM_BLOCK symmetries at a time so that the estimate's point
//     and projection are computed once per point of the block, lanes stride over the points; the pass is left out where projS is not asked
//     for (the row is NaN then) and where the identity is the only symmetry (projS = proj).  re / te / reS / teS: nine products and an
//     acos per symmetry, symmetries strided over the threads; the rotation products are formed in the host's fixed order (bop_eval._dot3 =
//     dot3_blas here) so that both sides hand the same bits to acos (near 0 deg the angle moves by 1e-6 deg per ulp of the cosine).
//     The means are sums whose order is fixed by the launch shape alone: thread partials in point order, xor-shuffle tree over the
//     wave's 64 lanes, the 4 waves added in index order.  No atomics; the same input gives the same bits.
//   * adi: mean over the model points p of the distance from R_g p + t_g to the nearest R_e q + t_e.  That distance equals
//     |p - R_g^T (R_e q + t_e - t_g)|, so only the q side is transformed, into LDS tiles of ADI_TILE points that every thread reads as a
//     broadcast.  A thread keeps ADI_QUERIES query points and their running minima of the SQUARED distance in registers (sqrt after the
//     min).  A pair is split along the query points into slabs of ADI_SLAB = 128 threads x ADI_QUERIES points, one workgroup each: grid
//     (slabs, pairs).  Every (pair, slab) writes one partial sum -- fixed tree again -- to the workspace and adi_finish_kernel adds a
//     pair's slabs in index order and divides by n.
// The kernels trust their sizes and assume finite poses: ops/score.py checks on the host and gives non-finite pairs NaN there.
#include <algorithm>

#include "common.h"
#include "dot3.h"  // dot3_blas: bop_eval._dot3

namespace unopose {

constexpr int METRIC_THREADS = 256;
constexpr int METRIC_SYM_TILE = 256;
constexpr int METRIC_SYM_BLOCK = 4;
constexpr int METRIC_OUTPUTS = 7;  // add, proj, re, te, projS, reS, teS
constexpr int ADI_THREADS = 128;
constexpr int ADI_QUERIES = 2;
constexpr int ADI_SLAB = ADI_THREADS * ADI_QUERIES;
constexpr int ADI_TILE = 1024;

// degrees between two rotations as bop_eval.re forms them: the diagonal of R_e R^T (dot3_blas), added in order, clamped, acos.
// Near 0 degrees one ulp of the cosine is 1e-6 degrees, so the trace has to carry the host's bits.
__device__ __forceinline__ double rotation_error_deg(const double *Re, const double *R) {
  const double d0 = dot3_blas(Re[0], R[0], Re[1], R[1], Re[2], R[2]), d1 = dot3_blas(Re[3], R[3], Re[4], R[4], Re[5], R[5]);
  const double d2 = dot3_blas(Re[6], R[6], Re[7], R[7], Re[8], R[8]);
  double trace = (d0 + d1) + d2;
  trace = trace <= 3.0 ? trace : 3.0;
  const double c = fmin(1.0, fmax(-1.0, 0.5 * (trace - 1.0)));
  return acos(c) * (180.0 / 3.14159265358979323846);
}

__global__ __launch_bounds__(METRIC_THREADS) void pose_metrics_kernel(const double *__restrict__ pts, int n, const double *__restrict__ syms, int S,
                                                                     const double *__restrict__ est, const double *__restrict__ gt,
                                                                     const double *__restrict__ Ks, int P, int proj_sym, double *__restrict__ out) {
  __shared__ double pose[METRIC_SYM_TILE][12];  // ground truth o symmetry: R row-major, then t
  __shared__ double red[4][5];
  const int p = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double *E = est + (size_t)p * 12, *G = gt + (size_t)p * 12, *K = Ks + (size_t)p * 9;
  double Re[12], Rg[12], Kp[9];
#pragma unroll
  for (int k = 0; k < 12; ++k) Re[k] = E[k], Rg[k] = G[k];
#pragma unroll
  for (int k = 0; k < 9; ++k) Kp[k] = K[k];
  const double inf = __builtin_inf();
  // The projS pass is the only part whose work is points x symmetries.  It is left out where the caller does not ask for projS, and where
  // the identity is the only symmetry (every asymmetric object): composing with it leaves the ground truth's bits, so projS IS proj.
  bool sym_pass = proj_sym != 0;
  if (sym_pass && S == 1) {
    bool identity = true;
#pragma unroll
    for (int k = 0; k < 12; ++k) identity = identity && syms[k] == ((k == 0 || k == 4 || k == 8) ? 1.0 : 0.0);
    sym_pass = !identity;
  }

  // add and proj against the ground truth as given
  double s_add = 0.0, s_proj = 0.0;
  for (int i = threadIdx.x; i < n; i += METRIC_THREADS) {
    const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    const double ex = Re[0] * x + Re[1] * y + Re[2] * z + Re[9], ey = Re[3] * x + Re[4] * y + Re[5] * z + Re[10];
    const double ez = Re[6] * x + Re[7] * y + Re[8] * z + Re[11];
    const double gx = Rg[0] * x + Rg[1] * y + Rg[2] * z + Rg[9], gy = Rg[3] * x + Rg[4] * y + Rg[5] * z + Rg[10];
    const double gz = Rg[6] * x + Rg[7] * y + Rg[8] * z + Rg[11];
    const double dx = gx - ex, dy = gy - ey, dz = gz - ez;
    s_add += sqrt(dx * dx + dy * dy + dz * dz);
    const double ew = Kp[6] * ex + Kp[7] * ey + Kp[8] * ez, gw = Kp[6] * gx + Kp[7] * gy + Kp[8] * gz;
    const double du = (Kp[0] * gx + Kp[1] * gy + Kp[2] * gz) / gw - (Kp[0] * ex + Kp[1] * ey + Kp[2] * ez) / ew;
    const double dv = (Kp[3] * gx + Kp[4] * gy + Kp[5] * gz) / gw - (Kp[3] * ex + Kp[4] * ey + Kp[5] * ez) / ew;
    s_proj += sqrt(du * du + dv * dv);
  }
  s_add = wave_all_sum(s_add), s_proj = wave_all_sum(s_proj);

  double min_p = inf, min_r = inf, min_t = inf;
  for (int s0 = 0; s0 < S; s0 += METRIC_SYM_TILE) {
    const int tile = min(METRIC_SYM_TILE, S - s0);
    __syncthreads();  // the previous tile has been read
    for (int s = threadIdx.x; s < tile; s += METRIC_THREADS) {
      const double *Q = syms + (size_t)(s0 + s) * 12;
      double T[12];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) T[3 * r + c] = dot3_blas(Rg[3 * r], Q[c], Rg[3 * r + 1], Q[3 + c], Rg[3 * r + 2], Q[6 + c]);  // R_g . S_R as numpy's dot
        T[9 + r] = Rg[3 * r] * Q[9] + Rg[3 * r + 1] * Q[10] + Rg[3 * r + 2] * Q[11] + Rg[9 + r];
      }
#pragma unroll
      for (int k = 0; k < 12; ++k) pose[s][k] = T[k];
      min_r = fmin(min_r, rotation_error_deg(Re, T));
      const double tx = T[9] - Re[9], ty = T[10] - Re[10], tz = T[11] - Re[11];
      min_t = fmin(min_t, tx * tx + ty * ty + tz * tz);
    }
    __syncthreads();
    for (int b = wave * METRIC_SYM_BLOCK; sym_pass && b < tile; b += 4 * METRIC_SYM_BLOCK) {  // wave-uniform
      double sp[METRIC_SYM_BLOCK];
#pragma unroll
      for (int j = 0; j < METRIC_SYM_BLOCK; ++j) sp[j] = 0.0;
      for (int i = lane; i < n; i += 64) {
        const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
        const double ex = Re[0] * x + Re[1] * y + Re[2] * z + Re[9], ey = Re[3] * x + Re[4] * y + Re[5] * z + Re[10];
        const double ez = Re[6] * x + Re[7] * y + Re[8] * z + Re[11];
        const double ew = Kp[6] * ex + Kp[7] * ey + Kp[8] * ez;
        const double eu = (Kp[0] * ex + Kp[1] * ey + Kp[2] * ez) / ew, ev = (Kp[3] * ex + Kp[4] * ey + Kp[5] * ez) / ew;
#pragma unroll
        for (int j = 0; j < METRIC_SYM_BLOCK; ++j) {
          const double *T = pose[min(b + j, tile - 1)];  // a short last block repeats its last symmetry: the minimum does not change
          const double gx = T[0] * x + T[1] * y + T[2] * z + T[9], gy = T[3] * x + T[4] * y + T[5] * z + T[10];
          const double gz = T[6] * x + T[7] * y + T[8] * z + T[11];
          const double gw = Kp[6] * gx + Kp[7] * gy + Kp[8] * gz;
          const double du = (Kp[0] * gx + Kp[1] * gy + Kp[2] * gz) / gw - eu, dv = (Kp[3] * gx + Kp[4] * gy + Kp[5] * gz) / gw - ev;
          sp[j] += sqrt(du * du + dv * dv);
        }
      }
#pragma unroll
      for (int j = 0; j < METRIC_SYM_BLOCK; ++j) min_p = fmin(min_p, wave_all_sum(sp[j]));
    }
  }
  min_r = wave_all_fmin(min_r), min_t = wave_all_fmin(min_t);
  // a wave without a symmetry block of its own still holds +inf in min_p
  if (lane == 0) red[wave][0] = s_add, red[wave][1] = s_proj, red[wave][2] = min_r, red[wave][3] = min_t, red[wave][4] = min_p;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double tx = Rg[9] - Re[9], ty = Rg[10] - Re[10], tz = Rg[11] - Re[11];
    out[p] = (((red[0][0] + red[1][0]) + red[2][0]) + red[3][0]) / (double)n;
    out[(size_t)2 * P + p] = rotation_error_deg(Re, Rg);
    out[(size_t)3 * P + p] = sqrt(tx * tx + ty * ty + tz * tz);
    const double proj = (((red[0][1] + red[1][1]) + red[2][1]) + red[3][1]) / (double)n;
    out[(size_t)P + p] = proj;
    out[(size_t)4 * P + p] = sym_pass ? fmin(fmin(red[0][4], red[1][4]), fmin(red[2][4], red[3][4])) / (double)n
                                      : proj_sym ? proj : __builtin_nan("");
    out[(size_t)5 * P + p] = fmin(fmin(red[0][2], red[1][2]), fmin(red[2][2], red[3][2]));
    out[(size_t)6 * P + p] = sqrt(fmin(fmin(red[0][3], red[1][3]), fmin(red[2][3], red[3][3])));
  }
}

__global__ __launch_bounds__(ADI_THREADS) void adi_partial_kernel(const double *__restrict__ pts, int n, const double *__restrict__ est,
                                                                 const double *__restrict__ gt, double *__restrict__ partial) {
  __shared__ double tile[ADI_TILE][3];
  __shared__ double red[ADI_THREADS / 64];
  const int p = blockIdx.y, slab = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double *E = est + (size_t)p * 12, *G = gt + (size_t)p * 12;
  // q' = M q + v with M = R_g^T R_e, v = R_g^T (t_e - t_g)
  double M[9], v[3];
  {
    const double dx = E[9] - G[9], dy = E[10] - G[10], dz = E[11] - G[11];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) M[3 * r + c] = G[r] * E[c] + G[3 + r] * E[3 + c] + G[6 + r] * E[6 + c];
      v[r] = G[r] * dx + G[3 + r] * dy + G[6 + r] * dz;
    }
  }
  const double inf = __builtin_inf();
  double qx[ADI_QUERIES], qy[ADI_QUERIES], qz[ADI_QUERIES], best[ADI_QUERIES];
#pragma unroll
  for (int j = 0; j < ADI_QUERIES; ++j) {
    const int i = min(slab * ADI_SLAB + j * ADI_THREADS + (int)threadIdx.x, n - 1);  // a query past the end repeats the last point and is not added
    qx[j] = pts[3 * i], qy[j] = pts[3 * i + 1], qz[j] = pts[3 * i + 2], best[j] = inf;
  }
  for (int t0 = 0; t0 < n; t0 += ADI_TILE) {
    const int count = min(ADI_TILE, n - t0);
    __syncthreads();  // the previous tile has been read
    for (int k = threadIdx.x; k < count; k += ADI_THREADS) {
      const double x = pts[3 * (t0 + k)], y = pts[3 * (t0 + k) + 1], z = pts[3 * (t0 + k) + 2];
      tile[k][0] = M[0] * x + M[1] * y + M[2] * z + v[0];
      tile[k][1] = M[3] * x + M[4] * y + M[5] * z + v[1];
      tile[k][2] = M[6] * x + M[7] * y + M[8] * z + v[2];
    }
    __syncthreads();
    for (int k = 0; k < count; ++k) {
      const double x = tile[k][0], y = tile[k][1], z = tile[k][2];
#pragma unroll
      for (int j = 0; j < ADI_QUERIES; ++j) {
        const double dx = qx[j] - x, dy = qy[j] - y, dz = qz[j] - z;
        best[j] = fmin(best[j], dx * dx + dy * dy + dz * dz);
      }
    }
  }
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < ADI_QUERIES; ++j)
    if (slab * ADI_SLAB + j * ADI_THREADS + (int)threadIdx.x < n) s += sqrt(best[j]);
  s = wave_all_sum(s);
  if (lane == 0) red[wave] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double total = red[0];
#pragma unroll
    for (int w = 1; w < ADI_THREADS / 64; ++w) total += red[w];
    partial[(size_t)p * gridDim.x + slab] = total;
  }
}

__global__ __launch_bounds__(64) void adi_finish_kernel(const double *__restrict__ partial, int slabs, int n, int P, double *__restrict__ adi) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= P) return;
  double s = 0.0;
  for (int k = 0; k < slabs; ++k) s += partial[(size_t)p * slabs + k];
  adi[p] = s / (double)n;
}

}  // namespace unopose

using namespace unopose;

extern "C" {

int unopose_adi_tile_points(void) { return ADI_TILE; }
int unopose_adi_slab_points(void) { return ADI_SLAB; }

int unopose_pose_metrics(const double *pts, int n, const double *syms, int S, const double *est, const double *gt, const double *K, int P,
                         int proj_sym, double *out, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(pts && syms && est && gt && K && out, "pose_metrics: null pointer");
  UNOPOSE_REQUIRE(n >= 1 && n <= (1 << 24) && S >= 1 && P >= 1, "pose_metrics: bad sizes (n=%d S=%d P=%d)", n, S, P);
  hipLaunchKernelGGL(pose_metrics_kernel, dim3(P), dim3(METRIC_THREADS), 0, (hipStream_t)stream, pts, n, syms, S, est, gt, K, P, proj_sym, out);
  return check_launch("pose_metrics");
}

int unopose_adi(const double *pts, int n, const double *est, const double *gt, int P, double *workspace, double *adi, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(pts && est && gt && workspace && adi, "adi: null pointer");
  UNOPOSE_REQUIRE(n >= 1 && n <= (1 << 24) && P >= 1 && P <= 65535, "adi: bad sizes (n=%d P=%d)", n, P);
  const int slabs = cdiv(n, ADI_SLAB);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(adi_partial_kernel, dim3(slabs, P), dim3(ADI_THREADS), 0, s, pts, n, est, gt, workspace);
  if (int rc = check_launch("adi: partial sums")) return rc;
  hipLaunchKernelGGL(adi_finish_kernel, dim3(cdiv(P, 64)), dim3(64), 0, s, workspace, slabs, n, P, adi);
  return check_launch("adi");
}

}  // extern "C"
