// Pose refinement on the device, C ABI: unopose_icp_refine -- a batched, trimmed, Cauchy-weighted ICP, the whole loop of a pair in ONE
// workgroup and ONE launch.  The rule (tests/icp_ref.py states it in float64 numpy; ops.icp_refine's docstring restates it) is
// post_refinement (utils/model_utils.py:649-664) applied per pair with the correspondences found anew in every iteration:
//   x_i = (p_i - t) R;  j_i = argmin_j |x_i - q_j|^2 (lowest j on ties), d_i = sqrt(min);  in_i = m_i != 0 and d_i < tau;
//   c = sum in_i;  stop if c <= the previous count or c < 3;  w_i = in_i / (1 + (d_i / tau)^2);
//   (R, t) = weighted_procrustes(src = q_{j_i}, ref = p_i, w, weight_thresh = 0, eps = 1e-5).
// Layout of the work: a thread keeps its PPT query points in registers for the whole loop; the reference cloud is staged into LDS as
// three planes in tiles of ICP_TILE points (one tile: staged once; more: re-staged per iteration) and read as wave-uniform 16-byte
// broadcasts; the 2 + 6 + 9 sums go through wave_sum_f32 and are combined over the waves in wave order, so two runs agree bit for
// bit; thread 0 solves the 3x3 problem (kabsch_from_H) and hands R, t to the others through LDS.  No atomics, nothing waits on
// another workgroup, the stop is a workgroup-uniform branch.
#include "common.h"
#include "jacobi3.h"
#include "procrustes.h"

namespace unopose {

constexpr int ICP_TILE = 4096;      // reference points per LDS tile: 3 planes x 16 KiB, inside the 64 KiB every kernel gets
constexpr int ICP_MAX_WAVES = 16;   // 1024 threads
constexpr int ICP_MAX_N1 = 4096, ICP_MAX_N2 = 16384;

struct IcpLds {
  float q[3][ICP_TILE];
  float part[ICP_MAX_WAVES][9];
  float pose[12];
};

template <int PPT>
__global__ __launch_bounds__(1024) void icp_refine_kernel(const float *__restrict__ p, const float *__restrict__ q, const float *__restrict__ mask,
                                                          int N1, int N2, const float *__restrict__ R_in, const float *__restrict__ t_in, float tau,
                                                          int iters, float *__restrict__ R_out, float *__restrict__ t_out, int *__restrict__ trace,
                                                          int *__restrict__ idx, float *__restrict__ dist) {
  __shared__ __attribute__((aligned(16))) IcpLds lds;
  const int b = blockIdx.x, tid = threadIdx.x, T = blockDim.x, lane = tid & 63, wave = tid >> 6, NW = T >> 6;
  const float *P = p + (size_t)b * N1 * 3, *Q = q + (size_t)b * N2 * 3;
  const float *M = mask ? mask + (size_t)b * N1 : nullptr;
  const float inf = __builtin_inff();

  float pp[PPT][3], d[PPT];
  int bj[PPT];
  bool live[PPT];
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    const int i = tid + k * T;
    const bool ok = i < N1;
    const int ii = ok ? i : 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) pp[k][c] = P[ii * 3 + c];
    live[k] = ok && (M ? M[ii] != 0.f : true);
    d[k] = inf;   // what idx / dist hold when no search ran (iters = 0)
    bj[k] = -1;
  }
  float R[9], t[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = R_in[(size_t)b * 9 + i];
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = t_in[(size_t)b * 3 + i];

  auto block_sum = [&](float (&v)[9], int n) {   // v[0..n) summed over the workgroup in a fixed order, result in every thread
#pragma unroll
    for (int c = 0; c < 9; ++c)
      if (c < n) v[c] = wave_sum_f32(v[c]);
    __syncthreads();   // (the previous round's partials have been read)
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < 9; ++c)
        if (c < n) lds.part[wave][c] = v[c];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 9; ++c)
      if (c < n) {
        float s = lds.part[0][c];
        for (int w = 1; w < NW; ++w) s += lds.part[w][c];
        v[c] = s;
      }
  };

  int prev = 0, done = 0;   // done: entries of trace written
  for (int it = 0; it < iters; ++it) {
    float x[PPT][3], best[PPT];
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      const float a0 = pp[k][0] - t[0], a1 = pp[k][1] - t[1], a2 = pp[k][2] - t[2];
#pragma unroll
      for (int c = 0; c < 3; ++c) x[k][c] = (a0 * R[c] + a1 * R[3 + c]) + a2 * R[6 + c];
      best[k] = inf;
      bj[k] = 0;
    }
    // ---- nearest reference point: ascending j and a strict <, so the lowest index wins a tie
    for (int tile0 = 0; tile0 < N2; tile0 += ICP_TILE) {
      const int n = min(ICP_TILE, N2 - tile0), n4 = (n + 3) & ~3;
      if (it == 0 || N2 > ICP_TILE) {   // workgroup-uniform
        __syncthreads();   // (the tile before has been searched)
        for (int e = tid; e < n * 3; e += T) {
          const int j = e / 3;
          lds.q[e - 3 * j][j] = Q[(size_t)tile0 * 3 + e];
        }
        for (int j = n + tid; j < n4; j += T) lds.q[0][j] = lds.q[1][j] = lds.q[2][j] = inf;   // (distance inf: never < best)
        __syncthreads();
      }
#pragma unroll 2
      for (int j = 0; j < n4; j += 4) {
        const f32x4 qx = *reinterpret_cast<const f32x4 *>(&lds.q[0][j]);
        const f32x4 qy = *reinterpret_cast<const f32x4 *>(&lds.q[1][j]);
        const f32x4 qz = *reinterpret_cast<const f32x4 *>(&lds.q[2][j]);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
          for (int k = 0; k < PPT; ++k) {
            const float dx = x[k][0] - qx[u], dy = x[k][1] - qy[u], dz = x[k][2] - qz[u];
            const float d2 = (dx * dx + dy * dy) + dz * dz;
            if (d2 < best[k]) {
              best[k] = d2;
              bj[k] = tile0 + j + u;
            }
          }
        }
      }
    }
    // ---- inliers, their count and weights
    float w[PPT], v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      d[k] = sqrtf(best[k]);
      const bool in = live[k] && d[k] < tau;
      const float r = d[k] / tau;
      w[k] = in ? 1.f / (1.f + r * r) : 0.f;
      v[0] += w[k];
      v[1] += in ? 1.f : 0.f;   // (exact: at most 4096)
    }
    block_sum(v, 2);
    const int count = (int)v[1];
    if (tid == 0 && trace) trace[(size_t)b * iters + it] = count;
    done = it + 1;
    if (count <= prev || count < 3) break;   // workgroup-uniform
    prev = count;
    // ---- weighted Procrustes, src = q_j, ref = p (the three passes of geom.hip's procrustes_block_kernel)
    const float inv = 1.f / (v[0] + 1e-5f);
    float sp[PPT][3];
#pragma unroll
    for (int c = 0; c < 9; ++c) v[c] = 0.f;
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      w[k] *= inv;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        sp[k][c] = Q[(size_t)bj[k] * 3 + c];
        v[c] += sp[k][c] * w[k];
        v[3 + c] += pp[k][c] * w[k];
      }
    }
    block_sum(v, 6);
    const float s0 = v[0], s1 = v[1], s2 = v[2], r0 = v[3], r1 = v[4], r2 = v[5];
    float h[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      const float a0 = sp[k][0] - s0, a1 = sp[k][1] - s1, a2 = sp[k][2] - s2;
      const float b0 = w[k] * (pp[k][0] - r0), b1 = w[k] * (pp[k][1] - r1), b2 = w[k] * (pp[k][2] - r2);
      procrustes_accumulate(h, a0, a1, a2, b0, b1, b2);
    }
    block_sum(h, 9);
    if (tid == 0) {
      float Rn[9];
      kabsch_from_H(h, Rn);
#pragma unroll
      for (int i = 0; i < 9; ++i) lds.pose[i] = Rn[i];
      procrustes_translation(Rn, s0, s1, s2, r0, r1, r2, &lds.pose[9]);
    }
    __syncthreads();   // (thread 0 writes the next pose only after the three barriers of the next round's sums)
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = lds.pose[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = lds.pose[9 + i];
  }

  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < 9; ++i) R_out[(size_t)b * 9 + i] = R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) t_out[(size_t)b * 3 + i] = t[i];
  }
  if (trace)
    for (int k = done + tid; k < iters; k += T) trace[(size_t)b * iters + k] = -1;
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    const int i = tid + k * T;
    if (i < N1) {
      if (idx) idx[(size_t)b * N1 + i] = bj[k];
      if (dist) dist[(size_t)b * N1 + i] = d[k];
    }
  }
}

}  // namespace unopose

using namespace unopose;

extern "C" {

int unopose_icp_refine(const float *p, const float *q, const float *mask, int B, int N1, int N2, const float *R_in, const float *t_in,
                       float tau, int iters, float *R_out, float *t_out, int *trace, int *idx, float *dist, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(p && q && R_in && t_in && R_out && t_out, "icp_refine: null pointer");
  UNOPOSE_REQUIRE(B >= 0 && N1 >= 1 && N2 >= 1 && iters >= 0 && tau > 0.f, "icp_refine: bad sizes");
  UNOPOSE_REQUIRE(N1 <= ICP_MAX_N1 && N2 <= ICP_MAX_N2 && B <= 65535, "icp_refine: N1=%d N2=%d B=%d exceed the limits N1 <= %d, N2 <= %d, B <= 65535",
                  N1, N2, B, ICP_MAX_N1, ICP_MAX_N2);
  if (B == 0) return UNOPOSE_OK;
  // the fewest points per thread that fit N1 into 1024 threads, then the fewest whole waves that hold them
  const int ppt = N1 <= 1024 ? 1 : N1 <= 2048 ? 2 : 4;
  const int threads = 64 * cdiv(cdiv(N1, ppt), 64);
#define UNOPOSE_ICP(P) hipLaunchKernelGGL(icp_refine_kernel<P>, dim3(B), dim3(threads), 0, (hipStream_t)stream, p, q, mask, N1, N2, R_in, t_in, tau, \
                                          iters, R_out, t_out, trace, idx, dist)
  if (ppt == 1) UNOPOSE_ICP(1);
  else if (ppt == 2) UNOPOSE_ICP(2);
  else UNOPOSE_ICP(4);
#undef UNOPOSE_ICP
  return check_launch("icp_refine");
}

}  // extern "C"
