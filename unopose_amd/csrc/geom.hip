// Geometry operators of UNOPose's forward hot path for gfx950, C ABI part 2:
//   * unopose_lrf_global        -- LRF.forward + get_batch_lrf
//                                  (utils/model_utils.py:766-823, model/..._pose_estimation_model.py:78-93)
//   * unopose_query_lrf_group   -- QueryAndLRFGroup.forward = ball_query + group + LRF_batch
//                                  (pointnet2/pointnet2_utils.py:429-481, 522-584) in ONE kernel:
//                                  the neighbour list never leaves LDS.
//                                  Neighbour list and frame are lrf.h's, the code pe.hip runs too; only the x axis'
//                                  normalisation differs (finish_frame below).
//   * unopose_weighted_procrustes -- weighted_procrustes (utils/model_utils.py:667-743)
// All 3x3 eigen / singular problems are solved by Jacobi rotations in registers
// (jacobi3.h) instead of torch.svd.

#include "common.h"
#include "jacobi3.h"
#include "lrf.h"
#include "procrustes.h"

namespace unopose {

// Frame construction shared by the global and the per-point LRF, given
//   z  : sign-resolved normal,  acc : sum_i alpha_i beta_i v_i  (model_utils.py:804-812)
// x = acc / (|acc| + 1e-10) by MULTIPLICATION with the reciprocal here, by division in pe.hip's pe_frame_axes: the two forms differ in
// the last bit.  Each is kept because the outputs of its kernels are pinned (golden fixtures, bit-identity records under profiles/).
__device__ __forceinline__ void finish_frame(Vec3 z, Vec3 acc, Vec3 &xp, Vec3 &yp) {
  const float n = sqrtf(dot(acc, acc)) + 1e-10f;
  xp = scale(acc, 1.f / n);
  yp = cross(xp, z);
}

// ------------------------------------------------------------ global LRF ----
__global__ __launch_bounds__(256) void lrf_global_kernel(const float *__restrict__ pts, int N,
                                                         float *__restrict__ out, int use_ref_rad) {
  __shared__ float red[4];
  const int tid = threadIdx.x;
  const float *P = pts + (size_t)blockIdx.x * N * 3;
  float *O = out + (size_t)blockIdx.x * N * 3;
  float sx = 0, sy = 0, sz = 0;
  for (int i = tid; i < N; i += 256) {
    sx += P[i * 3 + 0];
    sy += P[i * 3 + 1];
    sz += P[i * 3 + 2];
  }
  const float inv_n = 1.f / (float)N;
  const float cx = block_sum_256(sx, red) * inv_n;
  const float cy = block_sum_256(sy, red) * inv_n;
  const float cz = block_sum_256(sz, red) * inv_n;

  float a00 = 0, a01 = 0, a02 = 0, a11 = 0, a12 = 0, a22 = 0, rmax = 0;
  for (int i = tid; i < N; i += 256) {
    const float x = cx - P[i * 3 + 0], y = cy - P[i * 3 + 1], z = cz - P[i * 3 + 2];
    a00 += x * x; a01 += x * y; a02 += x * z; a11 += y * y; a12 += y * z; a22 += z * z;
    rmax = fmaxf(rmax, sqrtf(x * x + y * y + z * z));
  }
  a00 = block_sum_256(a00, red) * inv_n;
  a01 = block_sum_256(a01, red) * inv_n;
  a02 = block_sum_256(a02, red) * inv_n;
  a11 = block_sum_256(a11, red) * inv_n;
  a12 = block_sum_256(a12, red) * inv_n;
  a22 = block_sum_256(a22, red) * inv_n;
  const float r = use_ref_rad ? 1.f : block_max_256(rmax, red);

  Vec3 e0, e1, z0;
  float l0, l1, l2;
  eig_sym3(a00, a01, a02, a11, a12, a22, e0, e1, z0, l0, l1, l2);

  float vote = 0;
  for (int i = tid; i < N; i += 256) {
    const float x = cx - P[i * 3 + 0], y = cy - P[i * 3 + 1], z = cz - P[i * 3 + 2];
    const float pr = z0.x * x + z0.y * y + z0.z * z;
    vote += (pr > 1e-3f ? 1.f : 0.f) - (pr < -1e-3f ? 1.f : 0.f);
  }
  vote = block_sum_256(vote, red);
  const Vec3 zp = vote < 0.f ? scale(z0, -1.f) : z0;

  float vx = 0, vy = 0, vz = 0;
  for (int i = tid; i < N; i += 256) {
    const Vec3 xn = v3(P[i * 3 + 0] - cx, P[i * 3 + 1] - cy, P[i * 3 + 2] - cz);
    const float nrm = dot(zp, xn);
    const Vec3 vi = sub(xn, scale(zp, nrm));
    float alpha = r - sqrtf(dot(xn, xn));
    alpha *= alpha;
    const float ab = alpha * (nrm * nrm);
    vx += ab * vi.x; vy += ab * vi.y; vz += ab * vi.z;
  }
  vx = block_sum_256(vx, red);
  vy = block_sum_256(vy, red);
  vz = block_sum_256(vz, red);
  Vec3 xp, yp;
  finish_frame(zp, v3(vx, vy, vz), xp, yp);
  for (int i = tid; i < N; i += 256) {
    const Vec3 q = v3((P[i * 3 + 0] - cx) / r, (P[i * 3 + 1] - cy) / r, (P[i * 3 + 2] - cz) / r);
    O[i * 3 + 0] = dot(xp, q);
    O[i * 3 + 1] = dot(yp, q);
    O[i * 3 + 2] = dot(zp, q);
  }
}

// -------------------------------------- fused ball_query + group + LRF ------
// One wavefront per centre.  LDS: SoA copy of the cloud + one neighbour list per wave.
// out (B,6,N,S): channels 0-2 = p_k - c (un-normalised), 3-5 = R^T (p_k - c) / radius
// (pointnet2_utils.py:567 channel order).
// IDX (the general form of QueryAndLRFGroup.forward, pointnet2_utils.py:548-565): the neighbour lists come from `idx_in` (B,N,S) --
// ball_query around `new_xyz`, optionally re-drawn by sample_uniformly -- channels 0-2 are relative to new_xyz[j] while the frame and
// channels 3-5 stay relative to xyz[j] (P:555 passes `xyz`, not `new_xyz`, to LRF_batch).
template <bool IDX>
__global__ __launch_bounds__(256) void query_lrf_group_kernel(const float *__restrict__ xyz, int N, float radius,
                                                              int S, int cpw, float *__restrict__ out,
                                                              const float *__restrict__ new_xyz, const int *__restrict__ idx_in) {
  extern __shared__ float4 smem4[];
  float *sx = reinterpret_cast<float *>(smem4);
  float *sy = sx + N, *sz = sy + N;
  int *nbr_all = reinterpret_cast<int *>(sz + N);
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int *nbr = nbr_all + wave * S;
  const float *P = xyz + (size_t)b * N * 3;
  for (int e = tid; e < N * 3; e += 256) lrf_stage_coord(sx, sy, sz, e, P[e]);
  __syncthreads();
  const float r2 = radius * radius;
  const size_t chan = (size_t)N * S;
  float *O = out + (size_t)b * 6 * chan;

  for (int ci = 0; ci < cpw; ++ci) {
    const int j = (blockIdx.x * 4 + wave) * cpw + ci;
    if (j >= N) break;  // wave-uniform
    const float cx = sx[j], cy = sy[j], cz = sz[j];
    float qx = cx, qy = cy, qz = cz;  // the centre channels 0-2 are relative to
    if constexpr (IDX) {
      const float *q = new_xyz + ((size_t)b * N + j) * 3;
      qx = q[0]; qy = q[1]; qz = q[2];
      const int *row_in = idx_in + ((size_t)b * N + j) * S;
      for (int l = lane; l < S; l += 64) {
        const int k = row_in[l];
        nbr[l] = (unsigned)k < (unsigned)N ? k : 0;
      }
      wave_lds_handover();
    } else {
      lrf_ball_query<int, int>(sx, sy, sz, N, S, r2, lane, cx, cy, cz, nbr, nullptr, -1, LrfGrid{}, false);
    }
    float a00, a01, a02, a11, a12, a22;
    lrf_covariance(sx, sy, sz, S, lane, cx, cy, cz, nbr, a00, a01, a02, a11, a12, a22);
    Vec3 e0, e1, z0;
    float l0, l1, l2;
    eig_sym3(a00, a01, a02, a11, a12, a22, e0, e1, z0, l0, l1, l2);
    Vec3 xp, yp, zp, acc;
    lrf_vote_xacc(sx, sy, sz, S, radius, lane, cx, cy, cz, nbr, z0, zp, acc);
    finish_frame(zp, acc, xp, yp);

    float *row = O + (size_t)j * S;
    for (int l = lane; l < S; l += 64) {
      const int k = nbr[l];
      const Vec3 d = v3(sx[k] - cx, sy[k] - cy, sz[k] - cz);
      const Vec3 q = v3(d.x / radius, d.y / radius, d.z / radius);
      row[l] = IDX ? sx[k] - qx : d.x;
      row[chan + l] = IDX ? sy[k] - qy : d.y;
      row[2 * chan + l] = IDX ? sz[k] - qz : d.z;
      row[3 * chan + l] = dot(xp, q);
      row[4 * chan + l] = dot(yp, q);
      row[5 * chan + l] = dot(zp, q);
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// -------------------------------------------------- weighted Procrustes -----
// (procrustes_accumulate and procrustes_translation: procrustes.h)
// R, t with ref ~ R src + t (model_utils.py:667-743).  One wavefront per problem.
__global__ __launch_bounds__(256) void procrustes_wave_kernel(const float *__restrict__ src,
                                                              const float *__restrict__ ref,
                                                              const float *__restrict__ w, int M, int N, float thresh,
                                                              float eps, float *__restrict__ Rout,
                                                              float *__restrict__ tout) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  const float *S = src + (size_t)m * N * 3;
  const float *Rf = ref + (size_t)m * N * 3;
  const float *W = w ? w + (size_t)m * N : nullptr;
  float ws = 0;
  for (int i = lane; i < N; i += 64) {
    float wi = W ? W[i] : 1.f;
    wi = wi < thresh ? 0.f : wi;
    ws += wi;
  }
  const float inv = 1.f / (wave_sum_f32(ws) + eps);
  float s0 = 0, s1 = 0, s2 = 0, r0 = 0, r1 = 0, r2 = 0;
  for (int i = lane; i < N; i += 64) {
    float wi = W ? W[i] : 1.f;
    wi = (wi < thresh ? 0.f : wi) * inv;
    s0 += S[i * 3 + 0] * wi; s1 += S[i * 3 + 1] * wi; s2 += S[i * 3 + 2] * wi;
    r0 += Rf[i * 3 + 0] * wi; r1 += Rf[i * 3 + 1] * wi; r2 += Rf[i * 3 + 2] * wi;
  }
  s0 = wave_sum_f32(s0); s1 = wave_sum_f32(s1); s2 = wave_sum_f32(s2);
  r0 = wave_sum_f32(r0); r1 = wave_sum_f32(r1); r2 = wave_sum_f32(r2);
  float h[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = lane; i < N; i += 64) {
    float wi = W ? W[i] : 1.f;
    wi = (wi < thresh ? 0.f : wi) * inv;
    const float a0 = S[i * 3 + 0] - s0, a1 = S[i * 3 + 1] - s1, a2 = S[i * 3 + 2] - s2;
    const float b0 = wi * (Rf[i * 3 + 0] - r0), b1 = wi * (Rf[i * 3 + 1] - r1), b2 = wi * (Rf[i * 3 + 2] - r2);
    procrustes_accumulate(h, a0, a1, a2, b0, b1, b2);
  }
#pragma unroll
  for (int i = 0; i < 9; ++i) h[i] = wave_sum_f32(h[i]);
  float R[9];
  kabsch_from_H(h, R);
  if (lane == 0) {
    float *Ro = Rout + (size_t)m * 9;
#pragma unroll
    for (int i = 0; i < 9; ++i) Ro[i] = R[i];
    procrustes_translation(R, s0, s1, s2, r0, r1, r2, tout + (size_t)m * 3);
  }
}

// One WORKGROUP per problem, the correspondences in REGISTERS (round 5; N <= 256 PPT): a thread owns PPT points, src / ref / w are read
// from memory ONCE (the one-wave-per-problem form above walks them three times: weights, centroids, covariance -- at 256 hypotheses x
// 2048 correspondences per pair, BASELINE configs[4], it is bound by those re-reads: 204 us for 470 MB of operands), the three passes of the
// reference's formulation (model_utils.py:667-743) run on the registers, reductions in a fixed order (DPP wave sums, then the four wave
// partials in order: deterministic).  Also what the model's own two calls per forward want: 32 problems were 32 wavefronts on the chip.
// WAVES = 4: the whole workgroup on one problem; WAVES = 1 (N <= 512): one wavefront per problem, four problems per workgroup, no barriers.
template <int PPT, int WAVES>
__global__ __launch_bounds__(256) void procrustes_block_kernel(const float *__restrict__ src, const float *__restrict__ ref, const float *__restrict__ w,
                                                               int M, int N, float thresh, float eps, float *__restrict__ Rout, float *__restrict__ tout) {
  __shared__ float part[4][9];
  constexpr int TP = 64 * WAVES;   // threads per problem
  const int m = blockIdx.x * (4 / WAVES) + threadIdx.x / TP, tid = threadIdx.x % TP, lane = tid & 63, wave = tid >> 6;
  if (WAVES == 1 && m >= M) return;   // (whole wavefronts: no barrier is skipped)
  const float *S = src + (size_t)m * N * 3, *Rf = ref + (size_t)m * N * 3;
  const float *W = w ? w + (size_t)m * N : nullptr;
  float wi[PPT], sp[PPT][3], rp[PPT][3];
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    const int i = tid + k * TP;
    const bool ok = i < N;
    const int ii = ok ? i : 0;
    const float x = W ? W[ii] : 1.f;
    wi[k] = !ok || x < thresh ? 0.f : x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      sp[k][c] = S[ii * 3 + c];
      rp[k][c] = Rf[ii * 3 + c];
    }
  }
  auto block_sum = [&](float (&v)[9], int n) {   // v[0..n) summed over the workgroup, result in every thread
#pragma unroll
    for (int c = 0; c < 9; ++c)
      if (c < n) v[c] = wave_sum_f32(v[c]);
    if (WAVES == 1) return;
    __syncthreads();   // (the previous round's partials have been read)
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < 9; ++c)
        if (c < n) part[wave][c] = v[c];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 9; ++c)
      if (c < n) v[c] = (part[0][c] + part[1][c]) + (part[2][c] + part[3][c]);
  };
  float v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < PPT; ++k) v[0] += wi[k];
  block_sum(v, 1);
  const float inv = 1.f / (v[0] + eps);
#pragma unroll
  for (int c = 0; c < 9; ++c) v[c] = 0.f;
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    wi[k] *= inv;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      v[c] += sp[k][c] * wi[k];
      v[3 + c] += rp[k][c] * wi[k];
    }
  }
  block_sum(v, 6);
  const float s0 = v[0], s1 = v[1], s2 = v[2], r0 = v[3], r1 = v[4], r2 = v[5];
  float h[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    const float a0 = sp[k][0] - s0, a1 = sp[k][1] - s1, a2 = sp[k][2] - s2;
    const float b0 = wi[k] * (rp[k][0] - r0), b1 = wi[k] * (rp[k][1] - r1), b2 = wi[k] * (rp[k][2] - r2);
    procrustes_accumulate(h, a0, a1, a2, b0, b1, b2);
  }
  block_sum(h, 9);
  if (tid == 0) {
    float R[9];
    kabsch_from_H(h, R);
    float *Ro = Rout + (size_t)m * 9;
#pragma unroll
    for (int i = 0; i < 9; ++i) Ro[i] = R[i];
    procrustes_translation(R, s0, s1, s2, r0, r1, r2, tout + (size_t)m * 3);
  }
}

// One THREAD per problem for tiny N (the 3-point hypotheses of the coarse stage).
template <int NP>
__global__ __launch_bounds__(256) void procrustes_thread_kernel(const float *__restrict__ src,
                                                                const float *__restrict__ ref,
                                                                const float *__restrict__ w, int M, float thresh,
                                                                float eps, float *__restrict__ Rout,
                                                                float *__restrict__ tout) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  const float *S = src + (size_t)m * NP * 3;
  const float *Rf = ref + (size_t)m * NP * 3;
  float wi[NP], ws = 0;
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    float x = w ? w[(size_t)m * NP + i] : 1.f;
    wi[i] = x < thresh ? 0.f : x;
    ws += wi[i];
  }
  const float inv = 1.f / (ws + eps);
  float s0 = 0, s1 = 0, s2 = 0, r0 = 0, r1 = 0, r2 = 0;
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    wi[i] *= inv;
    s0 += S[i * 3 + 0] * wi[i]; s1 += S[i * 3 + 1] * wi[i]; s2 += S[i * 3 + 2] * wi[i];
    r0 += Rf[i * 3 + 0] * wi[i]; r1 += Rf[i * 3 + 1] * wi[i]; r2 += Rf[i * 3 + 2] * wi[i];
  }
  float h[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const float a0 = S[i * 3 + 0] - s0, a1 = S[i * 3 + 1] - s1, a2 = S[i * 3 + 2] - s2;
    const float b0 = wi[i] * (Rf[i * 3 + 0] - r0), b1 = wi[i] * (Rf[i * 3 + 1] - r1),
                b2 = wi[i] * (Rf[i * 3 + 2] - r2);
    procrustes_accumulate(h, a0, a1, a2, b0, b1, b2);
  }
  float R[9];
  kabsch_from_H(h, R);
  float *Ro = Rout + (size_t)m * 9;
#pragma unroll
  for (int i = 0; i < 9; ++i) Ro[i] = R[i];
  procrustes_translation(R, s0, s1, s2, r0, r1, r2, tout + (size_t)m * 3);
}

}  // namespace unopose

using namespace unopose;

// query_lrf_group (IDX = false: the kernel's own ball query around the points) and lrf_group_idx (IDX = true: the caller's lists)
template <bool IDX>
static int launch_query_lrf_group(const float *xyz, const float *new_xyz, const int *idx, int B, int N, float radius, int nsample,
                                  float *out, unopose_stream_t stream) {
  constexpr const char *what = IDX ? "lrf_group_idx" : "query_lrf_group";
  UNOPOSE_REQUIRE(xyz && out && (!IDX || (new_xyz && idx)), "%s: null pointer", what);
  UNOPOSE_REQUIRE(B >= 0 && N >= 1 && nsample >= 1 && B <= 65535, "%s: bad sizes", what);
  if (B == 0) return UNOPOSE_OK;
  const size_t lds = ((size_t)3 * N + 4 * (size_t)nsample) * 4;  // the cloud + one list per wave
  UNOPOSE_REQUIRE(lds <= 64 * 1024, "%s: N=%d nsample=%d exceed the 64 KiB LDS tile", what, N, nsample);
  const long centres = (long)B * N;
  const int cpw = centres >= 65536 ? 8 : centres >= 16384 ? 4 : centres >= 4096 ? 2 : 1;
  hipLaunchKernelGGL(query_lrf_group_kernel<IDX>, dim3(cdiv(N, 4 * cpw), B), dim3(256), lds, (hipStream_t)stream, xyz, N, radius,
                     nsample, cpw, out, new_xyz, idx);
  return check_launch(what);
}

extern "C" {

int unopose_lrf_global(const float *pts, int B, int N, int use_ref_rad, float *out, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(pts && out, "lrf_global: null pointer");
  UNOPOSE_REQUIRE(B >= 0 && N >= 1, "lrf_global: bad sizes");
  if (B == 0) return UNOPOSE_OK;
  hipLaunchKernelGGL(lrf_global_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, pts, N, out, use_ref_rad);
  return check_launch("lrf_global");
}

int unopose_query_lrf_group(const float *xyz, int B, int N, float radius, int nsample, float *out,
                            unopose_stream_t stream) {
  return launch_query_lrf_group<false>(xyz, nullptr, nullptr, B, N, radius, nsample, out, stream);
}

int unopose_lrf_group_idx(const float *xyz, const float *new_xyz, const int *idx, int B, int N, float radius, int nsample,
                          float *out, unopose_stream_t stream) {
  return launch_query_lrf_group<true>(xyz, new_xyz, idx, B, N, radius, nsample, out, stream);
}

int unopose_weighted_procrustes(const float *src, const float *ref, const float *w, int M, int N, float thresh,
                                float eps, float *R, float *t, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(src && ref && R && t, "weighted_procrustes: null pointer");
  UNOPOSE_REQUIRE(M >= 0 && N >= 1, "weighted_procrustes: bad sizes");
  if (M == 0) return UNOPOSE_OK;
  hipStream_t s = (hipStream_t)stream;
  if (N == 3) {
    hipLaunchKernelGGL(procrustes_thread_kernel<3>, dim3(cdiv(M, 256)), dim3(256), 0, s, src, ref, w, M, thresh, eps,
                       R, t);
  } else if (N <= 2048) {
#define UNOPOSE_PB(P, WV) hipLaunchKernelGGL((procrustes_block_kernel<P, WV>), dim3(cdiv(M, 4 / WV)), dim3(256), 0, s, src, ref, w, M, N, thresh, eps, R, t)
    if (N <= 64) UNOPOSE_PB(1, 1);
    else if (N <= 128) UNOPOSE_PB(2, 1);
    else if (N <= 256) UNOPOSE_PB(4, 1);
    else if (N <= 512) UNOPOSE_PB(8, 1);
    else if (N <= 1024) UNOPOSE_PB(4, 4);
    else UNOPOSE_PB(8, 4);
#undef UNOPOSE_PB
  } else {
    hipLaunchKernelGGL(procrustes_wave_kernel, dim3(cdiv(M, 4)), dim3(256), 0, s, src, ref, w, M, N, thresh, eps, R,
                       t);
  }
  return check_launch("weighted_procrustes");
}

}  // extern "C"
