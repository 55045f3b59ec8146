// Fused positional-encoding branch of the fine matcher for gfx950 (C ABI part 2).
//
// Replaces, per scale, QueryAndLRFGroup -> SharedMLP[6,32,64,128] -> max over neighbours
// (core/unopose/model/oneref_predator_fine_point_matching.py:167-174,
//  core/unopose/model/pointnet2/pointnet2_utils.py:429-584, pointnet2/pytorch_utils.py:25-132).
// The reference materialises (B,6,N,S), (B,32,N,S), (B,64,N,S) and (B,128,N,S) fp32 tensors in HBM
// (268 MB for the last one alone at S=256, B=1).  Here ONE wavefront owns one centre: ball-query
// compaction into an LDS neighbour list, the per-point local reference frame (register Jacobi), and the
// three 1x1-conv layers (BatchNorm folded) chained on the fp32 matrix cores
// (v_mfma_f32_32x32x2_f32, exact fp32) with NO data movement between layers: the layers are computed
// transposed, D[out_ch][neighbour] = W[out_ch][k] * X[k][neighbour], so a layer's accumulator registers
// are directly the next layer's B operand (the k order inside the contraction is permuted to match the
// C/D register layout, and the weights are staged in LDS in that permuted order).  Only the (B,N,128)
// max-pooled result reaches HBM.
// That is the exact-fp32 kernel (pe_group_mlp_max_kernel).  The bf16 hi/lo-split form further down is two kernels: pe_geometry_kernel writes
// the lists, counts and frames of one or both scales of a cloud, pe_group_mlp_max_bf16x3_kernel runs the MLP + max over them.
// Neighbour list and frame are lrf.h's, the code geom.hip's query_lrf_group_kernel runs too; only the x axis' normalisation differs
// (pe_frame_axes below).
#include <algorithm>

#include "common.h"
#include "jacobi3.h"
#include "lrf.h"

namespace unopose {

// channel held by accumulator register r of half-wave h in the 32x32 C/D layout
__device__ __forceinline__ int cd_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// The ball query's grid (LrfGrid, lrf.h) is built by pe_geometry_kernel: at most PE_GDIM cells per axis.
constexpr int PE_GDIM = 8, PE_GCELLS = PE_GDIM * PE_GDIM * PE_GDIM;

// The frame of one centre from z0, the eigenvector of the smallest eigenvalue of the covariance (wave-uniform).
template <typename NT>
__device__ __forceinline__ void pe_frame_axes(const float *sx, const float *sy, const float *sz, int S, float radius, int lane,
                                              float cx, float cy, float cz, const NT *nbr, Vec3 z0, Vec3 &xp, Vec3 &yp, Vec3 &zp) {
  Vec3 acc;
  lrf_vote_xacc(sx, sy, sz, S, radius, lane, cx, cy, cz, nbr, z0, zp, acc);
  // x = acc / (|acc| + 1e-10) by DIVISION here, by multiplication with the reciprocal in geom.hip's finish_frame: the two forms differ
  // in the last bit.  Each is kept because the outputs of its kernels are pinned (bit-identity records under profiles/).
  const float nacc = sqrtf(acc.x * acc.x + acc.y * acc.y + acc.z * acc.z) + 1e-10f;
  xp = v3(acc.x / nacc, acc.y / nacc, acc.z / nacc);
  yp = cross(xp, zp);
}

// Ball query + frame of one centre, the eigen-solve on wave-uniform data (the exact-fp32 kernel below).
template <typename NT>
__device__ __forceinline__ int pe_centre_frame(const float *sx, const float *sy, const float *sz, int N, int S,
                                               float radius, float r2, int lane, float cx, float cy, float cz,
                                               NT *nbr, Vec3 &xp, Vec3 &yp, Vec3 &zp) {
  const int cnt = lrf_ball_query<NT, int>(sx, sy, sz, N, S, r2, lane, cx, cy, cz, nbr, nullptr, -1, LrfGrid{}, false);
  float a00, a01, a02, a11, a12, a22;
  lrf_covariance(sx, sy, sz, S, lane, cx, cy, cz, nbr, a00, a01, a02, a11, a12, a22);
  Vec3 e0, e1, z0;
  float l0, l1, l2;
  eig_sym3(a00, a01, a02, a11, a12, a22, e0, e1, z0, l0, l1, l2);
  pe_frame_axes(sx, sy, sz, S, radius, lane, cx, cy, cz, nbr, z0, xp, yp, zp);
  return cnt;
}

// The max-pool's last step for one accumulator register: the maximum over the 32 neighbour lanes of each half-wave (lanes 31 / 63
// hold it) goes to the stage slot of the register's channel.
__device__ __forceinline__ void pe_pool_neighbours(float v, float *slot, int col) {
  v = fmaxf(v, dpp_f32<0x111, 0xF>(v, 0.f));
  v = fmaxf(v, dpp_f32<0x112, 0xF>(v, 0.f));
  v = fmaxf(v, dpp_f32<0x114, 0xF>(v, 0.f));
  v = fmaxf(v, dpp_f32<0x118, 0xF>(v, 0.f));
  v = fmaxf(v, dpp_f32<0x142, 0xA>(v, 0.f));  // row_bcast:15 into rows 1 and 3
  if (col == 31) *slot = v;
}

struct PeLds {
  // weights transposed to [k][out] so that lanes (l & 31) read consecutive floats
  float w1[6 * 32];
  float w2[32 * 64];
  float w3[64 * 128];
  float b1[32], b2[64], b3[128];
};

__global__ __launch_bounds__(256) void pe_group_mlp_max_kernel(
    const float *__restrict__ xyz, int N, float radius, int S, int cpw, const float *__restrict__ w1,
    const float *__restrict__ b1, const float *__restrict__ w2, const float *__restrict__ b2,
    const float *__restrict__ w3, const float *__restrict__ b3, float *__restrict__ out) {
  extern __shared__ float4 smem4[];
  PeLds *L = reinterpret_cast<PeLds *>(smem4);
  float *sx = reinterpret_cast<float *>(L + 1);
  float *sy = sx + N, *sz = sy + N;
  int *nbr_all = reinterpret_cast<int *>(sz + N);
  float *stage_all = reinterpret_cast<float *>(nbr_all + 4 * S);  // [4 waves][128]
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5, col = lane & 31;
  int *nbr = nbr_all + wave * S;
  float *stage = stage_all + wave * 128;
  const float *P = xyz + (size_t)b * N * 3;

  for (int e = tid; e < N * 3; e += 256) lrf_stage_coord(sx, sy, sz, e, P[e]);
  // weights arrive row-major [out][in] (BN already folded): transpose to [in][out]
  for (int e = tid; e < 32 * 6; e += 256) L->w1[(e % 6) * 32 + e / 6] = w1[e];
  for (int e = tid; e < 64 * 32; e += 256) L->w2[(e % 32) * 64 + e / 32] = w2[e];
  for (int e = tid; e < 128 * 64; e += 256) L->w3[(e % 64) * 128 + e / 64] = w3[e];
  if (tid < 32) L->b1[tid] = b1[tid];
  if (tid < 64) L->b2[tid] = b2[tid];
  if (tid < 128) L->b3[tid] = b3[tid];
  __syncthreads();
  const float r2 = radius * radius;

  for (int ci = 0; ci < cpw; ++ci) {
    const int j = (blockIdx.x * 4 + wave) * cpw + ci;
    if (j >= N) break;  // wave-uniform
    const float cx = sx[j], cy = sy[j], cz = sz[j];
    Vec3 xp, yp, zp;
    const int cnt_nb = pe_centre_frame(sx, sy, sz, N, S, radius, r2, lane, cx, cy, cz, nbr, xp, yp, zp);
    // Neighbour-list entries past the `cnt` points inside the radius are copies of the FIRST neighbour (ball_query_gpu.cu:14-49): their
    // MLP rows equal row 0's and cannot change the maximum -- tiles that hold nothing but such copies are skipped (bit-identical result).
    // The frame above is computed over all S entries, copies included, as the reference does.
    const int S_eff = min(S, (max(min(cnt_nb, S), 1) + 31) & ~31);  // (no point inside the radius -- a NaN centre: the list is S copies of point 0, run one tile like the reference)

    // ---- MLP over tiles of 32 neighbours, running max over tiles
    f32x16 rmax[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) rmax[t][r] = 0.f;  // post-ReLU values are >= 0
    for (int t0 = 0; t0 < S_eff; t0 += 32) {
      const int k = nbr[t0 + col];
      const float dx = sx[k] - cx, dy = sy[k] - cy, dz = sz[k] - cz;
      const Vec3 q = v3(dx / radius, dy / radius, dz / radius);
      const float lx = dot(xp, q), ly = dot(yp, q), lz = dot(zp, q);
      // layer 1: K = 6 -> 3 MFMA steps; step s contracts features (2s | 2s+1) on (lower | upper) half
      f32x16 h1;
#pragma unroll
      for (int r = 0; r < 16; ++r) h1[r] = 0.f;
      h1 = __builtin_amdgcn_mfma_f32_32x32x2f32(L->w1[(0 + half) * 32 + col], half ? dy : dx, h1, 0, 0, 0);
      h1 = __builtin_amdgcn_mfma_f32_32x32x2f32(L->w1[(2 + half) * 32 + col], half ? lx : dz, h1, 0, 0, 0);
      h1 = __builtin_amdgcn_mfma_f32_32x32x2f32(L->w1[(4 + half) * 32 + col], half ? lz : ly, h1, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 16; ++r) h1[r] = fmaxf(h1[r] + L->b1[cd_row(r, half)], 0.f);
      // layer 2: 32 -> 64 (2 output tiles); step r contracts channels cd_row(r,0) | cd_row(r,1)
      f32x16 h2[2];
#pragma unroll
      for (int ot = 0; ot < 2; ++ot) {
#pragma unroll
        for (int r = 0; r < 16; ++r) h2[ot][r] = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r)
          h2[ot] = __builtin_amdgcn_mfma_f32_32x32x2f32(L->w2[cd_row(r, half) * 64 + ot * 32 + col], h1[r], h2[ot], 0,
                                                       0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) h2[ot][r] = fmaxf(h2[ot][r] + L->b2[ot * 32 + cd_row(r, half)], 0.f);
      }
      // layer 3: 64 -> 128 (4 output tiles, 2 input tiles)
#pragma unroll
      for (int ot = 0; ot < 4; ++ot) {
        f32x16 h3;
#pragma unroll
        for (int r = 0; r < 16; ++r) h3[r] = 0.f;
#pragma unroll
        for (int it = 0; it < 2; ++it)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            h3 = __builtin_amdgcn_mfma_f32_32x32x2f32(L->w3[(it * 32 + cd_row(r, half)) * 128 + ot * 32 + col],
                                                      h2[it][r], h3, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r)
          rmax[ot][r] = fmaxf(rmax[ot][r], fmaxf(h3[r] + L->b3[ot * 32 + cd_row(r, half)], 0.f));
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) pe_pool_neighbours(rmax[t][r], &stage[t * 32 + cd_row(r, half)], col);
    wave_lds_handover();
    float *O = out + ((size_t)b * N + j) * 128;
    O[lane] = stage[lane];
    O[lane + 64] = stage[lane + 64];
    __builtin_amdgcn_wave_barrier();
  }
}

// ------------------------------------------------------------------------------------------------
// bf16 hi/lo-split variant: the same three layers on v_mfma_f32_32x32x16_bf16 with both operands split
// into hi + lo bf16 parts (a*b ~ a_hi*b_hi + a_hi*b_lo + a_lo*b_hi, ~2^-16 relative error, fp32
// accumulation): 3 bf16 MFMAs replace 8 fp32 MFMAs.  Layer chaining without data movement as above:
// accumulator registers 8s..8s+7 of a 32x32 C/D tile hold, per half-wave hb, the channels
// 16s + (e&3) + 8(e>>2) + 4hb (e = 0..7) -- exactly one 16-wide k-step of the next layer -- so the
// weights are stored with their input channels permuted to k' = 16s + 8hb + e.
__device__ __forceinline__ int pe_kperm(int c) {  // input channel -> position in the permuted k order
  const int cc = c & 15;
  return (c & ~15) + ((cc >> 2) & 1) * 8 + (cc & 3) + 4 * (cc >> 3);
}

struct PeLdsB {
  u16 w1h[32][24], w1l[32][24];   // K padded 6 -> 16 (+8 pad)
  u16 w2h[64][40], w2l[64][40];   // K = 32 (+8 pad)
  u16 w3h[128][64], w3l[128][64]; // K = 64, 16-byte slots XOR-swizzled by (row & 7)
  float b1[32], b2[64], b3[128];
};

// One-time packing of the folded fp32 weights into the LDS image of the bf16x3 kernel.
__global__ __launch_bounds__(256) void pe_pack_weights_kernel(const float *__restrict__ w1, const float *__restrict__ b1,
                                                              const float *__restrict__ w2, const float *__restrict__ b2,
                                                              const float *__restrict__ w3, const float *__restrict__ b3,
                                                              PeLdsB *__restrict__ L) {
  const int tid = threadIdx.x;
  for (int e = tid; e < 32 * 16; e += 256) {
    const int o = e >> 4, kk = e & 15;
    const float v = kk < 6 ? w1[o * 6 + kk] : 0.f;
    const u16 h = f2bf(v);
    L->w1h[o][kk] = h;
    L->w1l[o][kk] = f2bf(v - bf2f(h));
  }
  for (int e = tid; e < 64 * 32; e += 256) {
    const int o = e >> 5, c = e & 31;
    const float v = w2[e];
    const u16 h = f2bf(v);
    L->w2h[o][pe_kperm(c)] = h;
    L->w2l[o][pe_kperm(c)] = f2bf(v - bf2f(h));
  }
  for (int e = tid; e < 128 * 64; e += 256) {
    const int o = e >> 6, c = e & 63;
    const float v = w3[e];
    const u16 h = f2bf(v);
    const int kp = pe_kperm(c) ^ ((o & 7) << 3);  // swizzle the 8-element (16-byte) slot
    L->w3h[o][kp] = h;
    L->w3l[o][kp] = f2bf(v - bf2f(h));
  }
  if (tid < 32) L->b1[tid] = b1[tid];
  if (tid < 64) L->b2[tid] = b2[tid];
  if (tid < 128) L->b3[tid] = b3[tid];
}

// ------------------------------------------------------------------------------------------------
// The geometry of the bf16x3 path in a kernel of its own: neighbour lists, counts and frames of every centre, for ONE scale or for
// the TWO scales of the positional encoding in one visit (the narrow scale's list is the wide one's filtered, exactly as the
// cand_in hand-off).  No weight image in LDS and eight waves per workgroup: the VALU- and latency-bound ball query / list / frame passes run
// at up to six waves per SIMD instead of the MLP kernel's two, and the cloud's grid is built once per workgroup for both scales.
// The 3 x 3 eigen-solve is the one piece that is NOT wave-collective any more: a wave first builds the lists and covariances of a
// batch of PE_GB of its centres (lists kept in LDS), lane i keeping centre i's wide-scale matrix and lane PE_GB + i its narrow-scale
// one, calls eig_sym3 ONCE with per-lane data (every lane runs exactly its own sweep count; lanes without a problem hold the zero
// matrix and leave at the first test), and then finishes the batch's frames with the wave-collective vote / x-axis passes.  The
// operations of every problem are those of the fused kernel; only who executes them changed.
constexpr int PE_GW = 8;  // waves per workgroup
constexpr int PE_GB = 4;  // centres per eigen-solve batch of a wave (measured at 32 x 2048, both scales: 4 centres per wave in one batch 171 us,
                          // 8 per wave in batches of 4 / 8: 179 / 183 us, 16 per wave in batches of 8: 189 us -- shorter waves balance better)
constexpr int PE_GEOM_SCRATCH = PE_GCELLS + 6 * PE_GW + PE_GW;  // 4-byte words of the grid build's scratch

__device__ __forceinline__ float pe_readlane_f32(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

__global__ __launch_bounds__(PE_GW * 64) void pe_geometry_kernel(
    const float *__restrict__ xyz, int N, int cpw, float rad0, int S0, float rad1, int S1, const int *__restrict__ cand_in,
    const int *__restrict__ cand_cnt_in, int cand_stride, u16 *__restrict__ lists0, int *__restrict__ cnt0,
    float *__restrict__ frames0, int *__restrict__ cand_out, u16 *__restrict__ lists1, int *__restrict__ cnt1,
    float *__restrict__ frames1, int use_grid) {
  extern __shared__ float4 smem4[];
  float *sx = reinterpret_cast<float *>(smem4);
  float *sy = sx + N, *sz = sy + N;
  const int BW = use_grid ? (N + 31) >> 5 : 0;                 // words of a wave's bit map
  uint32_t *bits_all = reinterpret_cast<uint32_t *>(sz + N);  // [PE_GW][BW] bit maps
  u16 *lists_all = reinterpret_cast<u16 *>(bits_all + PE_GW * BW);  // [PE_GW][PE_GB][S0 + S1] neighbour lists of a batch
  // the grid build's scratch borrows the lists' area (the host sizes it for both): cell counters / fill cursors, partial extrema, wave totals
  uint32_t *cnt32 = reinterpret_cast<uint32_t *>(lists_all);  // [PE_GCELLS]
  float *red = reinterpret_cast<float *>(cnt32 + PE_GCELLS);  // [6 PE_GW]
  uint32_t *wtot = reinterpret_cast<uint32_t *>(red + 6 * PE_GW);  // [PE_GW]
  const int SS = S0 + S1;
  u16 *gstart = lists_all + max(PE_GW * PE_GB * SS, 2 * PE_GEOM_SCRATCH);  // grid (use_grid): [PE_GCELLS + 2] cell starts, then [N] point ids by cell
  u16 *gorder = gstart + PE_GCELLS + 2;
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const float *P = xyz + (size_t)b * N * 3;

  for (int e = tid; e < N * 3; e += PE_GW * 64) lrf_stage_coord(sx, sy, sz, e, P[e]);
  __syncthreads();
  LrfGrid grid = {};
  if (use_grid) {
    // ---- the cloud's grid (cells of the WIDE radius serve both scales: a cell edge only has to be >= the radius queried)
    float lo[3] = {3e38f, 3e38f, 3e38f}, hi[3] = {-3e38f, -3e38f, -3e38f};
    for (int p = tid; p < N; p += PE_GW * 64) {
      lo[0] = fminf(lo[0], sx[p]), hi[0] = fmaxf(hi[0], sx[p]);
      lo[1] = fminf(lo[1], sy[p]), hi[1] = fmaxf(hi[1], sy[p]);
      lo[2] = fminf(lo[2], sz[p]), hi[2] = fmaxf(hi[2], sz[p]);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      lo[a] = -wave_max_f32(-lo[a]);
      hi[a] = wave_max_f32(hi[a]);
      if (lane == 0) red[wave * 6 + a] = lo[a], red[wave * 6 + 3 + a] = hi[a];
    }
    for (int c = tid; c < PE_GCELLS; c += PE_GW * 64) cnt32[c] = 0u;
    __syncthreads();
    float org[3], ih[3];
    int nd[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      float l = red[a], h = red[3 + a];
      for (int w = 1; w < PE_GW; ++w) l = fminf(l, red[w * 6 + a]), h = fmaxf(h, red[w * 6 + 3 + a]);
      const float ext = h - l, h0 = rad0 * 1.001f;  // (cells a little wider than the radius: a neighbour is at most ONE cell away under fp rounding)
      int n = (int)(ext / h0) + 1;
      float edge = h0;
      if (!(n <= PE_GDIM)) n = PE_GDIM, edge = fmaxf(h0, ext / (float)PE_GDIM * 1.001f);
      // (the same in every lane: kept in scalar registers)
      org[a] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(l)));
      ih[a] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(1.f / edge)));
      nd[a] = __builtin_amdgcn_readfirstlane(max(n, 1));
    }
    grid.ox = org[0], grid.oy = org[1], grid.oz = org[2], grid.ihx = ih[0], grid.ihy = ih[1], grid.ihz = ih[2];
    grid.nx = nd[0], grid.ny = nd[1], grid.nz = nd[2];
    grid.start = gstart, grid.order = gorder, grid.bits = bits_all + wave * BW;
    auto cell_of = [&](int p) {
      return (lrf_cell(sz[p], grid.oz, grid.ihz, grid.nz) * grid.ny + lrf_cell(sy[p], grid.oy, grid.ihy, grid.ny)) * grid.nx +
             lrf_cell(sx[p], grid.ox, grid.ihx, grid.nx);
    };
    for (int p = tid; p < N; p += PE_GW * 64) atomicAdd(&cnt32[cell_of(p)], 1u);
    __syncthreads();
    {  // exclusive scan of the PE_GCELLS counters: one cell per thread (of the first PE_GCELLS), wave scan, wave totals through LDS
      static_assert(PE_GW * 64 >= PE_GCELLS && PE_GCELLS % 64 == 0, "one cell per thread");
      const uint32_t c = tid < PE_GCELLS ? cnt32[tid] : 0u;
      const uint32_t incl = wave_inclusive_sum(c, lane);
      if (lane == 63) wtot[wave] = incl;
      __syncthreads();
      if (tid < PE_GCELLS) {
        uint32_t base = incl - c;
        for (int w = 0; w < wave; ++w) base += wtot[w];
        gstart[tid] = (u16)base;
        cnt32[tid] = base;  // the fill pass's cursor
        if (tid == PE_GCELLS - 1) gstart[PE_GCELLS] = (u16)(base + c);
      }
    }
    __syncthreads();
    for (int p = tid; p < N; p += PE_GW * 64) gorder[atomicAdd(&cnt32[cell_of(p)], 1u)] = (u16)p;
    __syncthreads();
  }
  const float r2_0 = rad0 * rad0, r2_1 = rad1 * rad1;
  u16 *mylists = lists_all + wave * PE_GB * SS;
  const int jbase = (blockIdx.x * PE_GW + wave) * cpw;

  for (int c0 = 0; c0 < cpw; c0 += PE_GB) {
    if (jbase + c0 >= N) break;  // wave-uniform
    const int nb = min(PE_GB, min(cpw - c0, N - jbase - c0));  // centres of this batch
    float m00 = 0.f, m01 = 0.f, m02 = 0.f, m11 = 0.f, m12 = 0.f, m22 = 0.f;  // this LANE's eigen-problem
#pragma unroll 1
    for (int i = 0; i < nb; ++i) {
      const int j = jbase + c0 + i;
      const size_t row = (size_t)b * N + j;
      const float cx = sx[j], cy = sy[j], cz = sz[j];
      u16 *n0 = mylists + i * SS, *n1 = n0 + S0;
      const int *cand = nullptr;
      int ncand = -1;
      if (cand_in) {
        ncand = cand_cnt_in[row];  // -1: the producer's list overflowed, scan everything
        cand = cand_in + row * cand_stride;
      }
      const int c = lrf_ball_query<u16, int>(sx, sy, sz, N, S0, r2_0, lane, cx, cy, cz, n0, cand, ncand, grid, use_grid != 0);
      {
        uint32_t *dst = reinterpret_cast<uint32_t *>(lists0 + row * S0);
        const uint32_t *src = reinterpret_cast<const uint32_t *>(n0);
        for (int l = lane; l < (S0 >> 1); l += 64) dst[l] = src[l];
        if (cand_out) {
          int *co = cand_out + row * S0;
          for (int l = lane; l < S0; l += 64) co[l] = n0[l];
        }
        if (lane == 0) cnt0[row] = c <= S0 ? c : -1;
      }
      float a00, a01, a02, a11, a12, a22;
      lrf_covariance(sx, sy, sz, S0, lane, cx, cy, cz, n0, a00, a01, a02, a11, a12, a22);
      if (lane == i) m00 = a00, m01 = a01, m02 = a02, m11 = a11, m12 = a12, m22 = a22;
      if (S1) {
        // the narrow scale tests the wide list's points (all of them lie in it) unless that list overflowed
        const int c1 = lrf_ball_query<u16, u16>(sx, sy, sz, N, S1, r2_1, lane, cx, cy, cz, n1, n0, c <= S0 ? c : -1, grid, use_grid != 0);
        uint32_t *dst = reinterpret_cast<uint32_t *>(lists1 + row * S1);
        const uint32_t *src = reinterpret_cast<const uint32_t *>(n1);
        for (int l = lane; l < (S1 >> 1); l += 64) dst[l] = src[l];
        if (lane == 0) cnt1[row] = c1 <= S1 ? c1 : -1;
        lrf_covariance(sx, sy, sz, S1, lane, cx, cy, cz, n1, a00, a01, a02, a11, a12, a22);
        if (lane == PE_GB + i) m00 = a00, m01 = a01, m02 = a02, m11 = a11, m12 = a12, m22 = a22;
      }
    }
    Vec3 e0, e1, z0;
    float l0, l1, l2;
    eig_sym3(m00, m01, m02, m11, m12, m22, e0, e1, z0, l0, l1, l2);
#pragma unroll 1
    for (int i = 0; i < nb; ++i) {
      const int j = jbase + c0 + i;
      const size_t row = (size_t)b * N + j;
      const float cx = sx[j], cy = sy[j], cz = sz[j];
      const u16 *n0 = mylists + i * SS, *n1 = n0 + S0;
#pragma unroll 1
      for (int sc = 0; sc < (S1 ? 2 : 1); ++sc) {
        const int src_lane = sc ? PE_GB + i : i;
        const Vec3 z = v3(pe_readlane_f32(z0.x, src_lane), pe_readlane_f32(z0.y, src_lane), pe_readlane_f32(z0.z, src_lane));
        Vec3 xp, yp, zp;
        pe_frame_axes(sx, sy, sz, sc ? S1 : S0, sc ? rad1 : rad0, lane, cx, cy, cz, sc ? n1 : n0, z, xp, yp, zp);
        const float f = lane == 0 ? xp.x : lane == 1 ? xp.y : lane == 2 ? xp.z : lane == 3 ? yp.x : lane == 4 ? yp.y : lane == 5 ? yp.z
                        : lane == 6 ? zp.x : lane == 7 ? zp.y : zp.z;
        if (lane < 9) (sc ? frames1 : frames0)[row * 9 + lane] = f;
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// The MLP of the bf16x3 path: list, count and frame of every centre come from pe_geometry_kernel; the tile loop is the fused
// kernel's.  A centre's list (S 16-bit ids), frame and count are fetched into registers one centre ahead, under the previous
// centre's tiles.
constexpr int PE_NW = 4;  // waves per workgroup of the bf16x3 kernel: two 4-wave workgroups per CU; 8 = one per CU (measured 4 % slower)
__global__ __launch_bounds__(PE_NW * 64, 8 / PE_NW) void pe_group_mlp_max_bf16x3_kernel(
    const float *__restrict__ xyz, int N, float radius, int S, int cpw, const uint4 *__restrict__ image,
    const u16 *__restrict__ lists, const int *__restrict__ counts, const float *__restrict__ frames, float *__restrict__ out,
    int out_ld, int out_split) {
  extern __shared__ float4 smem4[];
  PeLdsB *L = reinterpret_cast<PeLdsB *>(smem4);
  float *sx = reinterpret_cast<float *>(L + 1);
  float *sy = sx + N, *sz = sy + N;
  float *stage_all = sz + N;                                           // [PE_NW][128] floats
  u16 *nbr_all = reinterpret_cast<u16 *>(stage_all + PE_NW * 128);    // [PE_NW][S] neighbour lists (N < 65536)
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5, col = lane & 31;
  u16 *nbr = nbr_all + wave * S;
  float *stage = stage_all + wave * 128;
  const float *P = xyz + (size_t)b * N * 3;
  const int SW = S >> 1;  // list length in 4-byte words
  const uint32_t *LW = reinterpret_cast<const uint32_t *>(lists) + (size_t)b * N * SW;
  uint32_t pw0 = 0u, pw1 = 0u;  // the next centre's list words lane, lane + 64
  float pf = 0.f;               // lanes 0..8: its frame; lane 9: its count
  auto fetch = [&](int j) {
    const uint32_t *p = LW + (size_t)j * SW;
    pw0 = lane < SW ? p[lane] : 0u;
    pw1 = lane + 64 < SW ? p[lane + 64] : 0u;
    const size_t row = (size_t)b * N + j;
    pf = lane < 9 ? frames[row * 9 + lane] : lane == 9 ? __int_as_float(counts[row]) : 0.f;
  };
  const int j0 = (blockIdx.x * PE_NW + wave) * cpw;
  if (j0 < N) fetch(j0);

  for (int e = tid; e < N * 3; e += PE_NW * 64) lrf_stage_coord(sx, sy, sz, e, P[e]);
  // the LDS weight image (hi/lo bf16, permuted, swizzled; built once by pe_pack_weights_kernel) is copied
  // verbatim with coalesced 16-byte loads
  for (int e = tid; e < (int)(sizeof(PeLdsB) / 16); e += PE_NW * 64) smem4[e] = *reinterpret_cast<const float4 *>(image + e);
  __syncthreads();

  for (int ci = 0; ci < cpw; ++ci) {
    const int j = j0 + ci;
    if (j >= N) break;  // wave-uniform
    const float cx = sx[j], cy = sy[j], cz = sz[j];
    {
      uint32_t *nw = reinterpret_cast<uint32_t *>(nbr);
      if (lane < SW) nw[lane] = pw0;
      if (lane + 64 < SW) nw[lane + 64] = pw1;
      for (int l = lane + 128; l < SW; l += 64) nw[l] = LW[(size_t)j * SW + l];  // (lists longer than 256: not fetched ahead)
    }
    const Vec3 xp = v3(pe_readlane_f32(pf, 0), pe_readlane_f32(pf, 1), pe_readlane_f32(pf, 2));
    const Vec3 yp = v3(pe_readlane_f32(pf, 3), pe_readlane_f32(pf, 4), pe_readlane_f32(pf, 5));
    const Vec3 zp = v3(pe_readlane_f32(pf, 6), pe_readlane_f32(pf, 7), pe_readlane_f32(pf, 8));
    const int cnt_in = __builtin_amdgcn_readlane(__float_as_int(pf), 9);
    const int cnt = cnt_in < 0 ? S + 1 : cnt_in;  // -1: more points inside the radius than the list holds
    wave_lds_handover();
    if (ci + 1 < cpw && j + 1 < N) fetch(j + 1);

    f32x16 rmax[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) rmax[t][r] = 0.f;  // post-ReLU values are >= 0
    // (tiles of nothing but copies of the first neighbour -- the padding of a list with fewer than S points inside the radius -- are
    //  skipped: their rows equal row 0's, the maximum cannot change; round 5)
    const int S_eff = min(S, (max(min(cnt, S), 1) + 31) & ~31);  // (cnt == 0, a NaN centre: one tile of the all-point-0 list, like the reference)
    for (int t0 = 0; t0 < S_eff; t0 += 32) {
      // keep the weight fragments in LDS (re-read per tile) instead of letting the compiler hoist ~170
      // registers of loop-invariant operands: leaves room for 2 waves / SIMD so one wave's VALU phases
      // (ball query, frame, hi/lo splits) overlap the other's MFMAs
      asm volatile("" ::: "memory");
      const int k = nbr[t0 + col];
      const float dx = sx[k] - cx, dy = sy[k] - cy, dz = sz[k] - cz;
      const Vec3 q = v3(dx / radius, dy / radius, dz / radius);
      float f[8] = {dx, dy, dz, dot(xp, q), dot(yp, q), dot(zp, q), 0.f, 0.f};
      if (half) {
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = 0.f;  // k' 8..15 of the padded first layer
      }
      const bf16x8_hl x = split8_bf16(f);
      // The weight fragments and bias values of the NEXT group of MFMAs are read from LDS (into the other of two register sets) before
      // the current group is issued: left to the compiler every k-step's two fragments were read right in front of their three MFMAs
      // -- ~20 exposed LDS round trips per tile (round 4: the tile loop was latency-bound, the matrix pipe 36 % busy).
      struct Grp {
        bf16x8_hl w[4];
        float4 b[4];
      } ga, gb;
      auto load_l1 = [&](Grp &g) {
        g.w[0].hi = *reinterpret_cast<const bf16x8 *>(&L->w1h[col][half * 8]);
        g.w[0].lo = *reinterpret_cast<const bf16x8 *>(&L->w1l[col][half * 8]);
#pragma unroll
        for (int q = 0; q < 4; ++q) g.b[q] = *reinterpret_cast<const float4 *>(&L->b1[8 * q + 4 * half]);
      };
      auto load_l2 = [&](Grp &g, int ot) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          g.w[ks].hi = *reinterpret_cast<const bf16x8 *>(&L->w2h[ot * 32 + col][ks * 16 + half * 8]);
          g.w[ks].lo = *reinterpret_cast<const bf16x8 *>(&L->w2l[ot * 32 + col][ks * 16 + half * 8]);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) g.b[q] = *reinterpret_cast<const float4 *>(&L->b2[ot * 32 + 8 * q + 4 * half]);
      };
      auto load_l3 = [&](Grp &g, int ot) {
        const int row = ot * 32 + col;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const int kp = (ks * 16 + half * 8) ^ ((row & 7) << 3);
          g.w[ks].hi = *reinterpret_cast<const bf16x8 *>(&L->w3h[row][kp]);
          g.w[ks].lo = *reinterpret_cast<const bf16x8 *>(&L->w3l[row][kp]);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) g.b[q] = *reinterpret_cast<const float4 *>(&L->b3[ot * 32 + 8 * q + 4 * half]);
      };
      auto init = [&](f32x16 &h, const Grp &g) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          h[4 * q + 0] = g.b[q].x;
          h[4 * q + 1] = g.b[q].y;
          h[4 * q + 2] = g.b[q].z;
          h[4 * q + 3] = g.b[q].w;
        }
      };
      bf16x8_hl a1[2], a2[4];
      auto relu_split = [&](const f32x16 &h, bf16x8_hl *o) {
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          float v[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = fmaxf(h[s2 * 8 + e], 0.f);
          o[s2] = split8_bf16(v);
        }
      };
      load_l1(ga);
      load_l2(gb, 0);
      __builtin_amdgcn_sched_barrier(0);
      {
        f32x16 h1;
        init(h1, ga);
        h1 = mfma3_hh_hl_lh_32x32(ga.w[0], x, h1);
        load_l2(ga, 1);
        __builtin_amdgcn_sched_barrier(0);
        relu_split(h1, a1);
      }
      {
        f32x16 h2;
        init(h2, gb);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) h2 = mfma3_hh_hl_lh_32x32(gb.w[ks], a1[ks], h2);
        load_l3(gb, 0);
        __builtin_amdgcn_sched_barrier(0);
        relu_split(h2, a2);
        init(h2, ga);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) h2 = mfma3_hh_hl_lh_32x32(ga.w[ks], a1[ks], h2);
        load_l3(ga, 1);
        __builtin_amdgcn_sched_barrier(0);
        relu_split(h2, a2 + 2);
      }
#pragma unroll
      for (int ot = 0; ot < 4; ++ot) {
        Grp &g = (ot & 1) ? ga : gb;
        // (measured and not kept: b3 + ReLU once per centre after the loop -- max_k relu(h_k + b) = relu(max_k h_k + b) -- with the
        // accumulator starting from the inline constant 0: 2021 -> 2101 us at S = 256, 1036 -> 1139 us at S = 64)
        f32x16 h3;
        init(h3, g);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) h3 = mfma3_hh_hl_lh_32x32(g.w[ks], a2[ks], h3);
        if (ot + 2 < 4) {
          load_l3(g, ot + 2);  // (into the set the MFMAs above have just read: the hardware keeps the order)
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) rmax[ot][r] = fmaxf(rmax[ot][r], h3[r]);
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) pe_pool_neighbours(rmax[t][r], &stage[t * 32 + cd_row(r, half)], col);
    wave_lds_handover();
    float *O = out + ((size_t)b * N + j) * out_ld;
    if (!out_split) {
      O[lane] = stage[lane];
      O[lane + 64] = stage[lane + 64];
    } else {
      // split layout of csrc/gemm_f32.hip: 32-channel blocks of 128 bytes [hi (32 x bf16) | lo (32 x bf16)]; this scale's 128
      // channels are 4 blocks = 128 dwords, two per lane
      uint32_t *O32 = reinterpret_cast<uint32_t *>(O);
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int d = lane + 64 * q, blk = d >> 5, w = d & 31, k = blk * 32 + (w & 15) * 2;
        const float v0 = stage[k], v1 = stage[k + 1];
        const uint32_t h = cvt_pk_bf16_f32(v0, v1);
        O32[d] = (w & 16) ? cvt_pk_bf16_lo(v0, v1, h) : h;
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
}

}  // namespace unopose

using namespace unopose;

extern "C" {

int unopose_pe_image_bytes(void) { return (int)sizeof(PeLdsB); }

int unopose_pe_pack_weights(const float *w1, const float *b1, const float *w2, const float *b2, const float *w3,
                            const float *b3, void *image, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(w1 && b1 && w2 && b2 && w3 && b3 && image, "pe_pack_weights: null pointer");
  hipLaunchKernelGGL(pe_pack_weights_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, w1, b1, w2, b2, w3, b3,
                     (PeLdsB *)image);
  return check_launch("pe_pack_weights");
}

int unopose_pe_geometry(const float *xyz, int B, int N, float radius, int nsample, float radius2, int nsample2,
                        const int *cand_in, const int *cand_cnt_in, int cand_stride, void *lists, int *counts, float *frames,
                        int *cand_out, void *lists2, int *counts2, float *frames2, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(xyz && lists && counts && frames, "pe_geometry: null pointer");
  UNOPOSE_REQUIRE((cand_in == nullptr) == (cand_cnt_in == nullptr) && (!cand_in || cand_stride >= 1),
                  "pe_geometry: candidate list and its counts go together");
  UNOPOSE_REQUIRE(B >= 0 && N >= 1 && nsample >= 32 && nsample % 32 == 0 && nsample2 >= 0 && nsample2 % 32 == 0 && B <= 65535,
                  "pe_geometry: nsample must be a positive multiple of 32 (got %d, %d)", nsample, nsample2);
  UNOPOSE_REQUIRE(nsample2 == 0 || (lists2 && counts2 && frames2 && radius2 <= radius),
                  "pe_geometry: the second scale needs its outputs and a radius no larger than the first's");
  if (B == 0) return UNOPOSE_OK;
  // cloud (3 N floats) + the 16-bit lists of a batch (the grid build's scratch borrows their area); with the ball query's grid, the
  // waves' bit maps and the grid itself (cell starts + the cell-sorted point ids).  The grid takes clouds of 256..4096 points.
  const size_t lists_bytes = (size_t)2 * std::max(PE_GW * PE_GB * (nsample + nsample2), 2 * PE_GEOM_SCRATCH);
  size_t lds = (size_t)3 * N * 4 + lists_bytes;
  const size_t grid_bytes = ((size_t)PE_GCELLS + 2 + (size_t)N) * 2 + (size_t)PE_GW * ((N + 31) >> 5) * 4;
  UNOPOSE_REQUIRE(N < 65536 && lds <= 160 * 1024, "pe_geometry: N=%d nsample=%d+%d exceed the LDS tile", N, nsample, nsample2);
  const int use_grid = radius > 0.f && N <= 4096 && N >= 256 && lds + grid_bytes <= 160 * 1024;
  if (use_grid) lds += grid_bytes;
  lds = (lds + 15) & ~(size_t)15;
  static bool opt[64];
  if (lds_optin(opt, (const void *)pe_geometry_kernel, 160 * 1024, "pe_geometry") != UNOPOSE_OK) return UNOPOSE_ELAUNCH;
  const long centres = (long)B * N;
  const int cpw = centres >= 16384 ? PE_GB : centres >= 8192 ? 2 : 1;
  dim3 grid(cdiv(N, PE_GW * cpw), B);
  hipLaunchKernelGGL(pe_geometry_kernel, grid, dim3(PE_GW * 64), lds, (hipStream_t)stream, xyz, N, cpw, radius, nsample, radius2,
                     nsample2, cand_in, cand_cnt_in, cand_stride, (u16 *)lists, counts, frames, cand_out, (u16 *)lists2, counts2,
                     frames2, use_grid);
  return check_launch("pe_geometry");
}

int unopose_pe_mlp_max_packed(const float *xyz, int B, int N, float radius, int nsample, const void *image, const void *lists,
                              const int *counts, const float *frames, void *out, int out_ld, int out_split,
                              unopose_stream_t stream) {
  UNOPOSE_REQUIRE(xyz && image && lists && counts && frames && out, "pe_mlp_max_packed: null pointer");
  UNOPOSE_REQUIRE(out_ld >= 128 && (out_split == 0 || out_split == 1), "pe_mlp_max_packed: bad output stride / mode");
  UNOPOSE_REQUIRE(B >= 0 && N >= 1 && nsample >= 32 && nsample % 32 == 0 && B <= 65535,
                  "pe_mlp_max_packed: nsample must be a positive multiple of 32 (got %d)", nsample);
  if (B == 0) return UNOPOSE_OK;
  // weight image + cloud (3 N floats) + staging + 16-bit neighbour lists
  size_t lds = sizeof(PeLdsB) + ((size_t)3 * N + PE_NW * 128) * 4 + (size_t)PE_NW * nsample * 2;
  UNOPOSE_REQUIRE(N < 65536 && lds <= 160 * 1024, "pe_mlp_max_packed: N=%d nsample=%d exceed the LDS tile", N, nsample);
  lds = (lds + 15) & ~(size_t)15;
  static bool opt[64];
  if (lds_optin(opt, (const void *)pe_group_mlp_max_bf16x3_kernel, 160 * 1024, "pe_mlp_max_packed") != UNOPOSE_OK) return UNOPOSE_ELAUNCH;
  const long centres = (long)B * N;
  const int cpw = centres >= 65536 ? 16 : centres >= 32768 ? 8 : centres >= 8192 ? 4 : centres >= 2048 ? 2 : 1;
  dim3 grid(cdiv(N, PE_NW * cpw), B);
  hipLaunchKernelGGL(pe_group_mlp_max_bf16x3_kernel, grid, dim3(PE_NW * 64), lds, (hipStream_t)stream, xyz, N, radius, nsample,
                     cpw, (const uint4 *)image, (const u16 *)lists, counts, frames, (float *)out, out_ld, out_split);
  return check_launch("pe_mlp_max_packed");
}

int unopose_pe_group_mlp_max(const float *xyz, int B, int N, float radius, int nsample, const float *w1,
                             const float *b1, const float *w2, const float *b2, const float *w3, const float *b3,
                             int bf16x3, float *out, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(xyz && w1 && b1 && w2 && b2 && w3 && b3 && out, "pe_group_mlp_max: null pointer");
  UNOPOSE_REQUIRE(B >= 0 && N >= 1 && nsample >= 32 && nsample % 32 == 0 && B <= 65535,
                  "pe_group_mlp_max: nsample must be a positive multiple of 32 (got %d)", nsample);
  if (B == 0) return UNOPOSE_OK;
  const size_t lds = sizeof(PeLds) + ((size_t)3 * N + 4 * (size_t)nsample + 4 * 128) * 4;
  UNOPOSE_REQUIRE(lds <= 160 * 1024, "pe_group_mlp_max: N=%d nsample=%d exceed the LDS tile", N, nsample);
  static bool opt[64];
  if (lds_optin(opt, (const void *)pe_group_mlp_max_kernel, 160 * 1024, "pe_group_mlp_max") != UNOPOSE_OK) return UNOPOSE_ELAUNCH;
  const long centres = (long)B * N;
  const int cpw = centres >= 32768 ? 8 : centres >= 8192 ? 4 : centres >= 2048 ? 2 : 1;
  dim3 grid(cdiv(N, 4 * cpw), B);
  UNOPOSE_REQUIRE(!bf16x3, "pe_group_mlp_max: the bf16x3 form takes a packed weight image "
                           "(unopose_pe_pack_weights + unopose_pe_geometry + unopose_pe_mlp_max_packed)");
  hipLaunchKernelGGL(pe_group_mlp_max_kernel, grid, dim3(256), lds, (hipStream_t)stream, xyz, N, radius, nsample, cpw,
                     w1, b1, w2, b2, w3, b3, out);
  return check_launch("pe_group_mlp_max");
}

}  // extern "C"
