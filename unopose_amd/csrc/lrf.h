// The per-point local reference frame of QueryAndLRFGroup (pointnet2_utils.py:429-481, 522-584), ONE implementation for every kernel
// that builds it: geom.hip's query_lrf_group_kernel and pe.hip's fused fp32 and geometry kernels.  All pieces are wave-collective,
// one wavefront per centre over an SoA copy of the cloud in LDS:
//   lrf_stage_coord  -- the cloud's SoA copy into LDS, one float of it
//   lrf_ball_query   -- the neighbour list: the first S points inside the radius IN INDEX ORDER, empty slots padded with the first hit
//   lrf_covariance   -- the covariance of c - p_k over the padded list (the 3 x 3 eigen-solve on it is jacobi3.h's eig_sym3)
//   lrf_vote_xacc    -- the sign vote on the normal (+-1e-3 thresholds) and the x axis' accumulator, weights (r - |d|)^2 (z.d)^2
// The x axis is the accumulator over |acc| + 1e-10.  That last step is NOT here: geom.hip multiplies by the reciprocal (finish_frame),
// pe.hip divides (pe_frame_axes); see the comments there.
// This header is compiled under two flag sets on purpose: pe.hip with -fno-honor-nans, geom.hip with IEEE NaN handling.
#pragma once
#include "common.h"
#include "jacobi3.h"

namespace unopose {

constexpr int LRF_SCAN_STEPS = 4;  // 64-candidate steps of the ball query per loop trip (measured against 1 step per trip)

// Float e of the cloud (N x 3, AoS) into its SoA slot.  The loop over e stays in the kernels, which differ in their thread counts: with the
// loop in here too, the kernels' instruction streams no longer equal the ones their outputs were validated with.
__device__ __forceinline__ void lrf_stage_coord(float *sx, float *sy, float *sz, int e, float v) {
  const int p = e / 3, comp = e - p * 3;
  (comp == 0 ? sx : comp == 1 ? sy : sz)[p] = v;
}

// ---- A uniform grid for the ball query (built by pe.hip's geometry kernel).  The scan tests all N points of the cloud per centre
// although ~75 of 2048 lie inside the radius; cells of edge >= 1.001 radius (a bounded number per axis: larger clouds get larger cells)
// leave the 27 cells around the centre's, and cell ids run along x, so those are NINE contiguous runs of the cell-sorted point list:
// ~9 steps of 64 candidates instead of 32.  The reference's order (the first S hits BY INDEX) is kept exactly: hits set bits of an
// N-bit map in LDS (ds_or), and the list is read off the map in index order (popcount prefix over the lanes' words) -- same hit test
// on the same coordinates, same list, bit-identical outputs.
struct LrfGrid {
  float ox, oy, oz, ihx, ihy, ihz;  // origin, inverse cell edges
  int nx, ny, nz;
  const u16 *start;  // [cells + 1]: first slot of a cell in `order`
  const u16 *order;  // [N] point ids sorted by cell
  uint32_t *bits;    // this wave's map, ceil(N / 32) words
};
__device__ __forceinline__ int lrf_cell(float v, float o, float ih, int n) { return max(0, min(n - 1, (int)((v - o) * ih))); }

// Ball query (pointnet2 ball_query_gpu.cu:14-49 semantics) into the wave's LDS neighbour list: fills nbr[0..S), padding included.
// `cand` / `ncand`: optional list of candidate indices IN INDEX ORDER that is known to contain every point within the radius (the
// neighbour list a larger-radius pass of the same cloud wrote); ncand < 0 = scan the whole cloud.  `cand` may be a list in LDS (CT =
// u16) or in global memory (CT = int).  Returns the number of points inside the radius if the list holds them all, a value > S otherwise.
template <typename NT, typename CT>
__device__ __forceinline__ int lrf_ball_query(const float *sx, const float *sy, const float *sz, int N, int S, float r2, int lane,
                                              float cx, float cy, float cz, NT *nbr, const CT *cand, int ncand, const LrfGrid &g, bool use_grid) {
  int cnt = 0, first = 0;
  if (use_grid && ncand < 0) {
    const int W = (N + 31) >> 5;
    for (int w = lane; w < W; w += 64) g.bits[w] = 0u;
    // the nine runs: lane i < 9 looks up run (dy, dz) = (i % 3 - 1, i / 3 - 1)
    const int icx = lrf_cell(cx, g.ox, g.ihx, g.nx), icy = lrf_cell(cy, g.oy, g.ihy, g.ny),
              icz = lrf_cell(cz, g.oz, g.ihz, g.nz);
    int rs = 0, re = 0;
    if (lane < 9) {
      const int y = icy + lane % 3 - 1, z = icz + lane / 3 - 1;
      if (y >= 0 && y < g.ny && z >= 0 && z < g.nz) {
        const int row = (z * g.ny + y) * g.nx;
        rs = g.start[row + max(icx - 1, 0)];
        re = g.start[row + min(icx + 1, g.nx - 1) + 1];
      }
    }
    wave_lds_handover();
#pragma unroll 1
    for (int i = 0; i < 9; ++i) {
      const int s0 = __builtin_amdgcn_readlane(rs, i), e0 = __builtin_amdgcn_readlane(re, i);
      for (int q = s0 + lane; q < e0; q += 64) {
        const int k = g.order[q];
        const float x = sx[k], y = sy[k], z = sz[k];
        const float d2 = (cx - x) * (cx - x) + (cy - y) * (cy - y) + (cz - z) * (cz - z);
        if (d2 < r2) atomicOr(&g.bits[k >> 5], 1u << (k & 31));
      }
    }
    wave_lds_handover();
    // the list in index order: lane-owned words, exclusive prefix of their popcounts
    for (int w0 = 0; w0 < W; w0 += 64) {
      const int w = w0 + lane;
      uint32_t bits = w < W ? g.bits[w] : 0u;
      const int pc = __builtin_popcount(bits);
      const int incl = wave_inclusive_sum(pc, lane);
      int pos = cnt + incl - pc;
      while (bits) {
        const int bpos = __builtin_ctz(bits);
        bits &= bits - 1u;
        if (pos < S) nbr[pos] = (NT)(32 * w + bpos);
        ++pos;
      }
      cnt += __builtin_amdgcn_readlane(incl, 63);
    }
    wave_lds_handover();
    if (cnt > 0) first = nbr[0];
  } else {
  const int nscan = ncand >= 0 ? ncand : N;
  int k0 = 0;
  // LRF_SCAN_STEPS (four) 64-candidate steps per trip: their LDS reads, distance tests and ballots are independent, only the list positions chain
  // through cnt (one step at a time the loop was a chain of LDS -> VALU -> ballot -> scalar latencies: a third of a launch)
  constexpr int U = LRF_SCAN_STEPS;
  for (; k0 < nscan && cnt < S; k0 += 64 * U) {
    int kk[U];
    unsigned long long mask[U];
    bool hit[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      int k = k0 + 64 * u + lane;
      hit[u] = false;
      if (k < nscan) {
        if (ncand >= 0) k = cand[k];
        const float x = sx[k], y = sy[k], z = sz[k];
        const float d2 = (cx - x) * (cx - x) + (cy - y) * (cy - y) + (cz - z) * (cz - z);
        hit[u] = d2 < r2;
      }
      kk[u] = k;
      mask[u] = __ballot(hit[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (mask[u]) {
        const int pre =
            (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask[u] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask[u], 0u));
        const int pos = cnt + pre;
        if (hit[u] && pos < S) nbr[pos] = (NT)kk[u];
        if (cnt == 0) {
          const int fl = __builtin_ctzll(mask[u]);  // lane of the first hit
          first = ncand >= 0 ? __builtin_amdgcn_readlane(kk[u], fl) : k0 + 64 * u + fl;
        }
        cnt += __builtin_popcountll(mask[u]);
      }
    }
  }
  if (k0 < nscan) cnt = S + 1;  // stopped early at a full list: the rest of the cloud was not looked at
  }
  for (int l = min(cnt, S) + lane; l < S; l += 64) nbr[l] = (NT)first;  // cnt == 0 -> index 0
  wave_lds_handover();
  return cnt;
}

// ---- local reference frame (LRF_batch, pointnet2_utils.py:436-481) in three wave-collective pieces: the covariance of the list,
// the eigen-solve (eig_sym3: per centre in the fused kernels, one centre per LANE in pe.hip's geometry kernel), the sign vote and x axis.
// (measured and not kept, round 5: the three passes with the padding entries' terms as per-pass constants -- bit-identical, no faster:
//  the frame's time is the eigen-solver and the wave reductions, not these reads)
template <typename NT>
__device__ __forceinline__ void lrf_covariance(const float *sx, const float *sy, const float *sz, int S, int lane, float cx, float cy,
                                               float cz, const NT *nbr, float &a00, float &a01, float &a02, float &a11, float &a12,
                                               float &a22) {
  a00 = 0, a01 = 0, a02 = 0, a11 = 0, a12 = 0, a22 = 0;
  for (int l = lane; l < S; l += 64) {
    const int k = nbr[l];
    const float x = cx - sx[k], y = cy - sy[k], z = cz - sz[k];
    a00 += x * x; a01 += x * y; a02 += x * z; a11 += y * y; a12 += y * z; a22 += z * z;
  }
  const float inv_s = 1.f / (float)S;
  a00 = wave_sum_f32(a00) * inv_s; a01 = wave_sum_f32(a01) * inv_s; a02 = wave_sum_f32(a02) * inv_s;
  a11 = wave_sum_f32(a11) * inv_s; a12 = wave_sum_f32(a12) * inv_s; a22 = wave_sum_f32(a22) * inv_s;
}

// z0: the eigenvector of the smallest eigenvalue of the covariance (wave-uniform).  Out: zp = the sign-resolved normal,
// acc = sum_k alpha_k beta_k v_k (pointnet2_utils.py:455-466), NOT normalised.
template <typename NT>
__device__ __forceinline__ void lrf_vote_xacc(const float *sx, const float *sy, const float *sz, int S, float radius, int lane,
                                              float cx, float cy, float cz, const NT *nbr, Vec3 z0, Vec3 &zp, Vec3 &acc) {
  int vote = 0;
  for (int l0i = 0; l0i < S; l0i += 64) {
    const int l = l0i + lane;
    float pr = 0.f;
    if (l < S) {
      const int k = nbr[l];
      pr = z0.x * (cx - sx[k]) + z0.y * (cy - sy[k]) + z0.z * (cz - sz[k]);
    }
    vote += __builtin_popcountll(__ballot(pr > 1e-3f)) - __builtin_popcountll(__ballot(pr < -1e-3f));
  }
  zp = vote < 0 ? scale(z0, -1.f) : z0;
  float vx = 0, vy = 0, vz = 0;
  for (int l = lane; l < S; l += 64) {
    const int k = nbr[l];
    const Vec3 xn = v3(sx[k] - cx, sy[k] - cy, sz[k] - cz);
    const float nrm = dot(zp, xn);
    const Vec3 vi = sub(xn, scale(zp, nrm));
    float alpha = radius - sqrtf(dot(xn, xn));
    alpha *= alpha;
    const float ab = alpha * (nrm * nrm);
    vx += ab * vi.x; vy += ab * vi.y; vz += ab * vi.z;
  }
  vx = wave_sum_f32(vx); vy = wave_sum_f32(vy); vz = wave_sum_f32(vz);
  acc = v3(vx, vy, vz);
}

}  // namespace unopose
