// Potential symmetries of an object model (unopose_amd/model_sym.py): for C candidate rigid transforms T_c = (R, t) of ONE cloud of N points the
// directed squared deviation  out[c] = max_i min_j d2(T_c p_i, p_j),  the quantity behind the Hausdorff test h(V, S V) < bound with which the
// BOP organisers define a model's potential symmetries.  `model_sym.sym_deviation_host` is the specification.  Everything is float64:
// T_c p is dot3_blas(...) + t per component (csrc/dot3.h, bop_eval._dot3), a squared distance is (dx*dx + dy*dy) + dz*dz as modelinfo.hip
// forms it (-ffp-contract=off), and min and max do not depend on the order they are taken in, so the value carries the host's bits.
//
//   * sym_deviation_kernel: grid (slice, candidate).  A workgroup takes the query tiles slice, slice + slices, ... of its candidate: SYM_OWN
//     transformed query points per thread in registers with their running minima, the cloud walked through LDS tiles of SYM_TILE points read
//     as broadcasts (pts_pair_kernel's scheme with min for max).  The tile's largest minimum goes into out[c] with one 64-bit vector atomic
//     max on the bit pattern: squared distances are non-negative, so their patterns order like unsigned integers.
//   * early exit: a query point whose minimum exceeds bound2 rejects the candidate: the workgroup writes +inf, whose pattern is above every
//     finite one, so the same atomic max carries it and out[c] itself is the "rejected" word.  It is read before every query tile; a
//     workgroup that finds it set stops.  A rejected candidate ends as +inf whichever workgroup notices first and whatever the others still
//     add, an accepted one as the exact maximum over all tiles: the result does not depend on the tiling.  The entry point gives every
//     candidate one slice when there are many candidates (a rejected one then costs one query tile against the cloud, not N^2) and spreads a
//     few candidates over the device.
// A query index past the end repeats the last point (a pair that exists), a cloud tile is read up to its count: no access leaves the
// buffers whatever the values are.
#include <algorithm>

#include "common.h"
#include "dot3.h"

namespace unopose {

constexpr int SYM_THREADS = 256;
constexpr int SYM_OWN = 2;
constexpr int SYM_TILE = SYM_THREADS * SYM_OWN;  // query points of a workgroup's pass = points of an LDS tile
constexpr int SYM_MAX_POINTS = 1 << 22;
constexpr int SYM_MAX_CANDIDATES = 1 << 20;
constexpr int SYM_LAUNCH_CANDIDATES = 65535;     // grid y
constexpr int SYM_FILL_WORKGROUPS = 4096;        // workgroups wanted per launch before candidates share query tiles
constexpr unsigned long long SYM_INF_BITS = 0x7ff0000000000000ull;

__global__ __launch_bounds__(SYM_THREADS) void sym_deviation_kernel(const double *__restrict__ pts, int n, const double *__restrict__ T, double bound2,
                                                                   unsigned long long *out) {
  __shared__ double tx[SYM_TILE], ty[SYM_TILE], tz[SYM_TILE];
  __shared__ double red[SYM_THREADS / 64];
  __shared__ int stop;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double *M = T + 12 * (size_t)blockIdx.y;
  unsigned long long *o = out + blockIdx.y;
  double R[9], t[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = M[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = M[9 + k];
  const int tiles = (n + SYM_TILE - 1) / SYM_TILE;
  for (int row = blockIdx.x; row < tiles; row += gridDim.x) {
    __syncthreads();  // the previous pass has read `red` and `stop`
    if (threadIdx.x == 0) stop = __hip_atomic_load(o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == SYM_INF_BITS;
    __syncthreads();
    if (stop) break;  // block-uniform
    double qx[SYM_OWN], qy[SYM_OWN], qz[SYM_OWN], best[SYM_OWN];
#pragma unroll
    for (int j = 0; j < SYM_OWN; ++j) {
      const int i = min(row * SYM_TILE + j * SYM_THREADS + (int)threadIdx.x, n - 1);  // an own point past the end repeats the last one
      const double x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
      qx[j] = dot3_blas(R[0], x, R[1], y, R[2], z) + t[0];
      qy[j] = dot3_blas(R[3], x, R[4], y, R[5], z) + t[1];
      qz[j] = dot3_blas(R[6], x, R[7], y, R[8], z) + t[2];
      best[j] = __builtin_inf();
    }
    for (int t0 = 0; t0 < n; t0 += SYM_TILE) {
      const int count = min(SYM_TILE, n - t0);
      if (t0) __syncthreads();  // the previous tile has been read
      for (int i = threadIdx.x; i < count; i += SYM_THREADS) {
        tx[i] = pts[3 * (size_t)(t0 + i)], ty[i] = pts[3 * (size_t)(t0 + i) + 1], tz[i] = pts[3 * (size_t)(t0 + i) + 2];
      }
      __syncthreads();
      for (int i = 0; i < count; ++i) {
        const double x = tx[i], y = ty[i], z = tz[i];
#pragma unroll
        for (int j = 0; j < SYM_OWN; ++j) {
          const double dx = qx[j] - x, dy = qy[j] - y, dz = qz[j] - z;
          best[j] = fmin(best[j], (dx * dx + dy * dy) + dz * dz);
        }
      }
    }
    double m = best[0];
#pragma unroll
    for (int j = 1; j < SYM_OWN; ++j) m = fmax(m, best[j]);
    m = wave_all_fmax(m);
    if (lane == 0) red[wave] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
      for (int w = 1; w < SYM_THREADS / 64; ++w) m = fmax(m, red[w]);
      // the largest minimum exceeds the bound exactly when some point's minimum does
      atomicMax(o, m > bound2 ? SYM_INF_BITS : (unsigned long long)__double_as_longlong(m));
    }
  }
}

}  // namespace unopose

using namespace unopose;

extern "C" {

int unopose_sym_deviation_tile(void) { return SYM_TILE; }
int unopose_sym_deviation_launch_candidates(void) { return SYM_LAUNCH_CANDIDATES; }

int unopose_sym_deviation(const double *pts, int N, const double *T, int C, double bound2, double *out, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(pts && T && out, "sym_deviation: null pointer");
  UNOPOSE_REQUIRE(N >= 1 && N <= SYM_MAX_POINTS, "sym_deviation: %d points (1 .. 2^22)", N);
  UNOPOSE_REQUIRE(C >= 1 && C <= SYM_MAX_CANDIDATES, "sym_deviation: %d candidates (1 .. 2^20)", C);
  UNOPOSE_REQUIRE(bound2 >= 0.0, "sym_deviation: squared bound %g (>= 0, +inf allowed)", bound2);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(out, 0, sizeof(double) * (size_t)C, s) != hipSuccess) {  // +0.0: the value the atomic maxima start from
    (void)hipGetLastError();
    set_error("sym_deviation: cannot clear the output");
    return UNOPOSE_ELAUNCH;
  }
  const int tiles = cdiv(N, SYM_TILE);
  for (int c0 = 0; c0 < C; c0 += SYM_LAUNCH_CANDIDATES) {
    const int cs = std::min(SYM_LAUNCH_CANDIDATES, C - c0);
    const int slices = std::min(tiles, std::max(1, SYM_FILL_WORKGROUPS / cs));
    hipLaunchKernelGGL(sym_deviation_kernel, dim3(slices, cs), dim3(SYM_THREADS), 0, s, pts, N, T + 12 * (size_t)c0, bound2,
                       (unsigned long long *)out + c0);
    if (int rc = check_launch("sym_deviation")) return rc;
  }
  return UNOPOSE_OK;
}

}  // extern "C"
