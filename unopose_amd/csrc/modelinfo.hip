// models_info.json on the device (unopose_amd/model_info.py; the toolkit's scripts/calc_model_info.py with misc.calc_pts_diameter): per object
// the axis-aligned box and the largest squared distance between two of its points, for M objects packed in one array per launch sequence.
// `model_info.extent_host` is the specification.  Everything is float64 and a squared distance is (dx*dx + dy*dy) + dz*dz as written: the
// library is built with -ffp-contract=off, a maximum does not depend on the order it is taken in, so the value carries the host's bits.
//
//   * pts_scan_kernel: one workgroup of EXT_SCAN_THREADS threads per object.  Pass 1: the three minima, the three maxima and the mean c.
//     With pruning four more passes: the point a farthest from c (r_max = |a - c|), the point b farthest from a, the point farthest from b
//     (L = that distance: a lower bound of the diameter that an actual pair attains), and the ordered compaction of the points that can
//     still belong to a pair at distance >= L: by the triangle inequality |p - q| <= r_p + r_q <= r_p + r_max, so a point with
//     (r_p + r_max) (1 + 2^-40) < L cannot; b and its partner survive (their distance IS L), so the maximum over the survivors is the
//     global one, formed from the same pair by the same expression.  The margin 2^-40 is far above the few ulp of the square roots and
//     sums compared.  Which points survive is not part of the result: only the maximum is.  Ties keep the smallest index.
//   * pts_pair_kernel: the all-pairs maximum over the (surviving) points, cut into tiles of EXT_TILE points.  Grid (row a, slice,
//     object): a workgroup keeps the row's tile as EXT_OWN "own" points per thread with their running maxima in registers and walks the
//     tiles b = a + slice, a + slice + EXT_SPLIT, ... of the SAME object through LDS, read as broadcasts (adi_partial_kernel's scheme with
//     max for min; b >= a because a squared distance is symmetric to the bit), then does the same for row tiles - 1 - a, so that every
//     workgroup of a slice has the same amount of work.  Wave then workgroup maximum, then one 64-bit vector atomic
//     max on the bit pattern: squared distances are non-negative and finite, so their patterns order like unsigned integers and the
//     result does not depend on the order the workgroups arrive in.  No V^2 storage, no pair across two objects.
// The kernels never read outside [0, n_total) points whatever the device copy of the offsets holds; the entry point validates the host copy.
#include <algorithm>

#include "common.h"

namespace unopose {

constexpr int EXT_THREADS = 256;
constexpr int EXT_OWN = 2;
constexpr int EXT_TILE = EXT_THREADS * EXT_OWN;  // own points of a workgroup = points of an LDS tile
constexpr int EXT_SPLIT = 8;                     // workgroups that share the walk over the tiles b >= a
constexpr int EXT_SCAN_THREADS = 1024;
constexpr int EXT_SCAN_WAVES = EXT_SCAN_THREADS / 64;
constexpr int EXT_OUT = 7;                       // min x, y, z, max x, y, z, largest squared distance
constexpr int EXT_MAX_POINTS = 1 << 24;
constexpr int EXT_MAX_OBJECTS = 65535;           // grid z

__device__ __forceinline__ double dist2(double ax, double ay, double az, double bx, double by, double bz) {
  const double dx = ax - bx, dy = ay - by, dz = az - bz;
  return (dx * dx + dy * dy) + dz * dz;
}

// The object's points of the launch: [lo, lo + cnt) of the packed array, or nothing if the table does not fit n_total.
__device__ __forceinline__ bool object_range(const long long *__restrict__ offs, const long long *__restrict__ counts, int k, long long n_total,
                                             long long &lo, int &cnt) {
  lo = offs[k];
  const long long c = counts ? counts[k] : offs[k + 1] - lo;
  if (lo < 0 || c < 1 || c > EXT_MAX_POINTS || lo > n_total - c) return false;
  cnt = (int)c;
  return true;
}

// The point of [0, n) farthest from q: (squared distance, smallest index that attains it), the same in every thread.
__device__ double farthest_from(const double *__restrict__ p, int n, double qx, double qy, double qz, int &arg, double (*red)[EXT_SCAN_WAVES],
                                int (*red_i)[EXT_SCAN_WAVES], int slot) {
  double best = -1.0;
  int at = 0;
  for (int i = threadIdx.x; i < n; i += EXT_SCAN_THREADS) {
    const double d = dist2(p[3 * (size_t)i], p[3 * (size_t)i + 1], p[3 * (size_t)i + 2], qx, qy, qz);
    if (d > best) best = d, at = i;  // increasing i: the first of a thread's ties stays
  }
  const double wmax = wave_all_fmax(best);
  const int cand = wave_all_min(best == wmax ? at : 0x7fffffff);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) red[slot][wave] = wmax, red_i[slot][wave] = cand;
  __syncthreads();
  double m = red[slot][0];
  int mi = red_i[slot][0];
#pragma unroll
  for (int w = 1; w < EXT_SCAN_WAVES; ++w) {
    const double v = red[slot][w];
    const int vi = red_i[slot][w];
    if (v > m || (v == m && vi < mi)) m = v, mi = vi;
  }
  arg = mi;
  return m;
}

__global__ __launch_bounds__(EXT_SCAN_THREADS) void pts_scan_kernel(const double *__restrict__ pts, const long long *__restrict__ offs, long long n_total,
                                                                   int prune, double *__restrict__ kept, long long *__restrict__ kept_count,
                                                                   double *__restrict__ out) {
  __shared__ double red[7][EXT_SCAN_WAVES];
  __shared__ int red_i[3][EXT_SCAN_WAVES];
  __shared__ int wave_kept[EXT_SCAN_WAVES];
  const int k = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double *o = out + (size_t)k * EXT_OUT;
  long long lo;
  int n;
  if (!object_range(offs, nullptr, k, n_total, lo, n)) {
    if (threadIdx.x < EXT_OUT) o[threadIdx.x] = __builtin_nan("");
    if (prune && threadIdx.x == 0) kept_count[k] = 0;
    return;
  }
  const double *p = pts + 3 * (size_t)lo;
  const double inf = __builtin_inf();
  double mn[3] = {inf, inf, inf}, mx[3] = {-inf, -inf, -inf}, sum[3] = {0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < n; i += EXT_SCAN_THREADS) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double v = p[3 * (size_t)i + c];
      mn[c] = fmin(mn[c], v), mx[c] = fmax(mx[c], v), sum[c] += v;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    mn[c] = wave_all_fmin(mn[c]), mx[c] = wave_all_fmax(mx[c]);
    if (lane == 0) red[c][wave] = mn[c], red[3 + c][wave] = mx[c];
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    double v = red[threadIdx.x][0];
    for (int w = 1; w < EXT_SCAN_WAVES; ++w) v = threadIdx.x < 3 ? fmin(v, red[threadIdx.x][w]) : fmax(v, red[threadIdx.x][w]);
    o[threadIdx.x] = v;
  }
  if (threadIdx.x == 0) o[6] = 0.0;  // the pair (i, i): the value the atomic maxima start from
  if (!prune) return;

  // the centre: any point serves the bound, the mean keeps r_max small.  Sums in a fixed order.
  __syncthreads();
  double c3[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    sum[c] = wave_all_sum(sum[c]);
    if (lane == 0) red[c][wave] = sum[c];
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double s = red[c][0];
    for (int w = 1; w < EXT_SCAN_WAVES; ++w) s += red[c][w];
    c3[c] = s / (double)n;
  }
  int a, b, e;
  const double r_max = sqrt(farthest_from(p, n, c3[0], c3[1], c3[2], a, red + 3, red_i, 0));
  farthest_from(p, n, p[3 * (size_t)a], p[3 * (size_t)a + 1], p[3 * (size_t)a + 2], b, red + 3, red_i, 1);
  const double L = sqrt(farthest_from(p, n, p[3 * (size_t)b], p[3 * (size_t)b + 1], p[3 * (size_t)b + 2], e, red + 3, red_i, 2));
  // ordered compaction into the object's own stretch of `kept`
  double *q = kept + 3 * (size_t)lo;
  const double margin = 1.0 + 0x1p-40;
  int base = 0;
  for (int i0 = 0; i0 < n; i0 += EXT_SCAN_THREADS) {
    const int i = i0 + (int)threadIdx.x;
    double x = 0.0, y = 0.0, z = 0.0;
    bool keep = false;
    if (i < n) {
      x = p[3 * (size_t)i], y = p[3 * (size_t)i + 1], z = p[3 * (size_t)i + 2];
      keep = !((sqrt(dist2(x, y, z, c3[0], c3[1], c3[2])) + r_max) * margin < L);
    }
    const unsigned long long mask = __ballot(keep);
    __syncthreads();  // the previous round's counts have been read
    if (lane == 0) wave_kept[wave] = __popcll(mask);
    __syncthreads();
    int before = base, total = base;
#pragma unroll
    for (int w = 0; w < EXT_SCAN_WAVES; ++w) {
      if (w < wave) before += wave_kept[w];
      total += wave_kept[w];
    }
    if (keep) {
      const int at = before + __popcll(mask & ((1ull << lane) - 1ull));  // at <= i < n: inside the object's stretch
      q[3 * (size_t)at] = x, q[3 * (size_t)at + 1] = y, q[3 * (size_t)at + 2] = z;
    }
    base = total;
  }
  if (threadIdx.x == 0) kept_count[k] = base;
}

__global__ __launch_bounds__(EXT_THREADS) void pts_pair_kernel(const double *__restrict__ pts, const long long *__restrict__ offs,
                                                              const long long *__restrict__ counts, long long n_total, double *__restrict__ out) {
  __shared__ double tx[EXT_TILE], ty[EXT_TILE], tz[EXT_TILE];
  __shared__ double red[EXT_THREADS / 64];
  const int k = blockIdx.z, a = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long lo;
  int n;
  if (!object_range(offs, counts, k, n_total, lo, n)) return;  // block-uniform
  const int tiles = (n + EXT_TILE - 1) / EXT_TILE;
  if (a >= (tiles + 1) / 2) return;
  const double *p = pts + 3 * (size_t)lo;
  double m = 0.0;
  // two rows per workgroup, a and tiles - 1 - a: the long walk of one and the short walk of the other add up to the same work for every a
  for (int pass = 0; pass < 2; ++pass) {
    const int row = pass ? tiles - 1 - a : a;
    if (pass && row == a) break;
    double qx[EXT_OWN], qy[EXT_OWN], qz[EXT_OWN], best[EXT_OWN];
#pragma unroll
    for (int j = 0; j < EXT_OWN; ++j) {
      const int i = min(row * EXT_TILE + j * EXT_THREADS + (int)threadIdx.x, n - 1);  // an own point past the end repeats the last one: a pair that exists
      qx[j] = p[3 * (size_t)i], qy[j] = p[3 * (size_t)i + 1], qz[j] = p[3 * (size_t)i + 2], best[j] = 0.0;
    }
    for (int b = row + (int)blockIdx.y; b < tiles; b += EXT_SPLIT) {
      const int t0 = b * EXT_TILE, count = min(EXT_TILE, n - t0);
      __syncthreads();  // the previous tile has been read
      for (int i = threadIdx.x; i < count; i += EXT_THREADS) {
        tx[i] = p[3 * (size_t)(t0 + i)], ty[i] = p[3 * (size_t)(t0 + i) + 1], tz[i] = p[3 * (size_t)(t0 + i) + 2];
      }
      __syncthreads();
      for (int i = 0; i < count; ++i) {
        const double x = tx[i], y = ty[i], z = tz[i];
#pragma unroll
        for (int j = 0; j < EXT_OWN; ++j) best[j] = fmax(best[j], dist2(qx[j], qy[j], qz[j], x, y, z));
      }
    }
#pragma unroll
    for (int j = 0; j < EXT_OWN; ++j) m = fmax(m, best[j]);
  }
  m = wave_all_fmax(m);
  if (lane == 0) red[wave] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < EXT_THREADS / 64; ++w) m = fmax(m, red[w]);
    m = fmax(m, red[0]);
    atomicMax((unsigned long long *)(out + (size_t)k * EXT_OUT + 6), (unsigned long long)__double_as_longlong(m));
  }
}

}  // namespace unopose

using namespace unopose;

extern "C" {

int unopose_pts_extent_tile_points(void) { return EXT_TILE; }
int unopose_pts_extent_doubles(void) { return EXT_OUT; }

int unopose_pts_extent(const double *pts, const long long *offsets, const long long *offsets_dev, int M, int prune, double *kept,
                       long long *kept_count, double *out, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(pts && offsets && offsets_dev && out, "pts_extent: null pointer");
  UNOPOSE_REQUIRE(!prune || (kept && kept_count), "pts_extent: pruning needs the kept and kept_count buffers");
  UNOPOSE_REQUIRE(M >= 1 && M <= EXT_MAX_OBJECTS, "pts_extent: %d objects per call (1 .. %d)", M, EXT_MAX_OBJECTS);
  UNOPOSE_REQUIRE(offsets[0] == 0, "pts_extent: offsets start at %lld, not 0", offsets[0]);
  long long largest = 0;
  for (int k = 0; k < M; ++k) {
    const long long v = offsets[k + 1] - offsets[k];
    UNOPOSE_REQUIRE(v >= 0, "pts_extent: offsets decrease at object %d (%lld after %lld)", k, offsets[k + 1], offsets[k]);
    UNOPOSE_REQUIRE(v >= 1, "pts_extent: object %d is empty", k);
    UNOPOSE_REQUIRE(v <= EXT_MAX_POINTS, "pts_extent: object %d has %lld points (at most 2^24)", k, v);
    largest = v > largest ? v : largest;
  }
  const long long n_total = offsets[M];
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(pts_scan_kernel, dim3(M), dim3(EXT_SCAN_THREADS), 0, s, pts, offsets_dev, n_total, prune, kept, kept_count, out);
  if (int rc = check_launch("pts_extent: box and pruning")) return rc;
  // the grid is sized by the largest object before pruning: a workgroup whose tile the object (or what is left of it) does not have returns
  const int tiles = cdiv(largest, EXT_TILE);
  hipLaunchKernelGGL(pts_pair_kernel, dim3((tiles + 1) / 2, std::min(tiles, EXT_SPLIT), M), dim3(EXT_THREADS), 0, s, prune ? (const double *)kept : pts, offsets_dev,
                     prune ? (const long long *)kept_count : (const long long *)nullptr, n_total, out);
  return check_launch("pts_extent");
}

}  // extern "C"
