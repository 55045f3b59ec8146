// One-reference target lists on the device (unopose_amd/ref_targets.py): for the Q query views and C candidate views of ONE object, under its S
// symmetries, per query the keyed-random pick among the candidates within the rotation bound, how many there are, and the nearest allowed
// candidate.  `ref_targets.select_host` is the specification.  Everything is float64; both 3 x 3 products are formed by dot3_blas
// (bop_eval._dot3), the trace is (d0 + d1) + d2 clamped to 3, and every decision is a comparison of such traces, so the value carries the
// host's bits whatever the launch shape.
//
//   * ref_partial_kernel: grid (candidate slabs, query tiles), one wave per workgroup.  A lane owns REF_OWN queries: their rotations, scene and
//     key, the first half of the priority hash and the running results stay in registers.  The workgroup walks the (candidate, symmetry)
//     entries of its slab in candidate-major order in tiles of REF_TILE: each lane composes one T = R_c S (27 operations, once per entry and
//     query tile) into LDS, then every lane reads the tile as broadcasts (adi_partial_kernel's scheme): 9 multiply / fma operations and a max
//     per (query, candidate, symmetry).  At a candidate's last symmetry the lane decides: allowed (other scene, or other key), nearest so
//     far (strictly larger trace: the lower index stays), eligible (best >= trace_min), and, if so, the priority
//     mix64(mix64(seed + G + q_key) + G + c_key) against the smallest so far (strictly smaller: the lower index stays).
//     One partial per (query, slab) goes to the workspace.
//   * ref_finish_kernel: one wave per query.  Lanes stride over the slabs and combine the partials; every combination carries the candidate
//     index and breaks ties by it, and the eligible counts are integers, so the result does not depend on how the candidates were cut.
// No atomics.  The kernels trust their sizes: the entry point checks them, ops/score.py checks the values (finite, bounded).
#include <algorithm>

#include "common.h"
#include "dot3.h"

namespace unopose {

constexpr int REF_THREADS = 64;
constexpr int REF_OWN = 2;
constexpr int REF_QTILE = REF_THREADS * REF_OWN;  // queries of a workgroup
constexpr int REF_TILE = 64;                      // (candidate, symmetry) entries of an LDS tile: one per lane
constexpr int REF_BLOCKS = 2048;                  // workgroups the automatic slab size aims at: two waves for each of the 1024 SIMDs
constexpr int REF_FIELDS = 5;                     // nearest trace, nearest, priority, pick, eligible count
constexpr int REF_MAX_Q = 1 << 22, REF_MAX_C = 1 << 24, REF_MAX_S = 1 << 16, REF_MAX_ENTRIES = 1 << 30, REF_MAX_SLABS = 65535;
constexpr unsigned long long REF_GOLDEN = 0x9E3779B97F4A7C15ull;

__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// a replaces b as the nearest: larger trace, the lower index among equals.  "None" is (-inf, -1) and loses to every candidate.
__device__ __forceinline__ bool nearer(double ta, int ia, double tb, int ib) { return ta > tb || (ta == tb && ia >= 0 && ia < ib); }
// a replaces b as the pick: a exists, and b does not or has the larger priority, the lower index among equals.
__device__ __forceinline__ bool preferred(unsigned long long pa, int ia, unsigned long long pb, int ib) {
  return ia >= 0 && (ib < 0 || pa < pb || (pa == pb && ia < ib));
}

__global__ __launch_bounds__(REF_THREADS) void ref_partial_kernel(const double *__restrict__ Rq, const long long *__restrict__ q_scene,
                                                                 const unsigned long long *__restrict__ q_key, int Q, const double *__restrict__ Rc,
                                                                 const long long *__restrict__ c_scene, const unsigned long long *__restrict__ c_key,
                                                                 int C, const double *__restrict__ syms, int S, double trace_min,
                                                                 unsigned long long seed, int cross_scene, int slab, int slabs,
                                                                 long long *__restrict__ ws) {
  __shared__ double T[REF_TILE][9];
  const int c0 = blockIdx.x * slab, c1 = min(C, c0 + slab);
  const int entries = (c1 - c0) * S;  // <= REF_MAX_ENTRIES, checked at the entry point
  const double ninf = -__builtin_inf();
  double R[REF_OWN][9], best[REF_OWN], near_t[REF_OWN];
  long long scene[REF_OWN];
  unsigned long long key[REF_OWN], half[REF_OWN], prio[REF_OWN];
  int near_i[REF_OWN], pick[REF_OWN], count[REF_OWN];
#pragma unroll
  for (int j = 0; j < REF_OWN; ++j) {
    const int q = min((int)blockIdx.y * REF_QTILE + j * REF_THREADS + (int)threadIdx.x, Q - 1);  // a query past the end repeats the last one and is not written
#pragma unroll
    for (int k = 0; k < 9; ++k) R[j][k] = Rq[(size_t)q * 9 + k];
    scene[j] = q_scene[q], key[j] = q_key[q], half[j] = mix64(seed + REF_GOLDEN + key[j]);
    best[j] = ninf, near_t[j] = ninf, near_i[j] = -1, prio[j] = 0ull, pick[j] = -1, count[j] = 0;
  }
  int c = c0, s = 0;  // the entry the walk stands at: wave-uniform
  for (int e0 = 0; e0 < entries; e0 += REF_TILE) {
    const int n = min(REF_TILE, entries - e0);
    __syncthreads();  // the previous tile has been read
    if ((int)threadIdx.x < n) {
      const int e = e0 + (int)threadIdx.x, cl = e / S;
      const double *A = Rc + (size_t)(c0 + cl) * 9, *B = syms + (size_t)(e - cl * S) * 9;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int k = 0; k < 3; ++k) T[threadIdx.x][3 * r + k] = dot3_blas(A[3 * r], B[k], A[3 * r + 1], B[3 + k], A[3 * r + 2], B[6 + k]);  // R_c . S as re_sym forms R_gt S
      }
    }
    __syncthreads();
    for (int i = 0; i < n; ++i) {
      double t[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) t[k] = T[i][k];
#pragma unroll
      for (int j = 0; j < REF_OWN; ++j) {
        const double d0 = dot3_blas(R[j][0], t[0], R[j][1], t[1], R[j][2], t[2]), d1 = dot3_blas(R[j][3], t[3], R[j][4], t[4], R[j][5], t[5]);
        const double d2 = dot3_blas(R[j][6], t[6], R[j][7], t[7], R[j][8], t[8]);
        double trace = (d0 + d1) + d2;
        trace = trace <= 3.0 ? trace : 3.0;
        best[j] = fmax(best[j], trace);
      }
      if (++s < S) continue;
      // the candidate's last symmetry: decide, then start the next candidate
      const long long cs = c_scene[c];
      const unsigned long long ck = c_key[c];
#pragma unroll
      for (int j = 0; j < REF_OWN; ++j) {
        const bool allowed = cross_scene ? cs != scene[j] : ck != key[j];
        if (allowed) {
          if (best[j] > near_t[j]) near_t[j] = best[j], near_i[j] = c;
          if (best[j] >= trace_min) {
            const unsigned long long p = mix64(half[j] + REF_GOLDEN + ck);
            if (pick[j] < 0 || p < prio[j]) prio[j] = p, pick[j] = c;
            ++count[j];
          }
        }
        best[j] = ninf;
      }
      s = 0, ++c;
    }
  }
#pragma unroll
  for (int j = 0; j < REF_OWN; ++j) {
    const int q = (int)blockIdx.y * REF_QTILE + j * REF_THREADS + (int)threadIdx.x;
    if (q >= Q) continue;
    const size_t plane = (size_t)Q * slabs, at = (size_t)q * slabs + blockIdx.x;
    ws[at] = __double_as_longlong(near_t[j]);
    ws[plane + at] = near_i[j];
    ws[2 * plane + at] = (long long)prio[j];
    ws[3 * plane + at] = pick[j];
    ws[4 * plane + at] = count[j];
  }
}

__global__ __launch_bounds__(64) void ref_finish_kernel(const long long *__restrict__ ws, int Q, int slabs, long long *__restrict__ out) {
  const int q = blockIdx.x, lane = threadIdx.x;
  const size_t plane = (size_t)Q * slabs, row = (size_t)q * slabs;
  double near_t = -__builtin_inf();
  int near_i = -1, pick = -1;
  unsigned long long prio = 0ull;
  long long count = 0;
  for (int k = lane; k < slabs; k += 64) {
    const double t = __longlong_as_double(ws[row + k]);
    const int ti = (int)ws[plane + row + k], pi = (int)ws[3 * plane + row + k];
    const unsigned long long p = (unsigned long long)ws[2 * plane + row + k];
    if (nearer(t, ti, near_t, near_i)) near_t = t, near_i = ti;
    if (preferred(p, pi, prio, pick)) prio = p, pick = pi;
    count += ws[4 * plane + row + k];
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const double t = __shfl_xor(near_t, o, 64);
    const int ti = __shfl_xor(near_i, o, 64), pi = __shfl_xor(pick, o, 64);
    const unsigned long long p = (unsigned long long)__shfl_xor((long long)prio, o, 64);
    if (nearer(t, ti, near_t, near_i)) near_t = t, near_i = ti;
    if (preferred(p, pi, prio, pick)) prio = p, pick = pi;
  }
  count = wave_all_sum(count);
  if (lane == 0) {
    out[q] = pick;
    out[(size_t)Q + q] = count;
    out[(size_t)2 * Q + q] = near_i;
    out[(size_t)3 * Q + q] = __double_as_longlong(near_t + 0.0);  // a trace of -0.0 leaves as +0.0, as on the host
  }
}

static int automatic_slab(int Q, int C, int S) {
  const long tiles = cdiv(Q, REF_QTILE);
  const long want = std::max(1l, REF_BLOCKS / tiles);
  long slab = std::max((long)cdiv(C, want), (long)cdiv(REF_TILE, S));  // no workgroup with less than one tile of entries
  slab = std::max(slab, (long)cdiv(C, REF_MAX_SLABS));
  slab = std::min(slab, (long)std::max(1, REF_MAX_ENTRIES / S));
  return (int)std::min(slab, (long)C);
}

}  // namespace unopose

using namespace unopose;

extern "C" {

int unopose_ref_select_query_tile(void) { return REF_QTILE; }
int unopose_ref_select_entry_tile(void) { return REF_TILE; }

int unopose_ref_select_slab(int Q, int C, int S) {
  if (!(Q >= 1 && Q <= REF_MAX_Q && C >= 1 && C <= REF_MAX_C && S >= 1 && S <= REF_MAX_S)) {
    set_error("ref_select: bad sizes (Q=%d C=%d S=%d)", Q, C, S);
    return 0;  // a slab size is at least 1
  }
  return automatic_slab(Q, C, S);
}

int unopose_ref_select(const double *Rq, const long long *q_scene, const unsigned long long *q_key, int Q, const double *Rc,
                       const long long *c_scene, const unsigned long long *c_key, int C, const double *syms, int S, double trace_min,
                       unsigned long long seed, int cross_scene, int slab, long long *workspace, long long *out, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(Rq && q_scene && q_key && Rc && c_scene && c_key && syms && workspace && out, "ref_select: null pointer");
  UNOPOSE_REQUIRE(Q >= 1 && Q <= REF_MAX_Q && C >= 1 && C <= REF_MAX_C && S >= 1 && S <= REF_MAX_S, "ref_select: bad sizes (Q=%d C=%d S=%d)", Q, C, S);
  UNOPOSE_REQUIRE(trace_min == trace_min, "ref_select: trace_min is NaN");
  UNOPOSE_REQUIRE(slab >= 1 && slab <= C, "ref_select: %d candidates per slab (1 .. C = %d)", slab, C);
  UNOPOSE_REQUIRE((long long)slab * S <= REF_MAX_ENTRIES, "ref_select: a slab of %d candidates x %d symmetries (at most 2^30 entries)", slab, S);
  const int slabs = cdiv(C, slab);
  UNOPOSE_REQUIRE(slabs <= REF_MAX_SLABS, "ref_select: %d slabs of %d candidates (at most %d)", slabs, slab, REF_MAX_SLABS);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ref_partial_kernel, dim3(slabs, cdiv(Q, REF_QTILE)), dim3(REF_THREADS), 0, s, Rq, q_scene, q_key, Q, Rc, c_scene, c_key, C, syms,
                     S, trace_min, seed, cross_scene, slab, slabs, workspace);
  if (int rc = check_launch("ref_select: partials")) return rc;
  hipLaunchKernelGGL(ref_finish_kernel, dim3(Q), dim3(64), 0, s, workspace, Q, slabs, out);
  return check_launch("ref_select");
}

}  // extern "C"
