// Scoring mask proposals against reference views (unopose_amd/match_dets.py states the rule in numpy; ops/detect.py wraps these):
//   * patch validity of a resized window mask (integers; equal to the numpy rule in every byte),
//   * unit token rows in bf16 (fp32 norm, one rounding),
//   * the appearance score of every (proposal, object) pair: the T x T cosine products of their patch tokens on
//     v_mfma_f32_16x16x32_bf16, the maximum over the object's valid patches per proposal patch and the mean of those maxima over the
//     proposal's valid patches -- only valid patches are multiplied, and the products live in accumulators only, 32 rows x 128 columns
//     per wave at a time,
//   * the class-token cosine of every pair,
//   * suppression of overlapping proposals of one category: masks packed to bits, areas and pair intersections by popcount, one
//     wavefront that walks the score order.
// No atomics anywhere: every result depends on the inputs alone, so two calls return the same bits.
#include "attn_common.h"  // row16_max; the bf16x8 / f32x4 fragment types and the butterfly are common.h's

namespace unopose {
namespace {

constexpr int DM_PATCH = 14;      // pixels per patch side (the ViT's)
constexpr int DM_MAX_T = 4096;    // patch tokens per view the score kernel keeps row maxima for (16 KiB of LDS)
constexpr int DM_RT = 2;          // 16-row tiles of a wave's row block (32 proposal patches)
constexpr int DM_CT = 8;          // 16-column tiles per pass (128 object patches)
constexpr int DM_MAX_MASKS = 4096;  // proposals of one suppression call (order and kept list in LDS)

// out[k][r * side + c] = 1 iff at least half of the 14 x 14 pixels of patch (r, c) of the resized window are set; pixel (Y, X) of the
// resized crop reads window pixel (Y s / img_size, X s / img_size) of the s x s window k (desc: byte offset, s).
__global__ __launch_bounds__(256) void dm_patch_valid_kernel(const uint8_t *__restrict__ packed, const int *__restrict__ desc, int K,
                                                             int img_size, int side, uint8_t *__restrict__ out) {
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  const int per = side * side;
  if (g >= (long)K * per) return;
  const int k = (int)(g / per), pc = (int)(g - (long)k * per);
  const int r = pc / side, c = pc - r * side;
  const int off = desc[2 * k], s = desc[2 * k + 1];
  int cnt = 0;
  for (int dy = 0; dy < DM_PATCH; ++dy) {
    const int sy = (r * DM_PATCH + dy) * s / img_size;
    const uint8_t *row = packed + off + (long)sy * s;
    for (int dx = 0; dx < DM_PATCH; ++dx) cnt += row[(c * DM_PATCH + dx) * s / img_size] != 0;
  }
  out[g] = (uint8_t)(2 * cnt >= DM_PATCH * DM_PATCH);
}

__device__ __forceinline__ float dm_load(const float *p) { return *p; }
__device__ __forceinline__ float dm_load(const u16 *p) { return bf2f(*p); }

// One wave per row: fp32 sum of squares (each lane its elements in order, then the butterfly), x / norm rounded once to bf16.
template <typename T>
__global__ __launch_bounds__(256) void dm_unit_rows_kernel(const T *__restrict__ x, long rows, int D, u16 *__restrict__ out) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const T *xr = x + row * D;
  float ss = 0.f;
  for (int d = lane; d < D; d += 64) {
    const float v = dm_load(xr + d);
    ss += v * v;
  }
  const float nrm = sqrtf(wave_all_sum(ss));
  u16 *o = out + row * D;
  for (int d = lane; d < D; d += 64) o[d] = nrm > 0.f ? f2bf(dm_load(xr + d) / nrm) : (u16)0;
}

// The numbers of the set bytes of v[0 .. T) in ascending order -> idx (LDS, u16: T <= 4096); returns their count.  One wave.
__device__ __forceinline__ int dm_compact(const uint8_t *__restrict__ v, int T, int lane, u16 *idx) {
  int n = 0;
  for (int base = 0; base < T; base += 64) {
    const bool set = base + lane < T && v[base + lane] != 0;
    const unsigned long long mask = __ballot(set);
    if (set) idx[n + __popcll(mask & ((1ull << lane) - 1ull))] = (u16)(base + lane);
    n += __popcll(mask);
  }
  return n;
}

// out[p][o] = mean over the valid rows i of q[p] of max over the valid rows j of r[o] of q[p][i] . r[o][j]; 0 when either side has no
// valid row.  One workgroup per (p, o).  Only valid rows take part, so the workgroup first lists them (waves 0 and 1, one side each) and
// then works on the nq x nr products of the listed rows alone: wave w owns the blocks w, w + 4, ... of 32 listed proposal rows and walks
// the listed object rows 128 at a time.  Fragments straight from global memory, each lane through the pointer of its own row (a lane reads
// 16 consecutive bytes: A[row l & 15][k = 8 (l >> 4) + e], B[k][column l & 15] the same from the other side), so the listing costs no
// copy; four k-steps of loads are in flight ahead of their MFMAs.  Tail tiles read the last listed row and are masked: columns by `cv`,
// rows by never being summed.
__global__ __launch_bounds__(256) void dm_patch_match_kernel(const u16 *__restrict__ q, const uint8_t *__restrict__ qv, const u16 *__restrict__ r,
                                                             const uint8_t *__restrict__ rv, int O, int T, int D, float *__restrict__ out) {
  __shared__ float rowmax[DM_MAX_T];
  __shared__ u16 qidx[DM_MAX_T], ridx[DM_MAX_T];
  __shared__ int count[2];
  const int p = blockIdx.y, o = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const u16 *Q = q + (long)p * T * D, *R = r + (long)o * T * D;

  if (wave < 2) {
    const int n = wave == 0 ? dm_compact(qv + (long)p * T, T, lane, qidx) : dm_compact(rv + (long)o * T, T, lane, ridx);
    if (lane == 0) count[wave] = n;
  }
  __syncthreads();
  const int nq = count[0], nr = count[1];
  if (nq == 0 || nr == 0) {  // uniform over the workgroup
    if (threadIdx.x == 0) out[(long)p * O + o] = 0.f;
    return;
  }

  const float ninf = -__builtin_inff();
  const int n_ct = (nr + 15) >> 4;
  for (int rb = wave; rb * (16 * DM_RT) < nq; rb += 4) {
    const int row0 = rb * (16 * DM_RT);
    const int nu = min(DM_RT, (nq - row0 + 15) >> 4);
    const u16 *ap[DM_RT];
#pragma unroll
    for (int u = 0; u < DM_RT; ++u) ap[u] = Q + (long)qidx[min(row0 + u * 16 + li, nq - 1)] * D + 8 * lg;
    float m[DM_RT][4];
#pragma unroll
    for (int u = 0; u < DM_RT; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) m[u][e] = ninf;

    for (int c0 = 0; c0 < n_ct; c0 += DM_CT) {
      bool cv[DM_CT];
      const u16 *bp[DM_CT];
#pragma unroll
      for (int j = 0; j < DM_CT; ++j) {
        const int col = (c0 + j) * 16 + li;
        cv[j] = col < nr;
        bp[j] = R + (long)ridx[min(col, nr - 1)] * D + 8 * lg;
      }
      const int nj = min(DM_CT, n_ct - c0);
      f32x4 acc[DM_RT][DM_CT];
#pragma unroll
      for (int u = 0; u < DM_RT; ++u)
#pragma unroll
        for (int j = 0; j < DM_CT; ++j) acc[u][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
      for (int k = 0; k < D; k += 32) {
        bf16x8 a[DM_RT], b[DM_CT];
#pragma unroll
        for (int u = 0; u < DM_RT; ++u) a[u] = *reinterpret_cast<const bf16x8 *>(ap[u] + k);
#pragma unroll
        for (int j = 0; j < DM_CT; ++j) b[j] = *reinterpret_cast<const bf16x8 *>(bp[j] + k);
#pragma unroll
        for (int j = 0; j < DM_CT; ++j) {
          if (j < nj) {  // uniform: whole column tiles past the last listed row are not multiplied
#pragma unroll
            for (int u = 0; u < DM_RT; ++u)
              if (u < nu) acc[u][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[u], b[j], acc[u][j], 0, 0, 0);
          }
        }
      }
      // C: column = l & 15, row = 4 (l >> 4) + e
#pragma unroll
      for (int j = 0; j < DM_CT; ++j)
        if (cv[j]) {
#pragma unroll
          for (int u = 0; u < DM_RT; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) m[u][e] = fmaxf(m[u][e], acc[u][j][e]);
        }
    }
#pragma unroll
    for (int u = 0; u < DM_RT; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float v = row16_max(m[u][e]);
        const int row = row0 + u * 16 + 4 * lg + e;
        if (li == 0 && row < nq) rowmax[row] = v;
      }
  }
  __syncthreads();
  if (wave == 0) {  // the one summation order: lane l adds the listed rows l, l + 64, ... in turn, then the butterfly
    float s = 0.f;
    for (int t = lane; t < nq; t += 64) s += rowmax[t];
    s = wave_all_sum(s);
    if (lane == 0) out[(long)p * O + o] = s / (float)nq;
  }
}

// out[p][o] = qc[p] . rc[o], one wave per pair, fp32, one order.
__global__ __launch_bounds__(256) void dm_class_cosine_kernel(const u16 *__restrict__ qc, const u16 *__restrict__ rc, long pairs, int O, int D,
                                                              float *__restrict__ out) {
  const long pair = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (pair >= pairs) return;
  const u16 *a = qc + (pair / O) * D, *b = rc + (pair % O) * D;
  float s = 0.f;
  for (int d = lane; d < D; d += 64) s += bf2f(a[d]) * bf2f(b[d]);
  s = wave_all_sum(s);
  if (lane == 0) out[pair] = s;
}

// bits[n][w] bit l = masks[n][64 w + l] != 0 (0 past the last pixel).  A wave packs 64 words: one ballot per word, one coalesced store.
__global__ __launch_bounds__(256) void dm_pack_bits_kernel(const uint8_t *__restrict__ masks, long HW, int n_words, unsigned long long *__restrict__ bits) {
  const int n = blockIdx.y, lane = threadIdx.x & 63;
  const int w0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
  if (w0 >= n_words) return;
  const uint8_t *m = masks + (long)n * HW;
  unsigned long long mine = 0;
  for (int i = 0; i < 64 && w0 + i < n_words; ++i) {
    const long px = (long)(w0 + i) * 64 + lane;
    const unsigned long long b = __ballot(px < HW && m[px] != 0);
    if (lane == i) mine = b;
  }
  if (w0 + lane < n_words) bits[(long)n * n_words + w0 + lane] = mine;
}

// inter[i][j] = inter[j][i] = |mask i AND mask j| for j >= i of the same category (the diagonal: the area, also written to area[i]); 0 for
// two categories.  One wave per pair.
__global__ __launch_bounds__(256) void dm_pair_counts_kernel(const unsigned long long *__restrict__ bits, const int *__restrict__ cat, int N, int n_words,
                                                             int *__restrict__ area, int *__restrict__ inter) {
  const int i = blockIdx.y, j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (j >= N || j < i) return;
  int c = 0;
  if (cat[i] == cat[j]) {
    const unsigned long long *a = bits + (long)i * n_words, *b = bits + (long)j * n_words;
    for (int w = lane; w < n_words; w += 64) c += __popcll(a[w] & b[w]);
    c = wave_all_sum(c);
  }
  if (lane == 0) {
    inter[(long)i * N + j] = c;
    inter[(long)j * N + i] = c;
    if (i == j) area[i] = c;
  }
}

// One wavefront: the order (score descending, number ascending) by counting, then the walk.  A proposal is kept iff no kept proposal of
// its category has (double)inter > iou * (double)union with it; keep[] also applies max_per (0: all) to the kept ones of a category in
// that order.  A score that is not a number takes no place in the order and is not kept.
__global__ __launch_bounds__(64) void dm_nms_walk_kernel(const double *__restrict__ score, const int *__restrict__ cat, const int *__restrict__ area,
                                                         const int *__restrict__ inter, int N, double iou, int max_per, uint8_t *__restrict__ keep) {
  __shared__ int order[DM_MAX_MASKS];
  __shared__ int kept[DM_MAX_MASKS];
  const int lane = threadIdx.x;
  for (int i = lane; i < N; i += 64) order[i] = -1;
  wave_lds_handover();
  for (int i = lane; i < N; i += 64) {  // keep[i] has one writer: this lane for a score that is no number, lane 0 at i's turn otherwise
    const double si = score[i];
    if (!(si == si)) {
      keep[i] = 0;
      continue;
    }
    int rank = 0;
    for (int j = 0; j < N; ++j) {
      const double sj = score[j];
      rank += (sj > si || (sj == si && j < i)) ? 1 : 0;
    }
    order[rank] = i;  // rank < N: at most N - 1 others precede
  }
  wave_lds_handover();
  int nk = 0;
  for (int t = 0; t < N; ++t) {
    const int i = order[t];
    if (i < 0) continue;  // uniform
    const int ci = cat[i], ai = area[i];
    bool sup = false;
    int same = 0;
    for (int k = lane; k < nk; k += 64) {
      const int j = kept[k];
      if (cat[j] == ci) {
        ++same;
        const int it = inter[(long)i * N + j];
        const long un = (long)ai + (long)area[j] - (long)it;
        sup = sup || (double)it > iou * (double)un;
      }
    }
    same = wave_all_sum(same);
    const bool stays = __ballot(sup) == 0;
    if (lane == 0) {
      keep[i] = (uint8_t)(stays && (max_per == 0 || same < max_per));
      if (stays) kept[nk] = i;
    }
    if (stays) {
      ++nk;
      wave_lds_handover();
    }
  }
}

}  // namespace
}  // namespace unopose

using namespace unopose;

extern "C" {

int unopose_patch_valid(const void *packed, const int *desc, int K, int img_size, void *out, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(packed && desc && out, "patch_valid: null pointer");
  UNOPOSE_REQUIRE(K >= 1 && K <= 65535 && img_size >= DM_PATCH && img_size <= 4096 && img_size % DM_PATCH == 0,
                  "patch_valid: bad sizes (K=%d img_size=%d)", K, img_size);
  const int side = img_size / DM_PATCH;
  hipLaunchKernelGGL(dm_patch_valid_kernel, dim3(cdiv((long)K * side * side, 256)), dim3(256), 0, (hipStream_t)stream, (const uint8_t *)packed, desc, K,
                     img_size, side, (uint8_t *)out);
  return check_launch("patch_valid");
}

int unopose_token_unit_rows(const void *x, int is_bf16, long rows, int D, void *out, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(x && out, "token_unit_rows: null pointer");
  UNOPOSE_REQUIRE(rows >= 1 && rows < (1L << 31) && D >= 1, "token_unit_rows: bad sizes (rows=%ld D=%d)", rows, D);
  if (is_bf16)
    hipLaunchKernelGGL(dm_unit_rows_kernel<u16>, dim3(cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, (const u16 *)x, rows, D, (u16 *)out);
  else
    hipLaunchKernelGGL(dm_unit_rows_kernel<float>, dim3(cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, (const float *)x, rows, D, (u16 *)out);
  return check_launch("token_unit_rows");
}

int unopose_patch_match_max_tokens(void) { return DM_MAX_T; }

int unopose_patch_match_score(const void *q_unit, const void *q_valid, const void *r_unit, const void *r_valid, int P, int O, int T, int D, float *out,
                              unopose_stream_t stream) {
  UNOPOSE_REQUIRE(q_unit && q_valid && r_unit && r_valid && out, "patch_match_score: null pointer");
  UNOPOSE_REQUIRE(P >= 1 && P <= 65535 && O >= 1 && O <= 65535 && T >= 1 && T <= DM_MAX_T && D >= 32 && D % 32 == 0,
                  "patch_match_score: bad sizes (P=%d O=%d T=%d D=%d; T <= %d, D a multiple of 32)", P, O, T, D, DM_MAX_T);
  UNOPOSE_REQUIRE(((uintptr_t)q_unit | (uintptr_t)r_unit) % 16 == 0, "patch_match_score: token rows must be 16-byte aligned");
  hipLaunchKernelGGL(dm_patch_match_kernel, dim3(O, P), dim3(256), 0, (hipStream_t)stream, (const u16 *)q_unit, (const uint8_t *)q_valid,
                     (const u16 *)r_unit, (const uint8_t *)r_valid, O, T, D, out);
  return check_launch("patch_match_score");
}

int unopose_class_cosine(const void *q_cls, const void *r_cls, int P, int O, int D, float *out, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(q_cls && r_cls && out, "class_cosine: null pointer");
  UNOPOSE_REQUIRE(P >= 1 && P <= 65535 && O >= 1 && O <= 65535 && D >= 1, "class_cosine: bad sizes (P=%d O=%d D=%d)", P, O, D);
  const long pairs = (long)P * O;
  hipLaunchKernelGGL(dm_class_cosine_kernel, dim3(cdiv(pairs, 4)), dim3(256), 0, (hipStream_t)stream, (const u16 *)q_cls, (const u16 *)r_cls, pairs, O, D,
                     out);
  return check_launch("class_cosine");
}

int unopose_mask_nms_max_masks(void) { return DM_MAX_MASKS; }

int unopose_mask_pair_counts(const void *masks, const int *category, int N, int H, int W, void *bits, int *area, int *inter, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(masks && category && bits && area && inter, "mask_pair_counts: null pointer");
  UNOPOSE_REQUIRE(N >= 1 && N <= DM_MAX_MASKS && H >= 1 && W >= 1 && (long)H * W < (1L << 31), "mask_pair_counts: bad sizes (N=%d H=%d W=%d)", N, H, W);
  const long HW = (long)H * W;
  const int n_words = (int)((HW + 63) / 64);
  hipLaunchKernelGGL(dm_pack_bits_kernel, dim3(cdiv(n_words, 256), N), dim3(256), 0, (hipStream_t)stream, (const uint8_t *)masks, HW, n_words,
                     (unsigned long long *)bits);
  hipLaunchKernelGGL(dm_pair_counts_kernel, dim3(cdiv(N, 4), N), dim3(256), 0, (hipStream_t)stream, (const unsigned long long *)bits, category, N,
                     n_words, area, inter);
  return check_launch("mask_pair_counts");
}

int unopose_mask_nms_walk(const double *score, const int *category, const int *area, const int *inter, int N, double nms_iou, int max_per_object,
                          void *keep, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(score && category && area && inter && keep, "mask_nms_walk: null pointer");
  UNOPOSE_REQUIRE(N >= 1 && N <= DM_MAX_MASKS && max_per_object >= 0 && nms_iou == nms_iou, "mask_nms_walk: bad arguments (N=%d max_per_object=%d)", N,
                  max_per_object);
  hipLaunchKernelGGL(dm_nms_walk_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, score, category, area, inter, N, nms_iou, max_per_object,
                     (uint8_t *)keep);
  return check_launch("mask_nms_walk");
}

}  // extern "C"
