// COCO run-length masks on the device, both directions, for all masks of a call at once (they share H x W).  The host functions are
// the specification and the results are held to equality with them: provider.rle_counts_from_string / provider.rle_decode for the
// decode, the BOP toolkit's pycoco_utils.binary_mask_to_rle / bbox_from_binary_mask (= provider.rle_encode) for the encode.
// Runs alternate 0s / 1s starting with 0s over the mask in COLUMN-major order: position p = x * H + y.
//
//   decode
//   * rle_parse: one workgroup per mask.  A compressed string is 5 data bits per byte (value - 48), bit 0x20 = "more", sign taken
//     from bit 0x10 of a number's last byte; a byte starts a number when its predecessor ends one, so the number index of a byte
//     is a prefix count of start bytes and every number is decoded by the thread on its first byte.  Count i >= 3 is coded as a
//     difference to count i - 2: counts 0, 1, 2 are raw, hence two interleaved prefix sums (odd chain from 1, even chain from 2).
//     The run starts are the exclusive prefix sum of the counts, n + 1 int32 per mask, clamped to [0, H * W] and monotone whatever
//     the input; a negative count or a total above H * W sets a flag instead.  The row of `stats` is initialised here.
//   * rle_fill: one thread per OUTPUT pixel in row-major order (coalesced stores): binary search of p in the mask's run starts
//     (staged in LDS when they fit), value = parity of the run, AND depth > 0 when a depth map is given; the count and the
//     extents of the result are reduced per wavefront and added to `stats` with integer atomics (order-free, so deterministic).
//   encode
//   * rle_column_scan: one thread per column (coalesced across the wavefront): boundaries (a pixel that differs from its
//     column-major predecessor; the first pixel's predecessor counts as 0) per column, and per mask their total, the area and
//     the extents.
//   * rle_compact: a workgroup per 64 columns; 64 x 64 tiles go through LDS so that global reads stay coalesced while a wavefront
//     walks a column with ballot + mbcnt compaction; a column's first output slot is the prefix of the column counts.
//   * rle_diff: counts = differences of the boundary positions, closed by H * W.
//   window_masks: the crop of each decoded mask to its window, packed back to back, plus the set pixels per window row --
//     what ops/prep.py's PrepPlan derives from host masks.
//
// Descriptor of mask d for the decode, RLE_DESC int32 (built on the host, ops/rle.py):
//   0 kind (0 list of counts, 1 compressed string)   1 start in the int32 list buffer / the byte buffer   2 its length there
//   3 n (number of counts)   4 start of its n + 1 run starts   5-7 unused
// Descriptor of window k, RLE_DESC int32: 0 mask number  1 y0  2 x0  3 h  4 w  5 start of its h * w bytes  6 start of its h rows
#include "common.h"

namespace unopose {

constexpr int RLE_DESC = 8;
constexpr int RLE_STATS = 6;
constexpr int RLE_FLAG_NEGATIVE = 1, RLE_FLAG_OVERLONG = 2, RLE_FLAG_MALFORMED = 4;
constexpr int RLE_FILL_PIXELS = 4096;  // output pixels per workgroup of rle_fill = run starts it can stage in LDS
constexpr int RLE_MAX_BYTES = 12;      // bytes of one number: 60 data bits

// inclusive prefix sum over the 256 threads of the workgroup, continued from `carry` (the same in every thread, advanced by the
// workgroup's total).  Every thread of the workgroup calls it.
__device__ __forceinline__ long long rle_block_scan(long long v, long long *wave_total, long long &carry) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  v = wave_inclusive_sum(v, lane);
  __syncthreads();  // the previous scan's totals have been read
  if (lane == 63) wave_total[wave] = v;
  __syncthreads();
  long long before = carry, total = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const long long t = wave_total[w];
    if (w < wave) before += t;
    total += t;
  }
  carry += total;
  return v + before;
}

__global__ __launch_bounds__(256) void rle_parse_kernel(const uint8_t *__restrict__ bytes, const int *__restrict__ lists,
                                                        const int *__restrict__ desc, int H, int W, int *__restrict__ starts,
                                                        int *__restrict__ stats) {
  __shared__ long long wave_total[4];
  __shared__ int flag_word;
  const int d = blockIdx.x, tid = threadIdx.x;
  const int *q = desc + d * RLE_DESC;
  const int kind = q[0], src = q[1], len = q[2], n = q[3];
  int *st = starts + q[4];  // n + 1 entries; holds the raw numbers of a string between the two phases
  const long long HW = (long long)H * W;
  int flags = 0;
  if (tid == 0) flag_word = 0;
  __syncthreads();
  if (kind == 1) {
    const uint8_t *s = bytes + src;
    long long numbers = 0;
    for (int c0 = 0; c0 < len; c0 += 256) {
      const int b = c0 + tid;
      const bool first = b < len && (b == 0 || !((s[b - 1] - 48) & 0x20));
      const long long idx = rle_block_scan(first ? 1 : 0, wave_total, numbers) - 1;
      if (first && idx < n) {
        long long x = 0;
        int k = 0, c = 0x20;
        for (int p = b; (c & 0x20) && p < len && k < RLE_MAX_BYTES; ++p, ++k) {
          c = s[p] - 48;
          x |= (long long)(c & 0x1F) << (5 * k);
        }
        if (c & 0x20) {  // no end within the string or within 60 bits
          flags |= RLE_FLAG_MALFORMED;
          x = 0;
        } else if (c & 0x10) {
          x |= -1LL << (5 * k);
        }
        if (x > 2147483647LL || x < -2147483647LL - 1) {
          flags |= RLE_FLAG_MALFORMED;
          x = 0;
        }
        st[idx] = (int)x;
      }
    }
    __syncthreads();  // the raw numbers, written by other threads, are read below
  }
  long long even = 0, odd = 0, run = 0;
  for (int c0 = 0; c0 < n; c0 += 256) {
    const int i = c0 + tid;
    const bool in = i < n;
    long long cnt = in ? (long long)(kind == 1 ? st[i] : lists[src + i]) : 0;
    if (kind == 1) {
      const long long e = rle_block_scan(in && !(i & 1) && i >= 2 ? cnt : 0, wave_total, even);
      const long long o = rle_block_scan(in && (i & 1) ? cnt : 0, wave_total, odd);
      if (i > 0) cnt = (i & 1) ? o : e;
    }
    if (!in) cnt = 0;
    if (cnt < 0) {
      flags |= RLE_FLAG_NEGATIVE;
      cnt = 0;
    }
    const long long begin = rle_block_scan(cnt, wave_total, run) - cnt;
    if (in) st[i] = (int)(begin < HW ? begin : HW);
  }
  if (run > HW) flags |= RLE_FLAG_OVERLONG;
  if (flags) atomicOr(&flag_word, flags);
  __syncthreads();
  if (tid == 0) {
    st[n] = (int)(run < HW ? run : HW);
    int *o = stats + d * RLE_STATS;
    o[0] = 0, o[1] = H, o[2] = 0, o[3] = W, o[4] = 0, o[5] = flag_word;
  }
}

// the run that holds position p: the last i in [0, n) with S[i] <= p (S[0] = 0; zero-length runs repeat a start and lose to the
// run after them, as in the host's slice assignments)
template <typename P>
__device__ __forceinline__ int rle_find_run(P S, int n, int p) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (S[mid] <= p) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void rle_fill_kernel(const int *__restrict__ desc, const int *__restrict__ starts,
                                                       const double *__restrict__ depth, int H, int W, uint8_t *__restrict__ masks,
                                                       int *__restrict__ stats) {
  __shared__ int staged[RLE_FILL_PIXELS];
  const int d = blockIdx.y, tid = threadIdx.x;
  const int *q = desc + d * RLE_DESC;
  const int n = q[3];
  const int *st = starts + q[4];
  const int HW = H * W, total = st[n];
  const bool fits = n + 1 <= RLE_FILL_PIXELS;
  if (fits) {
    for (int i = tid; i <= n; i += 256) staged[i] = st[i];
    __syncthreads();
  }
  uint8_t *out = masks + (size_t)d * HW;
  int count = 0, y_lo = H, y_hi = 0, x_lo = W, x_hi = 0;
  const int first = blockIdx.x * RLE_FILL_PIXELS;
  for (int o = first + tid; o < min(HW, first + RLE_FILL_PIXELS); o += 256) {
    const int y = o / W, x = o - y * W, p = x * H + y;
    int v = 0;
    if (p < total) v = (fits ? rle_find_run(staged, n, p) : rle_find_run(st, n, p)) & 1;
    if (depth != nullptr && !(depth[o] > 0.0)) v = 0;
    out[o] = (uint8_t)v;
    if (v) {
      ++count;
      y_lo = min(y_lo, y), y_hi = max(y_hi, y + 1), x_lo = min(x_lo, x), x_hi = max(x_hi, x + 1);
    }
  }
  count = wave_all_sum(count);
  y_lo = wave_all_min(y_lo), y_hi = wave_all_max(y_hi), x_lo = wave_all_min(x_lo), x_hi = wave_all_max(x_hi);
  if ((tid & 63) == 0 && count > 0) {
    int *o = stats + d * RLE_STATS;
    atomicAdd(o + 0, count);
    atomicMin(o + 1, y_lo), atomicMax(o + 2, y_hi), atomicMin(o + 3, x_lo), atomicMax(o + 4, x_hi);
  }
}

// totals (zero before the launch), 6 int32 per mask: boundaries, area, H - y_first, y_last + 1, W - x_first, x_last + 1
__global__ __launch_bounds__(256) void rle_column_scan_kernel(const uint8_t *__restrict__ masks, int H, int W, int *__restrict__ col_count,
                                                              int *__restrict__ totals) {
  const int d = blockIdx.y, x = blockIdx.x * 256 + threadIdx.x;
  const uint8_t *m = masks + (size_t)d * H * W;
  int nb = 0, area = 0, top = 0, bottom = 0;
  if (x < W) {
    bool prev = x > 0 && m[(size_t)(H - 1) * W + x - 1] != 0;
    for (int y = 0; y < H; ++y) {
      const bool v = m[(size_t)y * W + x] != 0;
      nb += v != prev;
      if (v) {
        ++area;
        top = max(top, H - y), bottom = y + 1;
      }
      prev = v;
    }
    col_count[(size_t)d * W + x] = nb;
  }
  const int left = area > 0 ? W - x : 0, right = area > 0 ? x + 1 : 0;
  const int s_nb = wave_all_sum(nb), s_area = wave_all_sum(area);
  const int m_top = wave_all_max(top), m_bottom = wave_all_max(bottom), m_left = wave_all_max(left), m_right = wave_all_max(right);
  if ((threadIdx.x & 63) == 0 && s_nb + s_area > 0) {
    int *o = totals + d * RLE_STATS;
    atomicAdd(o + 0, s_nb), atomicAdd(o + 1, s_area);
    atomicMax(o + 2, m_top), atomicMax(o + 3, m_bottom), atomicMax(o + 4, m_left), atomicMax(o + 5, m_right);
  }
}

// off[d] = start of mask d's counts in the output (boundaries + 1 of them); the boundary positions go to pos[off[d] ...] in order
__global__ __launch_bounds__(256) void rle_compact_kernel(const uint8_t *__restrict__ masks, const int *__restrict__ col_count,
                                                          const long long *__restrict__ off, int H, int W, int *__restrict__ pos) {
  __shared__ uint8_t tile[64][68];  // [row][column]; 68: a wavefront reading one column touches 32 distinct banks
  __shared__ long long col_base[64];
  __shared__ long long wave_total[4];
  const int d = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, x0 = blockIdx.x * 64;
  const uint8_t *m = masks + (size_t)d * H * W;
  const int *cc = col_count + (size_t)d * W;
  const long long begin = off[d], end = off[d + 1] - 1;  // the last slot is the closing count's
  long long before = 0;
  for (int i = tid; i < x0; i += 256) before += cc[i];
  long long carry = 0;
  rle_block_scan(before, wave_total, carry);  // carry = boundaries of the columns left of this tile
  if (wave == 0) {
    const long long c = x0 + lane < W ? cc[x0 + lane] : 0;
    col_base[lane] = begin + carry + wave_inclusive_sum(c, lane) - c;
  }
  for (int y0 = 0; y0 < H; y0 += 64) {
    __syncthreads();  // col_base written; the previous tile has been read
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int r = wave + 4 * k, yy = y0 + r, xx = x0 + lane;
      tile[r][lane] = yy < H && xx < W && m[(size_t)yy * W + xx] != 0;
    }
    __syncthreads();
    const int yy = y0 + lane;
    for (int c = wave; c < 64 && x0 + c < W; c += 4) {  // a column belongs to one wavefront for the whole walk
      const int xx = x0 + c;
      const bool v = tile[lane][c] != 0;
      bool prev;
      if (lane > 0) prev = tile[lane - 1][c] != 0;
      else if (y0 > 0) prev = m[(size_t)(y0 - 1) * W + xx] != 0;
      else prev = xx > 0 && m[(size_t)(H - 1) * W + xx - 1] != 0;
      const bool hit = yy < H && v != prev;
      const unsigned long long ballot = __ballot(hit);
      const int pre = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
      const long long base = col_base[c];
      if (hit && base + pre < end) pos[base + pre] = xx * H + yy;
      if (lane == 0) col_base[c] = base + __popcll(ballot);
    }
  }
}

__global__ __launch_bounds__(256) void rle_diff_kernel(const int *__restrict__ pos, const long long *__restrict__ off, int HW,
                                                       int *__restrict__ counts) {
  const int d = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  const long long begin = off[d], n = off[d + 1] - begin;
  if (i >= n) return;
  const int cur = i < n - 1 ? pos[begin + i] : HW, prev = i > 0 ? pos[begin + i - 1] : 0;
  counts[begin + i] = cur - prev;
}

__global__ __launch_bounds__(256) void window_masks_kernel(const uint8_t *__restrict__ masks, const int *__restrict__ desc, int H, int W,
                                                           uint8_t *__restrict__ packed, int *__restrict__ row_counts) {
  const int k = blockIdx.y, lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int *q = desc + k * RLE_DESC;
  const int y0 = q[1], x0 = q[2], h = q[3], w = q[4];
  if (r >= h) return;  // whole wavefronts leave together: a row belongs to one wavefront
  const uint8_t *src = masks + ((size_t)q[0] * H + y0 + r) * W + x0;
  uint8_t *dst = packed + (size_t)q[5] + (size_t)r * w;
  int count = 0;
  for (int c0 = 0; c0 < w; c0 += 64) {
    const int c = c0 + lane;
    const bool hit = c < w && src[c] != 0;
    if (c < w) dst[c] = hit;
    count += __popcll(__ballot(hit));
  }
  if (lane == 0) row_counts[q[6] + r] = count;
}

}  // namespace unopose

using namespace unopose;

extern "C" {

int unopose_rle_desc_ints(void) { return RLE_DESC; }
int unopose_rle_stats_ints(void) { return RLE_STATS; }

int unopose_rle_parse(const void *bytes, const int *lists, const int *desc, int D, int H, int W, int *starts, int *stats,
                      unopose_stream_t stream) {
  UNOPOSE_REQUIRE(bytes && lists && desc && starts && stats, "rle_parse: null pointer");
  UNOPOSE_REQUIRE(D >= 1 && D <= 65535 && H >= 1 && W >= 1 && (long)H * W < (1L << 31), "rle_parse: bad sizes (D=%d H=%d W=%d)", D, H, W);
  hipLaunchKernelGGL(rle_parse_kernel, dim3(D), dim3(256), 0, (hipStream_t)stream, (const uint8_t *)bytes, lists, desc, H, W, starts, stats);
  return check_launch("rle_parse");
}

int unopose_rle_fill(const int *desc, const int *starts, const double *depth, int D, int H, int W, void *masks, int *stats,
                     unopose_stream_t stream) {
  UNOPOSE_REQUIRE(desc && starts && masks && stats, "rle_fill: null pointer");
  UNOPOSE_REQUIRE(D >= 1 && D <= 65535 && H >= 1 && W >= 1 && (long)H * W < (1L << 31), "rle_fill: bad sizes (D=%d H=%d W=%d)", D, H, W);
  hipLaunchKernelGGL(rle_fill_kernel, dim3(cdiv((long)H * W, RLE_FILL_PIXELS), D), dim3(256), 0, (hipStream_t)stream, desc, starts, depth, H, W,
                     (uint8_t *)masks, stats);
  return check_launch("rle_fill");
}

int unopose_rle_column_scan(const void *masks, int D, int H, int W, int *col_count, int *totals, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(masks && col_count && totals, "rle_column_scan: null pointer");
  UNOPOSE_REQUIRE(D >= 1 && D <= 65535 && H >= 1 && W >= 1 && (long)H * W < (1L << 31), "rle_column_scan: bad sizes (D=%d H=%d W=%d)", D, H, W);
  hipLaunchKernelGGL(rle_column_scan_kernel, dim3(cdiv(W, 256), D), dim3(256), 0, (hipStream_t)stream, (const uint8_t *)masks, H, W, col_count,
                     totals);
  return check_launch("rle_column_scan");
}

int unopose_rle_compact(const void *masks, const int *col_count, const void *off, int D, int H, int W, int *pos, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(masks && col_count && off && pos, "rle_compact: null pointer");
  UNOPOSE_REQUIRE(D >= 1 && D <= 65535 && H >= 1 && W >= 1 && (long)H * W < (1L << 31), "rle_compact: bad sizes (D=%d H=%d W=%d)", D, H, W);
  hipLaunchKernelGGL(rle_compact_kernel, dim3(cdiv(W, 64), D), dim3(256), 0, (hipStream_t)stream, (const uint8_t *)masks, col_count,
                     (const long long *)off, H, W, pos);
  return check_launch("rle_compact");
}

int unopose_rle_diff(const int *pos, const void *off, int D, int max_n, int H, int W, int *counts, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(pos && off && counts, "rle_diff: null pointer");
  UNOPOSE_REQUIRE(D >= 1 && D <= 65535 && max_n >= 1 && H >= 1 && W >= 1 && (long)H * W < (1L << 31),
                  "rle_diff: bad sizes (D=%d max_n=%d H=%d W=%d)", D, max_n, H, W);
  hipLaunchKernelGGL(rle_diff_kernel, dim3(cdiv(max_n, 256), D), dim3(256), 0, (hipStream_t)stream, pos, (const long long *)off, H * W, counts);
  return check_launch("rle_diff");
}

int unopose_window_masks(const void *masks, const int *desc, int K, int max_h, int H, int W, void *packed, int *row_counts,
                         unopose_stream_t stream) {
  UNOPOSE_REQUIRE(masks && desc && packed && row_counts, "window_masks: null pointer");
  UNOPOSE_REQUIRE(K >= 1 && K <= 65535 && max_h >= 1 && max_h <= H && W >= 1, "window_masks: bad sizes (K=%d max_h=%d H=%d W=%d)", K, max_h, H, W);
  hipLaunchKernelGGL(window_masks_kernel, dim3(cdiv(max_h, 4), K), dim3(256), 0, (hipStream_t)stream, (const uint8_t *)masks, desc, H, W,
                     (uint8_t *)packed, row_counts);
  return check_launch("window_masks");
}

}  // extern "C"
