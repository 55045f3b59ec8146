// Training items from rendered views (unopose_amd/provider_online.py): everything per PIXEL and per POINT of a (query, reference) pair,
// for all views of a chunk at once.  `provider_online.items_from_views_host` is the specification and the results are held to equality
// with it, so every float64 expression below keeps its evaluation order (the build's -ffp-contract=off keeps them as written) and every
// float64 sum its stated order:
//   * items_view_rows / items_view_table: per view the visible mask of the object against an occluder (object depth > 0 and no occluder
//     there or the object not behind it), the scene depth and colour (the nearer surface; background 0), the optional dilation (the L1
//     ball of radius 4 clipped to the image = provider_train.dilate_cross(mask, 4)), per row the full / visible / final counts and the
//     extents of the final mask (wave ballots), per view their totals and extents (integer sums: no order to keep, no atomics);
//   * items_points: one workgroup per view, from the window the host derived: per window row the set count, the row-major rank of every
//     set pixel (row prefix + in-row popcount), for a query the float64 lift (provider.lift_depth on depth * 0.001), the centroid (each
//     row summed left to right by one lane, the row sums added top to bottom by one lane), the keep rule |p - mean| < 1.2 radius and
//     the ordered compaction of the kept pixels; then the draw (draw_index below = provider_online.draw_index), the gather into float32
//     points (rounded once, after the shift + noise or the spin) and int64 crop indices (Window.to_resized in float64); for a reference
//     the mean of the drawn points in draw order and the radius;
//   * items_crops: the window crops of the scene colours and masks in the atlas layout ops.finish_crops reads.
// The kernels trust their descriptors: ops/items.py builds and range-checks them on the host.
//
// View table, ITEM_TABLE int32 per view: 0 full (object pixels), 1 visible, 2 set (final mask), 3 top, 4 bottom, 5 left, 6 right (half-open
// extents of the final mask; H, 0, W, 0 when empty), 7 unused.
// Point descriptor, ITEM_DESC int32 per view: 0 source view, 1 y0, 2 x0, 3 h, 4 w (window), 5 pair, 6 valid.
// Crop descriptor, ITEM_CROP int32 per crop: 0 source view, 1 y0, 2 x0, 3 h, 4 w, 5 atlas row, 6 mask offset, 7 unused.
// Pair constants, ITEM_PAIR float64 per pair: 0..8 spin (row-major), 9..11 shift.
#include "common.h"
#include "item_mix.h"

namespace unopose {

constexpr int ITEM_TABLE = 8, ITEM_DESC = 8, ITEM_CROP = 8, ITEM_PAIR = 12, ITEM_ROW = 5;
constexpr int ITEM_MIN_KEPT = 32, ITEM_DILATE = 4, ITEM_ROUNDS = 6;
constexpr double ITEM_DEPTH_TO_M = 0.001;

// provider_online.draw_index: more than wanted -> a keyed bijection of [0, n_have) (balanced Feistel network over the next even number of
// bits, walked until it lands inside: the walk ends, i itself is on the cycle); else a keyed hash modulo n_have
__device__ __forceinline__ int item_draw_index(unsigned long long key, unsigned i, unsigned n_have, unsigned n_want) {
  const unsigned long long gold = 0x9e3779b97f4a7c15ull;
  if (n_have > n_want) {
    int k = 1;
    while ((1ull << (2 * k)) < (unsigned long long)n_have) ++k;
    const unsigned mask = (1u << k) - 1u;
    unsigned x = i;
    do {
      unsigned L = x >> k, R = x & mask;
      for (int r = 0; r < ITEM_ROUNDS; ++r) {
        const unsigned t = L ^ ((unsigned)item_mix(key + gold * (unsigned long long)(r + 1) + (unsigned long long)R) & mask);
        L = R, R = t;
      }
      x = (L << k) | R;
    } while (x >= n_have);
    return (int)x;
  }
  return (int)(item_mix(key ^ item_mix((unsigned long long)i + gold)) % (unsigned long long)n_have);
}

__device__ __forceinline__ bool item_visible(const float *__restrict__ od, const float *__restrict__ cd, size_t at) {
  const float o = od[at];
  if (!(o > 0.f)) return false;
  if (cd == nullptr) return true;
  const float c = cd[at];
  return !(c > 0.f) || o <= c;
}

// one wavefront per image row; occ_slot[v] = the view's occluder canvas, -1 = none
__global__ __launch_bounds__(256) void items_view_rows_kernel(const float *__restrict__ obj_depth, const uint8_t *__restrict__ obj_rgb,
                                                              const float *__restrict__ occ_depth, const uint8_t *__restrict__ occ_rgb,
                                                              const int *__restrict__ occ_slot, const int *__restrict__ dilate, int H, int W,
                                                              uint8_t *__restrict__ mask, float *__restrict__ scene_depth,
                                                              uint8_t *__restrict__ scene_rgb, int *__restrict__ rows) {
  const int v = blockIdx.y, lane = threadIdx.x & 63, y = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (y >= H) return;  // whole wavefronts leave together
  const size_t plane = (size_t)H * W;
  const float *od = obj_depth + (size_t)v * plane;
  const uint8_t *oc = obj_rgb + (size_t)v * plane * 3;
  const int slot = occ_slot[v];
  const float *cd = slot >= 0 ? occ_depth + (size_t)slot * plane : nullptr;
  const uint8_t *cc = slot >= 0 ? occ_rgb + (size_t)slot * plane * 3 : nullptr;
  const bool grow = dilate[v] != 0;
  int n_full = 0, n_vis = 0, n_set = 0, left = W, right = 0;
  for (int c0 = 0; c0 < W; c0 += 64) {
    const int x = c0 + lane;
    const bool in = x < W;
    bool full = false, vis = false, set = false;
    if (in) {
      const size_t at = (size_t)y * W + x;
      const float o = od[at], c = cd ? cd[at] : 0.f;
      full = o > 0.f;
      vis = item_visible(od, cd, at);
      set = vis;
      if (grow && !set) {
        for (int dy = -ITEM_DILATE; dy <= ITEM_DILATE && !set; ++dy) {
          const int yy = y + dy, reach = ITEM_DILATE - (dy < 0 ? -dy : dy);
          if (yy < 0 || yy >= H) continue;
          for (int xx = max(x - reach, 0); xx <= min(x + reach, W - 1) && !set; ++xx) set = item_visible(od, cd, (size_t)yy * W + xx);
        }
      }
      const bool front = !vis && c > 0.f;  // the occluder is the nearer surface (or the only one)
      scene_depth[(size_t)v * plane + at] = vis ? o : front ? c : 0.f;
      uint8_t *px = scene_rgb + ((size_t)v * plane + at) * 3;
#pragma unroll
      for (int k = 0; k < 3; ++k) px[k] = vis ? oc[at * 3 + k] : front ? cc[at * 3 + k] : (uint8_t)0;
      mask[(size_t)v * plane + at] = set ? 1 : 0;
    }
    const unsigned long long b_full = __ballot(full), b_vis = __ballot(vis), b_set = __ballot(set);
    n_full += __popcll(b_full), n_vis += __popcll(b_vis), n_set += __popcll(b_set);
    if (b_set) {
      left = min(left, c0 + (int)__ffsll((long long)b_set) - 1);
      right = max(right, c0 + 64 - (int)__clzll((long long)b_set));
    }
  }
  if (lane == 0) {
    int *o = rows + ((size_t)v * H + y) * ITEM_ROW;
    o[0] = n_full, o[1] = n_vis, o[2] = n_set, o[3] = left, o[4] = right;
  }
}

// one wavefront per view over its rows' records
__global__ __launch_bounds__(64) void items_view_table_kernel(const int *__restrict__ rows, int H, int W, int *__restrict__ table) {
  const int v = blockIdx.x, lane = threadIdx.x;
  int n_full = 0, n_vis = 0, n_set = 0, top = H, bottom = 0, left = W, right = 0;
  for (int y = lane; y < H; y += 64) {
    const int *r = rows + ((size_t)v * H + y) * ITEM_ROW;
    n_full += r[0], n_vis += r[1], n_set += r[2];
    if (r[2] > 0) top = min(top, y), bottom = max(bottom, y + 1), left = min(left, r[3]), right = max(right, r[4]);
  }
  n_full = wave_all_sum(n_full), n_vis = wave_all_sum(n_vis), n_set = wave_all_sum(n_set);
  top = wave_all_min(top), bottom = wave_all_max(bottom), left = wave_all_min(left), right = wave_all_max(right);
  if (lane == 0) {
    int *o = table + (size_t)v * ITEM_TABLE;
    o[0] = n_full, o[1] = n_vis, o[2] = n_set, o[3] = top, o[4] = bottom, o[5] = left, o[6] = right, o[7] = 0;
  }
}

struct ItemCamera {
  double fx, fy, cx, cy;
};

// provider.lift_depth of window pixel (r, c) on depth * 0.001, float64, its evaluation order
__device__ __forceinline__ void item_lift(const float *__restrict__ depth, int W, int y0, int x0, int r, int c, const ItemCamera &cam, double &X,
                                          double &Y, double &Z) {
  const double z = (double)depth[(size_t)(y0 + r) * W + x0 + c] * ITEM_DEPTH_TO_M;
  const double u = (double)(x0 + c) - cam.cx, v = (double)(y0 + r) - cam.cy;
  X = (u * z) / cam.fx, Y = (v * z) / cam.fy, Z = z;
}

// One workgroup per view of `desc`.  is_ref: references (draw from all set pixels, spin, radius out); else queries (keep rule against
// radius[pair], shift + noise).  Scratch per view: win_rows / row_base (max_side int32), pix / kept (max_side^2 int32), row_sums (3 max_side
// float64), drawn (3 n_want float64).  Outputs per view: counts[2 d] = set window pixels, counts[2 d + 1] = kept (= set for a reference),
// pts (n_want, 3) float32, choose (n_want) int64.
__global__ __launch_bounds__(256) void items_points_kernel(const uint8_t *__restrict__ mask, const float *__restrict__ scene_depth, int H, int W,
                                                           const int *__restrict__ desc, const double *__restrict__ pair_consts,
                                                           const unsigned long long *__restrict__ keys, const double *__restrict__ noise,
                                                           ItemCamera cam, int is_ref, int n_want, int S, int max_side,
                                                           int *__restrict__ win_rows, int *__restrict__ row_base, int *__restrict__ pix,
                                                           int *__restrict__ kept, double *__restrict__ row_sums, double *__restrict__ drawn,
                                                           double *__restrict__ radius, int *__restrict__ counts, float *__restrict__ pts,
                                                           long *__restrict__ choose) {
  __shared__ int s_n, s_wave[4], s_base;
  __shared__ double s_mean[3], s_red[4];
  const int d = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int *q = desc + (size_t)d * ITEM_DESC;
  const int v = q[0], y0 = q[1], x0 = q[2], h = q[3], w = q[4], pair = q[5];
  if (!q[6]) {  // no window: nothing of this view is read
    if (tid == 0) counts[2 * d] = 0, counts[2 * d + 1] = 0;
    return;
  }
  const size_t plane = (size_t)H * W;
  const uint8_t *m = mask + (size_t)v * plane;
  const float *depth = scene_depth + (size_t)v * plane;
  int *rows = win_rows + (size_t)d * max_side, *base = row_base + (size_t)d * max_side;
  int *px = pix + (size_t)d * max_side * max_side, *kp = kept + (size_t)d * max_side * max_side;
  double *rs = row_sums + (size_t)d * max_side * 3, *dr = drawn + (size_t)d * n_want * 3;

  // set pixels per window row
  for (int r = wid; r < h; r += 4) {
    const uint8_t *mr = m + (size_t)(y0 + r) * W + x0;
    int n = 0;
    for (int c0 = 0; c0 < w; c0 += 64) n += __popcll(__ballot(c0 + lane < w && mr[c0 + lane] != 0));
    if (lane == 0) rows[r] = n;
  }
  __syncthreads();
  if (tid == 0) {
    int n = 0;
    for (int r = 0; r < h; ++r) base[r] = n, n += rows[r];
    s_n = n;
  }
  __syncthreads();
  const int n_set = s_n;
  if (n_set == 0) {
    if (tid == 0) counts[2 * d] = 0, counts[2 * d + 1] = 0;
    return;
  }
  // np.flatnonzero of the window mask: rank = row prefix + in-row popcount
  for (int r = wid; r < h; r += 4) {
    const uint8_t *mr = m + (size_t)(y0 + r) * W + x0;
    int at = base[r];
    for (int c0 = 0; c0 < w; c0 += 64) {
      const int c = c0 + lane;
      const bool hit = c < w && mr[c] != 0;
      const unsigned long long ballot = __ballot(hit);
      const int pre = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
      if (hit) px[at + pre] = r * w + c;
      at += __popcll(ballot);
    }
  }
  __syncthreads();

  const int *have = px;
  int n_have = n_set;
  if (!is_ref) {
    // centroid of the set pixels: a row left to right, then the rows top to bottom
    for (int r = tid; r < h; r += 256) {
      const uint8_t *mr = m + (size_t)(y0 + r) * W + x0;
      double sx = 0.0, sy = 0.0, sz = 0.0;
      for (int c = 0; c < w; ++c)
        if (mr[c] != 0) {
          double X, Y, Z;
          item_lift(depth, W, y0, x0, r, c, cam, X, Y, Z);
          sx += X, sy += Y, sz += Z;
        }
      rs[3 * r + 0] = sx, rs[3 * r + 1] = sy, rs[3 * r + 2] = sz;
    }
    __syncthreads();
    if (tid == 0) {
      double sx = 0.0, sy = 0.0, sz = 0.0;
      for (int r = 0; r < h; ++r) sx += rs[3 * r + 0], sy += rs[3 * r + 1], sz += rs[3 * r + 2];
      s_mean[0] = sx / (double)n_set, s_mean[1] = sy / (double)n_set, s_mean[2] = sz / (double)n_set;
      s_base = 0;
    }
    __syncthreads();
    const double limit = 1.2 * radius[pair], mx = s_mean[0], my = s_mean[1], mz = s_mean[2];
    // the kept pixels, in order: 256 candidates at a time
    for (int j0 = 0; j0 < n_set; j0 += 256) {
      const int j = j0 + tid;
      bool keep = false;
      int flat = 0;
      if (j < n_set) {
        flat = px[j];
        const int r = flat / w, c = flat - r * w;
        double X, Y, Z;
        item_lift(depth, W, y0, x0, r, c, cam, X, Y, Z);
        const double dx = X - mx, dy = Y - my, dz = Z - mz;
        keep = sqrt((dx * dx + dy * dy) + dz * dz) < limit;
      }
      const unsigned long long ballot = __ballot(keep);
      const int pre = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
      if (lane == 0) s_wave[wid] = __popcll(ballot);
      __syncthreads();
      int before = s_base;
      for (int k = 0; k < wid; ++k) before += s_wave[k];
      if (keep) kp[before + pre] = flat;
      __syncthreads();
      if (tid == 0) s_base += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
      __syncthreads();
    }
    have = kp, n_have = s_base;
  }
  if (tid == 0) counts[2 * d] = n_set, counts[2 * d + 1] = n_have;
  if (n_have < (is_ref ? 1 : ITEM_MIN_KEPT)) return;  // the whole workgroup: n_have is uniform

  const double *pc = pair_consts + (size_t)pair * ITEM_PAIR;
  const unsigned long long key = keys[2 * pair + (is_ref ? 0 : 1)];
  const double sr = (double)S / (double)w, sc = (double)S / (double)h;
  for (int i = tid; i < n_want; i += 256) {
    const int flat = have[item_draw_index(key, (unsigned)i, (unsigned)n_have, (unsigned)n_want)];
    const int r = flat / w, c = flat - r * w;
    double X, Y, Z;
    item_lift(depth, W, y0, x0, r, c, cam, X, Y, Z);
    const size_t o = (size_t)d * n_want + i;
    // Window.to_resized: rows and columns alike are decomposed with the window HEIGHT (windows are square), scaled in float64, floored
    const int rr = flat / h, cc = flat - rr * h;
    choose[o] = (long)(floor((double)rr * sr) * (double)S + floor((double)cc * sc));
    if (is_ref) {
      dr[3 * i + 0] = X, dr[3 * i + 1] = Y, dr[3 * i + 2] = Z;
#pragma unroll
      for (int k = 0; k < 3; ++k) pts[3 * o + k] = (float)((X * pc[k] + Y * pc[3 + k]) + Z * pc[6 + k]);  // row vector times spin
    } else {
      const double *z = noise + ((size_t)pair * n_want + i) * 3;
      pts[3 * o + 0] = (float)(X + (pc[9] + 0.001 * z[0]));
      pts[3 * o + 1] = (float)(Y + (pc[10] + 0.001 * z[1]));
      pts[3 * o + 2] = (float)(Z + (pc[11] + 0.001 * z[2]));
    }
  }
  if (!is_ref) return;
  __syncthreads();
  if (tid == 0) {  // the mean of the drawn points, in draw order
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int i = 0; i < n_want; ++i) sx += dr[3 * i + 0], sy += dr[3 * i + 1], sz += dr[3 * i + 2];
    s_mean[0] = sx / (double)n_want, s_mean[1] = sy / (double)n_want, s_mean[2] = sz / (double)n_want;
  }
  __syncthreads();
  double far = 0.0;
  for (int i = tid; i < n_want; i += 256) {
    const double dx = dr[3 * i + 0] - s_mean[0], dy = dr[3 * i + 1] - s_mean[1], dz = dr[3 * i + 2] - s_mean[2];
    far = fmax(far, sqrt((dx * dx + dy * dy) + dz * dz));
  }
  far = wave_all_fmax(far);
  if (lane == 0) s_red[wid] = far;
  __syncthreads();
  if (tid == 0) radius[pair] = fmax(fmax(s_red[0], s_red[1]), fmax(s_red[2], s_red[3]));
}

// one wavefront per window row of a crop: colours into the atlas (AW pixels wide), mask bytes into the packed masks
__global__ __launch_bounds__(256) void items_crops_kernel(const uint8_t *__restrict__ mask, const uint8_t *__restrict__ scene_rgb, int H, int W,
                                                          const int *__restrict__ desc, int AW, uint8_t *__restrict__ atlas,
                                                          uint8_t *__restrict__ packed) {
  const int d = blockIdx.y, lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int *q = desc + (size_t)d * ITEM_CROP;
  const int v = q[0], y0 = q[1], x0 = q[2], h = q[3], w = q[4];
  if (r >= h) return;
  const size_t src = ((size_t)v * H + y0 + r) * W + x0;
  uint8_t *arow = atlas + (size_t)(q[5] + r) * AW * 3, *mrow = packed + (size_t)q[6] + (size_t)r * w;
  for (int c = lane; c < w; c += 64) {
    mrow[c] = mask[src + c];
#pragma unroll
    for (int k = 0; k < 3; ++k) arow[3 * c + k] = scene_rgb[(src + c) * 3 + k];
  }
}

}  // namespace unopose

using namespace unopose;

extern "C" {

int unopose_items_ints(int what) {
  const int v[] = {ITEM_TABLE, ITEM_DESC, ITEM_CROP, ITEM_PAIR, ITEM_ROW, ITEM_MIN_KEPT};
  return what >= 0 && what < 6 ? v[what] : -1;
}

int unopose_items_views(const float *obj_depth, const void *obj_rgb, const float *occ_depth, const void *occ_rgb, const int *occ_slot,
                        const int *dilate, int V, int H, int W, void *mask, float *scene_depth, void *scene_rgb, int *rows, int *table,
                        unopose_stream_t stream) {
  UNOPOSE_REQUIRE(obj_depth && obj_rgb && occ_slot && dilate && mask && scene_depth && scene_rgb && rows && table, "items_views: null pointer");
  UNOPOSE_REQUIRE(V >= 1 && V <= 65535 && H >= 1 && W >= 1 && (long)H * W < (1l << 31), "items_views: bad sizes (V=%d H=%d W=%d)", V, H, W);
  hipLaunchKernelGGL(items_view_rows_kernel, dim3(cdiv(H, 4), V), dim3(256), 0, (hipStream_t)stream, obj_depth, (const uint8_t *)obj_rgb,
                     occ_depth, (const uint8_t *)occ_rgb, occ_slot, dilate, H, W, (uint8_t *)mask, scene_depth, (uint8_t *)scene_rgb, rows);
  if (int rc = check_launch("items_view_rows")) return rc;
  hipLaunchKernelGGL(items_view_table_kernel, dim3(V), dim3(64), 0, (hipStream_t)stream, rows, H, W, table);
  return check_launch("items_view_table");
}

int unopose_items_points(const void *mask, const float *scene_depth, int H, int W, const int *desc, const double *pair_consts, const void *keys,
                         const double *noise, double fx, double fy, double cx, double cy, int D, int is_ref, int n_want, int S, int max_side,
                         int *win_rows, int *row_base, int *pix, int *kept, double *row_sums, double *drawn, double *radius, int *counts,
                         float *pts, void *choose, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(mask && scene_depth && desc && pair_consts && keys && win_rows && row_base && pix && kept && row_sums && drawn && radius &&
                      counts && pts && choose && (is_ref || noise),
                  "items_points: null pointer");
  UNOPOSE_REQUIRE(H >= 1 && W >= 1 && D >= 1 && D <= 65535 && n_want >= 1 && S >= 1 && S <= 4096 && max_side >= 1 && max_side <= 32767,
                  "items_points: bad sizes (H=%d W=%d D=%d n_want=%d S=%d max_side=%d)", H, W, D, n_want, S, max_side);
  const ItemCamera cam = {fx, fy, cx, cy};
  hipLaunchKernelGGL(items_points_kernel, dim3(D), dim3(256), 0, (hipStream_t)stream, (const uint8_t *)mask, scene_depth, H, W, desc, pair_consts,
                     (const unsigned long long *)keys, noise, cam, is_ref, n_want, S, max_side, win_rows, row_base, pix, kept, row_sums, drawn,
                     radius, counts, pts, (long *)choose);
  return check_launch("items_points");
}

int unopose_items_crops(const void *mask, const void *scene_rgb, int H, int W, const int *desc, int D, int max_h, int AW, void *atlas, void *packed,
                        unopose_stream_t stream) {
  UNOPOSE_REQUIRE(mask && scene_rgb && desc && atlas && packed, "items_crops: null pointer");
  UNOPOSE_REQUIRE(H >= 1 && W >= 1 && D >= 1 && D <= 65535 && max_h >= 1 && max_h <= H && AW >= 1, "items_crops: bad sizes (H=%d W=%d D=%d max_h=%d AW=%d)",
                  H, W, D, max_h, AW);
  hipLaunchKernelGGL(items_crops_kernel, dim3(cdiv(max_h, 4), D), dim3(256), 0, (hipStream_t)stream, (const uint8_t *)mask,
                     (const uint8_t *)scene_rgb, H, W, desc, AW, (uint8_t *)atlas, (uint8_t *)packed);
  return check_launch("items_crops");
}

}  // extern "C"
