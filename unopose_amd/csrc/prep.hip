// Query-side instance preparation of the BOP test provider (unopose_amd/provider.py) on the device: everything per PIXEL of a
// detection's window, for all detections of an image at once.  The provider's own functions are the specification and the results
// are held to equality with them, so every expression below keeps their evaluation order (the build's -ffp-contract=off keeps the
// float64 ones as written):
//   * prep_crop_resize: window -> (mask) -> OpenCV's 11-bit fixed-point bilinear resize (provider.resize_bilinear_u8: equal-size
//     copy, exact-2x area shortcut, two-tap passes with host-built tap tables) -> ImageNet normalisation through a 256 x 3 table
//     that provider.to_tensor_normalize filled (so the fp32 bits are its bits);
//   * prep_compact_lift: the set pixels of the window mask in row-major order (np.flatnonzero) -- one wavefront per window row,
//     ballot + mbcnt prefix inside the row, the row's start from a host-built prefix of the row counts -- back-projected in
//     float64 (provider.lift_depth), plus one float64 partial sum per row for the centroid;
//   * prep_distances: centroid (row partials summed in a fixed order: the result does not depend on the launch) and every point's
//     float64 distance to it;
//   * prep_gather: the drawn samples: cloud rows rounded once to fp32, window pixel -> resized-crop index (Window.to_resized).
// These are latency-bound kernels over at most a few hundred thousand pixels per detection: coalesced access, one launch per
// stage per image, nothing more.
//
// Descriptor of detection d, PREP_DESC int32 (built and range-checked on the host, ops/prep.py):
//   0 y0, 1 x0 (window origin in the image)   2 h, 3 w (window size)    4 mask_off (start of its h*w mask bytes)
//   5 pt_off (start of its points in the compacted arrays)   6 n (number of set mask pixels)   7 row_off (start of its h rows in
//   row_base / row_sums)   8 mode (0 copy, 1 2x area, 2 bilinear)   9 tap_x, 10 tap_y (starts of its 4*S tap tables)   11 unused
#include "common.h"

namespace unopose {

constexpr int PREP_DESC = 12;
constexpr int PREP_DIST_PER_BLOCK = 2048;

__global__ __launch_bounds__(256) void prep_crop_resize_kernel(const uint8_t *__restrict__ img, int W, int C, const int *__restrict__ desc,
                                                               const int *__restrict__ taps, const uint8_t *__restrict__ masks,
                                                               const float *__restrict__ lut, int S, int bgr, int use_mask,
                                                               float *__restrict__ out) {
  const int d = blockIdx.y, o = blockIdx.x * 256 + threadIdx.x;
  if (o >= S * S) return;
  const int *q = desc + d * PREP_DESC;
  const int y0 = q[0], x0 = q[1], w = q[3], mode = q[8];
  const uint8_t *m = masks + q[4];
  const int oy = o / S, ox = o - oy * S;
  // the (up to) four source pixels of this output pixel, in window coordinates, and their weights
  int ra = oy, rb = oy, ca = ox, cb = ox, a0 = 0, a1 = 0, b0 = 0, b1 = 0;
  if (mode == 1) {
    ra = 2 * oy, rb = 2 * oy + 1, ca = 2 * ox, cb = 2 * ox + 1;
  } else if (mode == 2) {
    const int *tx = taps + q[9], *ty = taps + q[10];
    ca = tx[ox], cb = tx[S + ox], a0 = tx[2 * S + ox], a1 = tx[3 * S + ox];
    ra = ty[oy], rb = ty[S + oy], b0 = ty[2 * S + oy], b1 = ty[3 * S + oy];
  }
  const bool keep_aa = !use_mask || m[ra * w + ca], keep_ab = !use_mask || m[ra * w + cb];
  const bool keep_ba = !use_mask || m[rb * w + ca], keep_bb = !use_mask || m[rb * w + cb];
  const uint8_t *paa = img + ((size_t)(y0 + ra) * W + x0 + ca) * C, *pab = img + ((size_t)(y0 + ra) * W + x0 + cb) * C;
  const uint8_t *pba = img + ((size_t)(y0 + rb) * W + x0 + ca) * C, *pbb = img + ((size_t)(y0 + rb) * W + x0 + cb) * C;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int ch = C == 1 ? 0 : (bgr ? C - 1 - k : k);
    const int vaa = keep_aa ? paa[ch] : 0;
    int v;
    if (mode == 0) {
      v = vaa;
    } else {
      const int vab = keep_ab ? pab[ch] : 0, vba = keep_ba ? pba[ch] : 0, vbb = keep_bb ? pbb[ch] : 0;
      if (mode == 1) {
        v = (vaa + vab + vba + vbb + 2) >> 2;
      } else {
        const int r0 = vaa * a0 + vab * a1, r1 = vba * a0 + vbb * a1;  // horizontal pass, x 2048
        v = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2;
        v = min(max(v, 0), 255);
      }
    }
    out[(((size_t)d * 3 + k) * S + oy) * S + ox] = lut[k * 256 + v];
  }
}

__global__ __launch_bounds__(256) void prep_compact_lift_kernel(const double *__restrict__ depth, int W, const int *__restrict__ desc,
                                                                const uint8_t *__restrict__ masks, const int *__restrict__ row_base,
                                                                double fx, double fy, double cx, double cy, int *__restrict__ pix,
                                                                double *__restrict__ cloud, double *__restrict__ row_sums) {
  const int d = blockIdx.y, lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int *q = desc + d * PREP_DESC;
  const int y0 = q[0], x0 = q[1], h = q[2], w = q[3], n = q[6], row_off = q[7];
  if (r >= h) return;  // whole wavefronts leave together: a row belongs to one wavefront
  const uint8_t *m = masks + q[4] + (size_t)r * w;
  const double *drow = depth + (size_t)(y0 + r) * W + x0;
  const double v = (double)(y0 + r) - cy;
  int base = row_base[row_off + r];  // set pixels of the rows above, inside this detection
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int c0 = 0; c0 < w; c0 += 64) {
    const int c = c0 + lane;
    const bool hit = c < w && m[c] != 0;
    const unsigned long long ballot = __ballot(hit);
    const int pre = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
    const int j = base + pre;
    if (hit && j < n) {
      const double z = drow[c], u = (double)(x0 + c) - cx;
      const double X = (u * z) / fx, Y = (v * z) / fy;
      const size_t g = (size_t)q[5] + j;
      pix[g] = r * w + c;
      cloud[3 * g + 0] = X, cloud[3 * g + 1] = Y, cloud[3 * g + 2] = z;
      sx += X, sy += Y, sz += z;
    }
    base += __popcll(ballot);
  }
  sx = wave_all_sum(sx), sy = wave_all_sum(sy), sz = wave_all_sum(sz);
  if (lane == 0) {
    double *o = row_sums + (size_t)(row_off + r) * 3;
    o[0] = sx, o[1] = sy, o[2] = sz;
  }
}

__global__ __launch_bounds__(256) void prep_distances_kernel(const int *__restrict__ desc, const double *__restrict__ cloud,
                                                             const double *__restrict__ row_sums, double *__restrict__ dist) {
  __shared__ double centre[3];
  const int d = blockIdx.y;
  const int *q = desc + d * PREP_DESC;
  const int h = q[2], n = q[6], row_off = q[7];
  const int first = blockIdx.x * PREP_DIST_PER_BLOCK;
  if (first >= n) return;
  if (threadIdx.x < 64) {  // every block of a detection adds the same values in the same order
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int r = threadIdx.x; r < h; r += 64) {
      const double *o = row_sums + (size_t)(row_off + r) * 3;
      sx += o[0], sy += o[1], sz += o[2];
    }
    sx = wave_all_sum(sx), sy = wave_all_sum(sy), sz = wave_all_sum(sz);
    if (threadIdx.x == 0) centre[0] = sx / (double)n, centre[1] = sy / (double)n, centre[2] = sz / (double)n;
  }
  __syncthreads();
  const double mx = centre[0], my = centre[1], mz = centre[2];
  for (int i = first + threadIdx.x; i < min(n, first + PREP_DIST_PER_BLOCK); i += 256) {
    const size_t g = (size_t)q[5] + i;
    const double dx = cloud[3 * g + 0] - mx, dy = cloud[3 * g + 1] - my, dz = cloud[3 * g + 2] - mz;
    dist[g] = sqrt(dx * dx + dy * dy + dz * dz);
  }
}

// sel[p] = (h, w) of the window of picked detection p; index[p][i] = position of its i-th drawn sample in the compacted arrays
__global__ __launch_bounds__(256) void prep_gather_kernel(const int *__restrict__ sel, const int *__restrict__ index, const int *__restrict__ pix,
                                                          const double *__restrict__ cloud, int n, int S, float *__restrict__ pts,
                                                          long *__restrict__ choose) {
  const int p = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int h = sel[2 * p], w = sel[2 * p + 1];
  const size_t o = (size_t)p * n + i, g = (size_t)index[o];
  pts[3 * o + 0] = (float)cloud[3 * g + 0];
  pts[3 * o + 1] = (float)cloud[3 * g + 1];
  pts[3 * o + 2] = (float)cloud[3 * g + 2];
  // Window.to_resized: rows and columns alike are decomposed with the window HEIGHT, scaled in float64, floored
  const int flat = pix[g], r = flat / h, c = flat - r * h;
  const double sr = (double)S / (double)w, sc = (double)S / (double)h;
  choose[o] = (long)(floor((double)r * sr) * (double)S + floor((double)c * sc));
}

}  // namespace unopose

using namespace unopose;

extern "C" {

int unopose_prep_desc_ints(void) { return PREP_DESC; }

int unopose_prep_crop_resize(const void *img, int H, int W, int C, const int *desc, const int *taps, const void *masks, const float *lut,
                             int D, int S, int bgr, int use_mask, float *out, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(img && desc && masks && lut && out, "prep_crop_resize: null pointer");
  UNOPOSE_REQUIRE(H >= 1 && W >= 1 && (C == 1 || C == 3 || C == 4) && D >= 1 && D <= 65535 && S >= 1 && S <= 4096,
                  "prep_crop_resize: bad sizes (H=%d W=%d C=%d D=%d S=%d)", H, W, C, D, S);
  hipLaunchKernelGGL(prep_crop_resize_kernel, dim3(cdiv((long)S * S, 256), D), dim3(256), 0, (hipStream_t)stream, (const uint8_t *)img, W, C,
                     desc, taps, (const uint8_t *)masks, lut, S, bgr, use_mask, out);
  return check_launch("prep_crop_resize");
}

int unopose_prep_compact_lift(const double *depth, int H, int W, const int *desc, const void *masks, const int *row_base, double fx,
                              double fy, double cx, double cy, int D, int max_h, int *pix, double *cloud, double *row_sums,
                              unopose_stream_t stream) {
  UNOPOSE_REQUIRE(depth && desc && masks && row_base && pix && cloud && row_sums, "prep_compact_lift: null pointer");
  UNOPOSE_REQUIRE(H >= 1 && W >= 1 && D >= 1 && D <= 65535 && max_h >= 1 && max_h <= H, "prep_compact_lift: bad sizes (H=%d W=%d D=%d max_h=%d)",
                  H, W, D, max_h);
  hipLaunchKernelGGL(prep_compact_lift_kernel, dim3(cdiv(max_h, 4), D), dim3(256), 0, (hipStream_t)stream, depth, W, desc,
                     (const uint8_t *)masks, row_base, fx, fy, cx, cy, pix, cloud, row_sums);
  return check_launch("prep_compact_lift");
}

int unopose_prep_distances(const int *desc, const double *cloud, const double *row_sums, int D, int max_n, double *dist,
                           unopose_stream_t stream) {
  UNOPOSE_REQUIRE(desc && cloud && row_sums && dist, "prep_distances: null pointer");
  UNOPOSE_REQUIRE(D >= 1 && D <= 65535 && max_n >= 1, "prep_distances: bad sizes (D=%d max_n=%d)", D, max_n);
  hipLaunchKernelGGL(prep_distances_kernel, dim3(cdiv(max_n, PREP_DIST_PER_BLOCK), D), dim3(256), 0, (hipStream_t)stream, desc, cloud,
                     row_sums, dist);
  return check_launch("prep_distances");
}

int unopose_prep_gather(const int *sel, const int *index, const int *pix, const double *cloud, int P, int n, int S, float *pts, void *choose,
                        unopose_stream_t stream) {
  UNOPOSE_REQUIRE(sel && index && pix && cloud && pts && choose, "prep_gather: null pointer");
  UNOPOSE_REQUIRE(P >= 1 && P <= 65535 && n >= 1 && S >= 1, "prep_gather: bad sizes (P=%d n=%d S=%d)", P, n, S);
  hipLaunchKernelGGL(prep_gather_kernel, dim3(cdiv(n, 256), P), dim3(256), 0, (hipStream_t)stream, sel, index, pix, cloud, n, S, pts,
                     (long *)choose);
  return check_launch("prep_gather");
}

}  // extern "C"
