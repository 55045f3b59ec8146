// The training provider's colour augmentation (unopose_amd/provider_train.py: ColorAugmentor) on the device, for all crops of a batch at
// once.  ColorAugmentor.apply is the specification and the results are held to equality with it, so every expression below keeps its
// evaluation order (the build's -ffp-contract=off keeps the fp32 ones as written; integer parts are Pillow's fixed-point formulas).
//
// Layout: the crops sit one under the other in a uint8 HWC atlas (H rows, W pixels per row, 3 channels), crop c on rows y0 .. y0 + h - 1,
// columns 0 .. w - 1; the columns right of w are padding that no kernel reads or writes.  A crop's chain is a run of CAUG_ENTRY-word
// entries in the `ops` table; one launch of coloraug_step executes chain position `pos` of every crop from `src` into `dst` (a crop
// whose chain has ended is copied through), the host alternates two atlases.  Two operators need more than that launch:
//   * contrast blends with the mean luma: coloraug_luma_sum adds the crop's L values into a 64-bit slot first (integer atomics: the sum
//     does not depend on the order);
//   * the Gaussian blur is three box passes along the rows, then three along the columns: coloraug_blur_lines keeps CAUG_LINES lines
//     (8 rows or 8 columns x 3 channels) in LDS for the three passes.  The row launch goes src -> dst, the column launch works in place
//     on dst: a workgroup owns its columns, reads them whole and writes only them.
//
// Descriptor of crop c, CAUG_DESC int32 (built and range-checked on the host, ops/augment.py):
//   0 y0   1 h   2 w   3 chain length   4 first entry in `ops`   5 start of its drop grids in `grids` (bytes)
//   6 start of its noise fields in `noise` (floats)   7 unused
// Entry, CAUG_ENTRY int32 words (floats as their bits): 0 opcode, then
//   coarse_dropout  ch, cw, offset of the ch x cw grid (1 = drop) behind the crop's grid start
//   gaussian_blur   r, ww, fw (Pillow's box radius and 8.24 weights, computed on the host)
//   sharpness / brightness / color / grayscale   factor
//   contrast        factor, slot of its luma sum
//   add / multiply_pc / multiply / linear_contrast   three per-channel values;   invert   three flags (float, non-zero = flip)
//   gaussian_noise  offset of the h x w x 3 field behind the crop's noise start
#include "common.h"

namespace unopose {

constexpr int CAUG_DESC = 8;
constexpr int CAUG_ENTRY = 4;
constexpr int CAUG_LINES = 24;       // lines per workgroup of the blur: 8 pixels x 3 channels
constexpr int CAUG_MAX_LINE = 1360;  // longest line the blur keeps in LDS: 2 x 24 x 1360 bytes < 64 KiB

enum {
  CAUG_COARSE_DROPOUT = 0, CAUG_GAUSSIAN_BLUR, CAUG_SHARPNESS, CAUG_CONTRAST, CAUG_BRIGHTNESS, CAUG_COLOR, CAUG_ADD, CAUG_INVERT,
  CAUG_MULTIPLY_PC, CAUG_MULTIPLY, CAUG_GAUSSIAN_NOISE, CAUG_LINEAR_CONTRAST, CAUG_GRAYSCALE, CAUG_N_OPS
};

__device__ __forceinline__ int caug_luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// np.clip(np.rint(x), 0, 255): rintf rounds halves to even
__device__ __forceinline__ uint8_t caug_u8(float x) { return (uint8_t)(int)fminf(fmaxf(rintf(x), 0.f), 255.f); }

// Image.blend(deg, img, f): truncation; clamped first when f is outside [0, 1]
__device__ __forceinline__ uint8_t caug_blend(float deg, float v, float f, bool inside) {
  float t = deg + f * (v - deg);
  if (!inside) t = fminf(fmaxf(t, 0.f), 255.f);
  return (uint8_t)(int)t;
}

// ImageFilter.SMOOTH at an interior pixel: clamp(floor(0.5 + sum p k)), the nine products added in row-major order
__device__ __forceinline__ float caug_smooth(const uint8_t *p, size_t pitch) {
  const float k1 = 1.0f / 13.0f, k5 = 5.0f / 13.0f;
  float s = 0.5f;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx)
      s = s + (float)p[(ptrdiff_t)dy * (ptrdiff_t)pitch + dx * 3] * ((dy == 0 && dx == 0) ? k5 : k1);
  return fminf(fmaxf(floorf(s), 0.f), 255.f);
}

__global__ __launch_bounds__(256) void coloraug_luma_sum_kernel(const uint8_t *__restrict__ src, int W, const int *__restrict__ desc,
                                                                const int *__restrict__ ops, int pos, unsigned long long *__restrict__ sums) {
  const int *q = desc + blockIdx.y * CAUG_DESC;
  const int h = q[1], w = q[2];
  if (pos >= q[3] || blockIdx.x * 256 >= h * w) return;  // uniform over the workgroup
  const int *e = ops + (size_t)(q[4] + pos) * CAUG_ENTRY;
  if (e[0] != CAUG_CONTRAST) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  unsigned v = 0;
  if (i < h * w) {
    const int y = i / w, x = i - y * w;
    const uint8_t *p = src + ((size_t)(q[0] + y) * W + x) * 3;
    v = (unsigned)caug_luma(p[0], p[1], p[2]);
  }
  v = wave_all_sum(v);
  if ((threadIdx.x & 63) == 0) atomicAdd(sums + e[2], (unsigned long long)v);
}

__global__ __launch_bounds__(256) void coloraug_step_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, int W,
                                                            const int *__restrict__ desc, const int *__restrict__ ops,
                                                            const uint8_t *__restrict__ grids, const float *__restrict__ noise,
                                                            const unsigned long long *__restrict__ sums, int pos) {
  const int *q = desc + blockIdx.y * CAUG_DESC;
  const int h = q[1], w = q[2];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= h * w) return;
  const int y = i / w, x = i - y * w;
  const size_t pitch = (size_t)W * 3, at = (size_t)(q[0] + y) * pitch + (size_t)x * 3;
  const uint8_t *p = src + at;
  uint8_t *o = dst + at;
  const int v0 = p[0], v1 = p[1], v2 = p[2];
  if (pos >= q[3]) {  // the chain has ended: copy through
    o[0] = (uint8_t)v0, o[1] = (uint8_t)v1, o[2] = (uint8_t)v2;
    return;
  }
  const int *e = ops + (size_t)(q[4] + pos) * CAUG_ENTRY;
  const int op = e[0];
  const float f1 = __int_as_float(e[1]), f2 = __int_as_float(e[2]), f3 = __int_as_float(e[3]);
  const float x0 = (float)v0, x1 = (float)v1, x2 = (float)v2;
  switch (op) {
    case CAUG_COARSE_DROPOUT: {
      const int ch = e[1], cw = e[2];
      const int gy = min((y * ch) / h, ch - 1), gx = min((x * cw) / w, cw - 1);
      const bool drop = grids[(size_t)q[5] + e[3] + gy * cw + gx] != 0;
      o[0] = drop ? 0 : (uint8_t)v0, o[1] = drop ? 0 : (uint8_t)v1, o[2] = drop ? 0 : (uint8_t)v2;
      break;
    }
    case CAUG_GAUSSIAN_BLUR:  // coloraug_blur_lines writes this crop
      break;
    case CAUG_SHARPNESS: {
      const bool in01 = f1 >= 0.f && f1 <= 1.f;
      if (y == 0 || x == 0 || y == h - 1 || x == w - 1) {  // SMOOTH copies the border ring: deg = img
        o[0] = caug_blend(x0, x0, f1, in01), o[1] = caug_blend(x1, x1, f1, in01), o[2] = caug_blend(x2, x2, f1, in01);
      } else {
        o[0] = caug_blend(caug_smooth(p + 0, pitch), x0, f1, in01);
        o[1] = caug_blend(caug_smooth(p + 1, pitch), x1, f1, in01);
        o[2] = caug_blend(caug_smooth(p + 2, pitch), x2, f1, in01);
      }
      break;
    }
    case CAUG_CONTRAST: {
      const unsigned long long n = (unsigned long long)h * (unsigned long long)w;
      const float m = (float)(int)((2ull * sums[e[2]] + n) / (2ull * n));
      const bool in01 = f1 >= 0.f && f1 <= 1.f;
      o[0] = caug_blend(m, x0, f1, in01), o[1] = caug_blend(m, x1, f1, in01), o[2] = caug_blend(m, x2, f1, in01);
      break;
    }
    case CAUG_BRIGHTNESS: {
      const bool in01 = f1 >= 0.f && f1 <= 1.f;
      o[0] = caug_blend(0.f, x0, f1, in01), o[1] = caug_blend(0.f, x1, f1, in01), o[2] = caug_blend(0.f, x2, f1, in01);
      break;
    }
    case CAUG_COLOR: {
      const bool in01 = f1 >= 0.f && f1 <= 1.f;
      const float l = (float)caug_luma(v0, v1, v2);
      o[0] = caug_blend(l, x0, f1, in01), o[1] = caug_blend(l, x1, f1, in01), o[2] = caug_blend(l, x2, f1, in01);
      break;
    }
    case CAUG_ADD:
      o[0] = caug_u8(x0 + f1), o[1] = caug_u8(x1 + f2), o[2] = caug_u8(x2 + f3);
      break;
    case CAUG_INVERT:
      o[0] = (uint8_t)(f1 != 0.f ? 255 - v0 : v0), o[1] = (uint8_t)(f2 != 0.f ? 255 - v1 : v1), o[2] = (uint8_t)(f3 != 0.f ? 255 - v2 : v2);
      break;
    case CAUG_MULTIPLY_PC:
    case CAUG_MULTIPLY:
      o[0] = caug_u8(x0 * f1), o[1] = caug_u8(x1 * f2), o[2] = caug_u8(x2 * f3);
      break;
    case CAUG_GAUSSIAN_NOISE: {
      const float *nz = noise + (size_t)q[6] + (size_t)e[1] + (size_t)i * 3;
      o[0] = caug_u8(x0 + nz[0]), o[1] = caug_u8(x1 + nz[1]), o[2] = caug_u8(x2 + nz[2]);
      break;
    }
    case CAUG_LINEAR_CONTRAST:
      o[0] = caug_u8(128.0f + f1 * (x0 - 128.0f)), o[1] = caug_u8(128.0f + f2 * (x1 - 128.0f)), o[2] = caug_u8(128.0f + f3 * (x2 - 128.0f));
      break;
    case CAUG_GRAYSCALE: {
      const float g = (x0 * 0.299f + x1 * 0.587f) + x2 * 0.114f, keep = 1.0f - f1;
      o[0] = caug_u8(keep * x0 + f1 * g), o[1] = caug_u8(keep * x1 + f1 * g), o[2] = caug_u8(keep * x2 + f1 * g);
      break;
    }
    default:  // the host admits no other opcode
      break;
  }
}

// axis 0: lines = the rows of a crop (one per channel), element stride 3 bytes; a workgroup takes 8 rows.
// axis 1: lines = its columns, element stride one atlas row; a workgroup takes 8 columns.  Either way line j of the workgroup is pixel
// j / 3 of its 8, channel j % 3, and the workgroup's bytes at element t are the 24 consecutive bytes of 8 pixels (axis 1) or 3 of each row.
__global__ __launch_bounds__(256) void coloraug_blur_lines_kernel(const uint8_t *src, uint8_t *dst, int W,  // (src == dst on axis 1)
                                                                  const int *__restrict__ desc, const int *__restrict__ ops, int pos,
                                                                  int axis, int stride) {
  extern __shared__ uint8_t lds[];  // 2 buffers x CAUG_LINES x stride
  const int *q = desc + blockIdx.y * CAUG_DESC;
  if (pos >= q[3]) return;
  const int *e = ops + (size_t)(q[4] + pos) * CAUG_ENTRY;
  if (e[0] != CAUG_GAUSSIAN_BLUR) return;
  const int h = q[1], w = q[2];
  const int len = axis == 0 ? w : h, across = axis == 0 ? h : w;  // elements per line; pixels across the lines
  const int first = blockIdx.x * 8;
  if (first >= across) return;  // (uniform: no barrier has been reached)
  const int npix = min(8, across - first), nlines = npix * 3;
  const int r = e[1];
  const uint32_t ww = (uint32_t)e[2], fw = (uint32_t)e[3];
  const size_t pitch = (size_t)W * 3, base = (size_t)q[0] * pitch;
  uint8_t *a = lds, *b = lds + CAUG_LINES * stride;
  // element t of line j: axis 0 -> row first + j / 3, column t, channel j % 3; axis 1 -> row t, column first + j / 3, channel j % 3
  for (int k = threadIdx.x; k < nlines * len; k += 256) {
    int j, t;
    size_t g;
    if (axis == 0) {
      const int row = k / (len * 3), rest = k - row * (len * 3);  // rest = t * 3 + channel: the row's bytes in memory order
      t = rest / 3, j = row * 3 + (rest - t * 3);
      g = base + (size_t)(first + row) * pitch + rest;
    } else {
      t = k / nlines, j = k - t * nlines;  // j = pixel * 3 + channel: consecutive bytes of row t
      g = base + (size_t)t * pitch + (size_t)first * 3 + j;
    }
    a[j * stride + t] = src[g];
  }
  __syncthreads();
  for (int pass = 0; pass < 3; ++pass) {
    for (int k = threadIdx.x; k < nlines * len; k += 256) {
      const int j = k / len, t = k - j * len;
      const uint8_t *line = a + j * stride;
      uint32_t acc = 0;
      for (int d = -r; d <= r; ++d) acc += line[min(max(t + d, 0), len - 1)];
      const uint32_t far = (uint32_t)line[max(t - r - 1, 0)] + (uint32_t)line[min(t + r + 1, len - 1)];
      b[j * stride + t] = (uint8_t)((acc * ww + far * fw + (1u << 23)) >> 24);
    }
    __syncthreads();
    uint8_t *s = a;
    a = b, b = s;
  }
  for (int k = threadIdx.x; k < nlines * len; k += 256) {
    int j, t;
    size_t g;
    if (axis == 0) {
      const int row = k / (len * 3), rest = k - row * (len * 3);
      t = rest / 3, j = row * 3 + (rest - t * 3);
      g = base + (size_t)(first + row) * pitch + rest;
    } else {
      t = k / nlines, j = k - t * nlines;
      g = base + (size_t)t * pitch + (size_t)first * 3 + j;
    }
    dst[g] = a[j * stride + t];
  }
}

}  // namespace unopose

using namespace unopose;

extern "C" {

int unopose_coloraug_ints(int what) {
  switch (what) {
    case 0: return CAUG_DESC;
    case 1: return CAUG_ENTRY;
    case 2: return CAUG_MAX_LINE;
    case 3: return CAUG_N_OPS;
    default: return -1;
  }
}

int unopose_coloraug_luma_sum(const void *src, int H, int W, const int *desc, const int *ops, int n_crops, int max_pixels, int pos, void *sums,
                              unopose_stream_t stream) {
  UNOPOSE_REQUIRE(src && desc && ops && sums, "coloraug_luma_sum: null pointer");
  UNOPOSE_REQUIRE(H >= 1 && W >= 1 && n_crops >= 1 && n_crops <= 65535 && max_pixels >= 1 && pos >= 0,
                  "coloraug_luma_sum: bad sizes (H=%d W=%d crops=%d max_pixels=%d pos=%d)", H, W, n_crops, max_pixels, pos);
  hipLaunchKernelGGL(coloraug_luma_sum_kernel, dim3(cdiv(max_pixels, 256), n_crops), dim3(256), 0, (hipStream_t)stream, (const uint8_t *)src, W,
                     desc, ops, pos, (unsigned long long *)sums);
  return check_launch("coloraug_luma_sum");
}

int unopose_coloraug_step(const void *src, void *dst, int H, int W, const int *desc, const int *ops, const void *grids, const float *noise,
                          const void *sums, int n_crops, int max_pixels, int pos, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(src && dst && src != dst && desc && ops && grids && noise && sums, "coloraug_step: null pointer or src == dst");
  UNOPOSE_REQUIRE(H >= 1 && W >= 1 && n_crops >= 1 && n_crops <= 65535 && max_pixels >= 1 && pos >= 0,
                  "coloraug_step: bad sizes (H=%d W=%d crops=%d max_pixels=%d pos=%d)", H, W, n_crops, max_pixels, pos);
  hipLaunchKernelGGL(coloraug_step_kernel, dim3(cdiv(max_pixels, 256), n_crops), dim3(256), 0, (hipStream_t)stream, (const uint8_t *)src,
                     (uint8_t *)dst, W, desc, ops, (const uint8_t *)grids, noise, (const unsigned long long *)sums, pos);
  return check_launch("coloraug_step");
}

int unopose_coloraug_blur_lines(const void *src, void *dst, int H, int W, const int *desc, const int *ops, int n_crops, int max_across,
                                int max_line, int pos, int axis, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(src && dst && desc && ops, "coloraug_blur_lines: null pointer");
  UNOPOSE_REQUIRE((axis == 0 && src != dst) || (axis == 1 && src == dst), "coloraug_blur_lines: rows go from src to dst, columns run in place");
  UNOPOSE_REQUIRE(H >= 1 && W >= 1 && n_crops >= 1 && n_crops <= 65535 && max_across >= 1 && max_line >= 1 && max_line <= CAUG_MAX_LINE && pos >= 0,
                  "coloraug_blur_lines: bad sizes (H=%d W=%d crops=%d max_across=%d max_line=%d pos=%d)", H, W, n_crops, max_across, max_line, pos);
  const int stride = (max_line + 3) & ~3;
  hipLaunchKernelGGL(coloraug_blur_lines_kernel, dim3(cdiv(max_across, 8), n_crops), dim3(256), (size_t)2 * CAUG_LINES * stride,
                     (hipStream_t)stream, (const uint8_t *)src, (uint8_t *)dst, W, desc, ops, pos, axis, stride);
  return check_launch("coloraug_blur_lines");
}

}  // extern "C"
