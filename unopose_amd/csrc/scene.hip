// The scene stage of the online training pairs (unopose_amd/provider_online.py, module docstring part 4): a textured background plane
// behind a query and a depth-sensor model (holes per cell, drop-outs at depth edges, axial noise, disparity quantisation) on rendered
// canvases, for all views of a call in one launch.  `provider_online.sense_views_host` is the specification and the results are held to
// equality with it in every depth bit and colour byte: all arithmetic is scalar float64 with + - x / floor rint and comparisons only, every
// expression keeps the specification's evaluation order (the build's -ffp-contract=off keeps them as written), and every random number is
// scene_hash(key, stream, index), a pure function.  Every stage reads the INPUT canvas only -- a pixel works out the noise-free depth of
// its four neighbours itself -- so no thread waits for another: no LDS, no barrier, no atomics.
//
// View descriptor, SCENE_DESC 64-bit words per view (provider_online.scene_rows; ops/items.py range-checks them): 0 view key, 1 texture key,
// 2 plane (0 / 1), 3 hole threshold, 4 edge-drop threshold (a hash's upper 32 bits below the threshold = the event), 5 hole cell in pixels,
// 6 disparity steps (0 = no quantisation), 7 unused; float64 from here: 8 9 10 the noise's a, b, z0 (sigma = a + b (z - z0)^2, metres),
// 11 focal x baseline, 12 edge threshold, 13-15 the plane's unit normal n, 16 n . p0, 17-19 p0 (metres), 20-22 and 23-25 the in-plane axes
// u, v, 26 texture cell (metres), 27 z_max, 28 29 30 the camera's f, cx, cy, 31 unused.
#include "common.h"
#include "item_mix.h"

namespace unopose {

constexpr int SCENE_DESC = 32;
constexpr unsigned SCENE_STREAM_HOLE = 0, SCENE_STREAM_EDGE = 1, SCENE_STREAM_NOISE = 2, SCENE_STREAM_TEXTURE = 3;
constexpr double SCENE_DEPTH_TO_M = 0.001;
constexpr double SCENE_G_SCALE = 1.7320508075688772 / 65536.0;  // sqrt(3) / 2^16

// provider_online._scene_hash; index < 2^40
__device__ __forceinline__ unsigned long long scene_hash(unsigned long long key, unsigned stream, unsigned long long index) {
  return item_mix(key ^ item_mix((index | ((unsigned long long)stream << 40)) + ITEM_GOLD));
}

// stage (a): the noise-free depth in metres of input pixel (x, y): the render's where it has one, else the background plane's where the
// view has a plane that faces the camera there within (0, z_max], else 0
__device__ __forceinline__ double scene_depth(const float *__restrict__ depth, int W, int x, int y, bool plane, const double *__restrict__ fl,
                                              bool &background) {
  const float raw = depth[(size_t)y * W + x];
  background = false;
  if (raw > 0.f) return (double)raw * SCENE_DEPTH_TO_M;
  if (!plane) return 0.0;
  const double rx = ((double)x - fl[29]) / fl[28], ry = ((double)y - fl[30]) / fl[28];
  const double nr = (fl[13] * rx + fl[14] * ry) + fl[15];
  if (!(nr < 0.0)) return 0.0;
  const double z = fl[16] / nr;
  if (!(z > 0.0 && z <= fl[27])) return 0.0;
  background = true;
  return z;
}

// provider_online._scene_texture: three octaves of value noise at plane coordinates (s, t)
__device__ __forceinline__ void scene_texture(unsigned long long tex_key, double s, double t, uint8_t *__restrict__ out) {
  const double weight[3] = {0.5, 0.3, 0.2};
  double total[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int o = 0; o < 3; ++o) {
    const double so = s * (double)(1 << o), to = t * (double)(1 << o);
    const double su = floor(so), sv = floor(to), fu = so - su, fv = to - sv;
    const long long iu = (long long)su, iv = (long long)sv;  // the host bounds |so|, |to| below 2^19
    unsigned long long h[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      h[j] = scene_hash(tex_key, SCENE_STREAM_TEXTURE + o,
                        ((unsigned long long)((iu + (j & 1)) & 0xFFFFF) << 20) | (unsigned long long)((iv + (j >> 1)) & 0xFFFFF));
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double b00 = (double)((h[0] >> (8 * c)) & 255), b10 = (double)((h[1] >> (8 * c)) & 255);
      const double b01 = (double)((h[2] >> (8 * c)) & 255), b11 = (double)((h[3] >> (8 * c)) & 255);
      const double top = b00 + (b10 - b00) * fu, bottom = b01 + (b11 - b01) * fu;
      const double value = (top + (bottom - top) * fv) * weight[o];
      total[c] = o == 0 ? value : total[c] + value;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) out[c] = (uint8_t)floor(total[c] + 0.5);
}

// one wavefront per image row, 64 pixels at a time
__global__ __launch_bounds__(256) void scene_sense_kernel(const float *__restrict__ depth, const uint8_t *__restrict__ rgb,
                                                          const unsigned long long *__restrict__ desc, int H, int W,
                                                          float *__restrict__ out_depth, uint8_t *__restrict__ out_rgb) {
  const int v = blockIdx.y, lane = threadIdx.x & 63, y = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (y >= H) return;
  const size_t plane_px = (size_t)H * W;
  const float *dv = depth + (size_t)v * plane_px;
  const unsigned long long *w = desc + (size_t)v * SCENE_DESC;
  const double *fl = reinterpret_cast<const double *>(w);
  const unsigned long long key = w[0], tex_key = w[1], hole_thr = w[3], edge_thr = w[4];
  const bool plane = w[2] != 0;
  const int hole_cell = (int)w[5], steps = (int)w[6], cells_x = (W + hole_cell - 1) / hole_cell;
  const double a = fl[8], b = fl[9], z0 = fl[10], fb = fl[11], edge_thres = fl[12];
  const bool sensor = a != 0.0 || b != 0.0 || steps != 0;
  for (int x = lane; x < W; x += 64) {
    const size_t at = (size_t)y * W + x;
    const unsigned long long pix = (unsigned long long)at;
    bool background;
    const double z = scene_depth(dv, W, x, y, plane, fl, background);
    uint8_t colour[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) colour[c] = rgb[((size_t)v * plane_px + at) * 3 + c];
    float out = dv[at];
    if (background) {
      const double rx = ((double)x - fl[29]) / fl[28], ry = ((double)y - fl[30]) / fl[28];
      const double dx = rx * z - fl[17], dy = ry * z - fl[18], dz = z - fl[19];
      const double s = ((dx * fl[20] + dy * fl[21]) + dz * fl[22]) / fl[26];
      const double t = ((dx * fl[23] + dy * fl[24]) + dz * fl[25]) / fl[26];
      scene_texture(tex_key, s, t, colour);
    }
    if (z > 0.0) {
      // (b) drop-outs on the noise-free depth
      const unsigned long long cell = (unsigned long long)((y / hole_cell) * cells_x + x / hole_cell);
      bool dropped = (scene_hash(key, SCENE_STREAM_HOLE, cell) >> 32) < hole_thr;
      if (!dropped && edge_thr != 0) {
        bool edge = false, unused;
        if (y > 0) {
          const double zn = scene_depth(dv, W, x, y - 1, plane, fl, unused);
          edge = edge || !(zn > 0.0) || fabs(z - zn) > edge_thres * z;
        }
        if (y + 1 < H) {
          const double zn = scene_depth(dv, W, x, y + 1, plane, fl, unused);
          edge = edge || !(zn > 0.0) || fabs(z - zn) > edge_thres * z;
        }
        if (x > 0) {
          const double zn = scene_depth(dv, W, x - 1, y, plane, fl, unused);
          edge = edge || !(zn > 0.0) || fabs(z - zn) > edge_thres * z;
        }
        if (x + 1 < W) {
          const double zn = scene_depth(dv, W, x + 1, y, plane, fl, unused);
          edge = edge || !(zn > 0.0) || fabs(z - zn) > edge_thres * z;
        }
        dropped = edge && (scene_hash(key, SCENE_STREAM_EDGE, pix) >> 32) < edge_thr;
      }
      if (dropped) {
        out = 0.f;
      } else if (sensor) {
        // (c) axial noise, then disparity quantisation
        const unsigned long long h = scene_hash(key, SCENE_STREAM_NOISE, pix);
        const long long fields = (long long)(h & 0xFFFF) + (long long)((h >> 16) & 0xFFFF) + (long long)((h >> 32) & 0xFFFF) + (long long)(h >> 48);
        const double g = (double)(fields - 131070) * SCENE_G_SCALE;
        double zs = z + (a + b * ((z - z0) * (z - z0))) * g;
        bool ok = zs > 0.0;
        if (ok && steps != 0) {
          const double k = rint(((double)steps * fb) / zs);
          ok = k >= 1.0;
          if (ok) zs = fb / (k / (double)steps);
        }
        out = ok ? (float)(zs * 1000.0) : 0.f;
      } else if (background) {
        out = (float)(z * 1000.0);
      }
    }
    out_depth[(size_t)v * plane_px + at] = out;
#pragma unroll
    for (int c = 0; c < 3; ++c) out_rgb[((size_t)v * plane_px + at) * 3 + c] = colour[c];
  }
}

}  // namespace unopose

using namespace unopose;

extern "C" {

int unopose_scene_desc_words(void) { return SCENE_DESC; }

int unopose_scene_sense(const float *depth, const void *rgb, const void *desc, int V, int H, int W, float *out_depth, void *out_rgb,
                        unopose_stream_t stream) {
  UNOPOSE_REQUIRE(depth && rgb && desc && out_depth && out_rgb, "scene_sense: null pointer");
  UNOPOSE_REQUIRE(depth != out_depth && rgb != out_rgb, "scene_sense: in place (a pixel reads its neighbours' input)");
  UNOPOSE_REQUIRE(V >= 1 && V <= 65535 && H >= 1 && W >= 1 && (long)H * W < (1l << 31), "scene_sense: bad sizes (V=%d H=%d W=%d)", V, H, W);
  hipLaunchKernelGGL(scene_sense_kernel, dim3(cdiv(H, 4), V), dim3(256), 0, (hipStream_t)stream, depth, (const uint8_t *)rgb,
                     (const unsigned long long *)desc, H, W, out_depth, (uint8_t *)out_rgb);
  return check_launch("scene_sense");
}

}  // extern "C"
