// The small trainable nn.Linear layers of the matcher under autograd (rows < 16384, N and K multiples of 64 up to 512): y = act(x W^T + b),
// dX = (g . [y > 0]) W, dW = (g . [y > 0])^T x and db = sum_rows (g . [y > 0]) straight from the fp32 tensors as stored -- x (rows, K),
// W (N, K), g and y (rows, N), all row-major.  No derived copy of a weight or an activation exists outside a kernel, so nothing can go stale.
//
// y and dX (`small_linear_fwd_kernel`, `small_linear_dx_kernel`: one body): fp32-class products on the bf16 matrix cores (common.h: hi / lo split, three 16x16x32 MFMAs per product,
// fp32 accumulation); the split happens on the way into registers (the activation operand) and into LDS (the weight operand).  A workgroup
// of four waves owns a 64 x 64 tile of the output and walks the contraction 64 elements (two MFMA k-blocks) at a time:
//   * the activation rows (x, or g masked by y > 0) are contiguous along the contraction in both products, so every wave loads the fragment of
//     its 16 rows itself: lane l holds row (l & 15), contraction elements 8 (l >> 4) .. + 7 -- two 16-byte loads, rows past `rows` count as 0;
//   * the 64 x 64 weight block is split ONCE per workgroup and parked in LDS as ready fragments [8-element group h][output column] of 16 bytes
//     (hi and lo).  Forward: W (N, K) is contiguous along the contraction K, a thread loads 8 consecutive k of one row n.  dX: the contraction
//     runs over N, a thread takes one column k and walks 8 rows n (the 64 lanes of a wave read 256 consecutive bytes per row): the
//     transposition costs nothing and no W^T is ever written.
// The weight fragment is the MFMA's A operand and the activation fragment its B operand, i.e. the wave computes the TRANSPOSE of its
// 16-row strip: a lane's four accumulator registers are then four consecutive output columns of one row (one 16-byte store; bias as one
// 16-byte load).  LDS is double-buffered, one barrier per step; two register sets hold steps s and s + 1, and the loads of step s + 2 are
// issued as soon as step s is split: at K = 256 half the operands are in flight before the first MFMA (the kernels are latency bound:
// one or two workgroups per CU).
//
// dW and db (`small_wgrad_kernel` + `small_wgrad_combine_kernel`): EXACT fp32 products and fp32 accumulation on v_mfma_f32_32x32x2_f32, as
// csrc/conv_train.hip::linear_wgrad_f32_kernel: the reduction runs along the rows and both operands have their lanes along contiguous
// memory as they are.  A workgroup owns a 64 x 64 tile of dW over one slice of the rows (a wave 32 x 32 of it); the waves that own the
// tile's k-column 0 also sum their masked g values: db of the slice.  Rows go 32 at a time through two register sets (the next trip's
// loads under this trip's matrix instructions), every load predicated on its row.  The number of slices and their bounds depend on (rows, N, K) alone
// (`small_slices`), each slice writes its own partial, and the combine kernel adds the partials in double in slice order: no atomics, two
// calls give the same bits.  When both the input and the parameters ask for a gradient, `small_backward_kernel` runs the dX tiles and the
// weight-gradient slices in one launch (the same two bodies, chosen by workgroup index): forward, backward, combine = three launches a layer.
#include "common.h"

namespace unopose {

namespace {

constexpr int SL_MAX_ROWS = 16383;

__device__ __forceinline__ void load8(const float *p, float (&v)[8]) {
  const float4 a = *reinterpret_cast<const float4 *>(p), b = *reinterpret_cast<const float4 *>(p + 4);
  v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
}

union frag_u {
  bf16x8 v;
  uint4 q;
};

// DX = false: out (rows, NO = N) = act(a (rows, C = K) w^T + bias), w (N, K).
// DX = true:  out (rows, NO = K) = (a . [mask > 0]) (rows, C = N) w, w (N, K); mask may be null.
// One step = 64 elements of the contraction (two MFMA k-blocks of 32).
// The loads of one 32-element block of a step: the 8 activation values (and mask values) of this lane's row, the 8 weight values of this
// thread's share.  Nothing here waits for a load (the mask is applied in `small_park`), so two steps stay in flight.
template <bool DX>
__device__ __forceinline__ void small_fetch(const float *ap, const float *mp, const float *wp, bool masked, int NO, float (&av)[8], float (&mv)[8],
                                            float (&wv)[8]) {
  load8(ap, av);  // (a row past `rows` reads row 0 and is zeroed in `small_park`: no branch around the loads)
  if (masked) load8(mp, mv);
  if (DX) {
#pragma unroll
    for (int j = 0; j < 8; ++j) wv[j] = wp[(size_t)j * NO];
  } else {
    load8(wp, wv);
  }
}
// Mask and split the activation block -> its fragment; split the weight block and park it in LDS (hi at `dst`, lo 512 slots on).
__device__ __forceinline__ bf16x8_hl small_park(float (&av)[8], const float (&mv)[8], const float (&wv)[8], bool row_ok, bool masked, uint4 *dst) {
  if (masked) {
#pragma unroll
    for (int j = 0; j < 8; ++j) av[j] = mv[j] > 0.f ? av[j] : 0.f;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) av[j] = row_ok ? av[j] : 0.f;
  const bf16x8_hl wf = split8_bf16(wv);
  frag_u hi, lo;
  hi.v = wf.hi, lo.v = wf.lo;
  dst[0] = hi.q;
  dst[512] = lo.q;
  return split8_bf16(av);
}

template <bool DX>
__device__ __forceinline__ void small_linear_body(const float *__restrict__ a, const float *__restrict__ mask, const float *__restrict__ w,
                                                  const float *__restrict__ bias, int rows, int NO, int C, int relu, float *__restrict__ out, int bx, int by) {
  __shared__ uint4 sB[2][2][8][64];  // [stage][hi / lo][8-element group of the step's 64][output column]
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int col0 = bx * 64, row0 = by * 64;
  const int r = row0 + wave * 16 + (lane & 15), h = lane >> 4;
  const bool row_ok = r < rows;
  const bool masked = DX && mask != nullptr;
  const float *ap = a + (size_t)(row_ok ? r : 0) * C + 8 * h;
  const float *mp = masked ? mask + (size_t)(row_ok ? r : 0) * C + 8 * h : nullptr;
  // this thread's share of the weight block of a step: groups sh and sh + 4 of column sc
  const int sc = DX ? (t & 63) : (t >> 2), sh = DX ? (t >> 6) : (t & 3);
  const float *wp = DX ? w + (size_t)(8 * sh) * NO + col0 + sc : w + (size_t)(col0 + sc) * C + 8 * sh;
  const size_t wblock = DX ? (size_t)32 * NO : 32;  // 32 elements further along the contraction

  f32x4 acc[4];
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) acc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};

  // two register sets (steps s and s + 1), two 32-element blocks each
  float a00[8], a01[8], m00[8], m01[8], w00[8], w01[8], a10[8], a11[8], m10[8], m11[8], w10[8], w11[8];
#define SMALL_FETCH(S, A0, A1, M0, M1, W0, W1)                                                                           \
  do {                                                                                                                   \
    small_fetch<DX>(ap + 64 * (S), mp + 64 * (S), wp + wblock * (2 * (S)), masked, NO, A0, M0, W0);                     \
    small_fetch<DX>(ap + 64 * (S) + 32, mp + 64 * (S) + 32, wp + wblock * (2 * (S) + 1), masked, NO, A1, M1, W1); \
  } while (0)
  // split the step held in a register set, park its weight fragments, refill the set with step S + 2 (if any), then the products
#define SMALL_CONSUME(S, A0, A1, M0, M1, W0, W1)                                              \
  do {                                                                                        \
    const int st = (S) & 1;                                                                   \
    const bf16x8_hl f0 = small_park(A0, M0, W0, row_ok, masked, &sB[st][0][sh][sc]);                  \
    const bf16x8_hl f1 = small_park(A1, M1, W1, row_ok, masked, &sB[st][0][sh + 4][sc]);              \
    if ((S) + 2 < steps) SMALL_FETCH((S) + 2, A0, A1, M0, M1, W0, W1);                        \
    __syncthreads();                                                                          \
    _Pragma("unroll") for (int cb = 0; cb < 4; ++cb) {                                        \
      frag_u bh, bl;                                                                          \
      bh.q = sB[st][0][h][cb * 16 + (lane & 15)];                                             \
      bl.q = sB[st][1][h][cb * 16 + (lane & 15)];                                             \
      acc[cb] = mfma3_hh_hl_lh_16x16(bf16x8_hl{bh.v, bl.v}, f0, acc[cb]);                     \
    }                                                                                         \
    _Pragma("unroll") for (int cb = 0; cb < 4; ++cb) {                                        \
      frag_u bh, bl;                                                                          \
      bh.q = sB[st][0][h + 4][cb * 16 + (lane & 15)];                                         \
      bl.q = sB[st][1][h + 4][cb * 16 + (lane & 15)];                                         \
      acc[cb] = mfma3_hh_hl_lh_16x16(bf16x8_hl{bh.v, bl.v}, f1, acc[cb]);                     \
    }                                                                                         \
  } while (0)

  const int steps = C >> 6;
  SMALL_FETCH(0, a00, a01, m00, m01, w00, w01);
  if (steps > 1) SMALL_FETCH(1, a10, a11, m10, m11, w10, w11);
#pragma unroll 1
  for (int s = 0; s < steps; s += 2) {
    SMALL_CONSUME(s, a00, a01, m00, m01, w00, w01);
    if (s + 1 < steps) SMALL_CONSUME(s + 1, a10, a11, m10, m11, w10, w11);
  }
#undef SMALL_FETCH
#undef SMALL_CONSUME
  // D[m][n]: m = output column cb * 16 + 4 (lane >> 4) + register, n = the row (lane & 15) of the wave's strip
  if (row_ok) {
    float *op = out + (size_t)r * NO + col0 + 4 * h;
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
      float4 v = make_float4(acc[cb][0], acc[cb][1], acc[cb][2], acc[cb][3]);
      if (!DX) {
        if (bias) {
          const float4 b = *reinterpret_cast<const float4 *>(bias + col0 + cb * 16 + 4 * h);
          v.x += b.x, v.y += b.y, v.z += b.z, v.w += b.w;
        }
        if (relu) v.x = fmaxf(v.x, 0.f), v.y = fmaxf(v.y, 0.f), v.z = fmaxf(v.z, 0.f), v.w = fmaxf(v.w, 0.f);
      }
      *reinterpret_cast<float4 *>(op + cb * 16) = v;
    }
  }
}

__global__ __launch_bounds__(256) void small_linear_fwd_kernel(const float *__restrict__ x, const float *__restrict__ w, const float *__restrict__ bias, int rows,
                                                               int N, int K, int relu, float *__restrict__ y) {
  small_linear_body<false>(x, nullptr, w, bias, rows, N, K, relu, y, blockIdx.x, blockIdx.y);
}
__global__ __launch_bounds__(256) void small_linear_dx_kernel(const float *__restrict__ g, const float *__restrict__ y, const float *__restrict__ w, int rows, int N,
                                                              int K, float *__restrict__ dx) {
  small_linear_body<true>(g, y, w, nullptr, rows, K, N, 0, dx, blockIdx.x, blockIdx.y);
}

// Row slices of the weight gradient: about 256 workgroups (one wave per SIMD of the chip), at least 32 rows per slice.  (512 workgroups were
// measured too: the main kernel no faster, twice the partials for the combining launch to read.)
__host__ __device__ inline int small_slices(int rows, int N, int K) {
  const int tiles = (N >> 6) * (K >> 6);
  const int want = (256 + tiles - 1) / tiles, cap = (rows + 31) / 32;
  return want < cap ? want : cap;
}
// rows per slice: even (the matrix instruction takes two rows per step)
__host__ __device__ inline int small_slice_rows(int rows, int slices) { return (((rows + slices - 1) / slices) + 1) & ~1; }

struct small_wgrad_regs {
  float a[16], m[16], b[16];
};

// part: [slices][N * K] partial dW, then [slices][N] partial db.
__device__ __forceinline__ void small_wgrad_body(const float *__restrict__ g, const float *__restrict__ y, const float *__restrict__ x, int rows, int N, int K,
                                                 int per, float *__restrict__ part, int bx, int by, int slices) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), col = lane & 31, kh = lane >> 5;
  const int tiles_k = K >> 6, tn = bx / tiles_k, tk = bx - tn * tiles_k;
  const int n0 = tn * 64 + (wave >> 1) * 32, k0 = tk * 64 + (wave & 1) * 32;
  const int r0 = by * per, r1 = min(rows, r0 + per);  // (r0 may lie past `rows` in the last slices: they write zeros)
  const bool masked = y != nullptr;
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  float bsum = 0.f;
  // A trip = 16 row pairs (lane half kh takes the even / odd row of a pair); a row at or past r1 reads as zero.  Loads only: the mask is
  // applied in `consume`, so the next trip's loads stay in flight under this trip's matrix instructions.
  auto fetch = [&](int r, small_wgrad_regs &R) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int rr = r + 2 * u + kh;
      const bool ok = rr < r1;
      const size_t row = ok ? rr : 0;
      R.a[u] = ok ? g[row * N + n0 + col] : 0.f;
      R.b[u] = ok ? x[row * K + k0 + col] : 0.f;
      if (masked) R.m[u] = ok ? y[row * N + n0 + col] : 0.f;
    }
  };
  auto consume = [&](small_wgrad_regs &R) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const float av = masked ? (R.m[u] > 0.f ? R.a[u] : 0.f) : R.a[u];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, R.b[u], acc, 0, 0, 0);
      bsum += av;
    }
  };
  small_wgrad_regs R0, R1;
  if (r0 < r1) fetch(r0, R0);
#pragma unroll 1
  for (int r = r0; r < r1; r += 64) {
    if (r + 32 < r1) fetch(r + 32, R1);
    consume(R0);
    if (r + 32 < r1) {
      if (r + 64 < r1) fetch(r + 64, R0);
      consume(R1);
    }
  }
  // D[m][n]: m = the A lane's column of g (n0 + m), n = the B lane's column of x (k0 + col)
  float *out = part + (size_t)by * N * K;
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) {
    const int m = (rr & 3) + 8 * (rr >> 2) + 4 * kh;
    out[(size_t)(n0 + m) * K + k0 + col] = acc[rr];
  }
  if (tk == 0 && (wave & 1) == 0) {  // (wave-uniform) even rows in lanes 0..31, odd rows in lanes 32..63: even + odd
    const float other = __shfl_xor(bsum, 32);
    if (kh == 0) part[(size_t)slices * N * K + (size_t)by * N + n0 + col] = bsum + other;
  }
}

__global__ __launch_bounds__(256) void small_wgrad_kernel(const float *__restrict__ g, const float *__restrict__ y, const float *__restrict__ x, int rows, int N,
                                                          int K, int per, float *__restrict__ part) {
  small_wgrad_body(g, y, x, rows, N, K, per, part, blockIdx.x, blockIdx.y, gridDim.y);
}

// dX and the weight-gradient partials in ONE launch: both are bound by latency (a workgroup or two per CU), so they run side by side instead of
// one behind the other.  The first tiles * slices workgroups take the weight gradient (the longer job first), the rest the 64 x 64 tiles of dX.
__global__ __launch_bounds__(256) void small_backward_kernel(const float *__restrict__ g, const float *__restrict__ y, const float *__restrict__ x,
                                                             const float *__restrict__ w, int rows, int N, int K, int per, int slices, float *__restrict__ dx,
                                                             float *__restrict__ part) {
  const int tiles = (N >> 6) * (K >> 6), n_w = tiles * slices, id = blockIdx.x;  // (workgroup-uniform branch)
  if (id < n_w) {
    small_wgrad_body(g, y, x, rows, N, K, per, part, id % tiles, id / tiles, slices);
  } else {
    const int j = id - n_w, tk = K >> 6;
    small_linear_body<true>(g, y, w, nullptr, rows, K, N, 0, dx, j % tk, j / tk);
  }
}

// dw[e] = sum over the slices, in slice order, in double; elements N K .. N K + N - 1 are db (when asked for).
__global__ __launch_bounds__(256) void small_wgrad_combine_kernel(const float *__restrict__ part, int slices, int NK, int N, float *__restrict__ dw,
                                                                  float *__restrict__ db) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < NK) {
    double s = 0.0;
    for (int i = 0; i < slices; ++i) s += (double)part[(size_t)i * NK + e];
    dw[e] = (float)s;
  } else if (db && e < NK + N) {
    const float *p = part + (size_t)slices * NK + (e - NK);
    double s = 0.0;
    for (int i = 0; i < slices; ++i) s += (double)p[(size_t)i * N];
    db[e - NK] = (float)s;
  }
}

inline bool small_domain(long rows, int N, int K) {
  return rows >= 1 && rows <= SL_MAX_ROWS && N >= 64 && N <= 512 && K >= 64 && K <= 512 && N % 64 == 0 && K % 64 == 0;
}
inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

}  // namespace unopose

using namespace unopose;

extern "C" {

int unopose_linear_small_train_ws_floats(long rows, int N, int K) {  // (at most 2^20 + 2^12 floats inside the domain); -1 outside it
  if (!small_domain(rows, N, K)) return -1;
  return small_slices((int)rows, N, K) * (N * K + N);
}

int unopose_linear_small_train_forward(const float *x, const float *w, const float *bias, long rows, int N, int K, int relu, float *y,
                                       unopose_stream_t stream) {
  UNOPOSE_REQUIRE(x && w && y, "linear_small_train_forward: null pointer");
  UNOPOSE_REQUIRE(small_domain(rows, N, K), "linear_small_train_forward: outside the domain 1 <= rows <= 16383, N and K multiples of 64 in [64, 512] (rows=%ld N=%d K=%d)",
                  rows, N, K);
  UNOPOSE_REQUIRE(aligned16(x) && aligned16(w) && aligned16(y) && aligned16(bias), "linear_small_train_forward: tensors must be 16-byte aligned");
  hipLaunchKernelGGL(small_linear_fwd_kernel, dim3(N >> 6, cdiv(rows, 64)), dim3(256), 0, (hipStream_t)stream, x, w, bias, (int)rows, N, K, relu ? 1 : 0, y);
  return check_launch("linear_small_train_forward");
}

int unopose_linear_small_train_dx(const float *g, const float *y, const float *w, long rows, int N, int K, float *dx, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(g && w && dx, "linear_small_train_dx: null pointer");
  UNOPOSE_REQUIRE(small_domain(rows, N, K), "linear_small_train_dx: outside the domain 1 <= rows <= 16383, N and K multiples of 64 in [64, 512] (rows=%ld N=%d K=%d)", rows,
                  N, K);
  UNOPOSE_REQUIRE(aligned16(g) && aligned16(y) && aligned16(w) && aligned16(dx), "linear_small_train_dx: tensors must be 16-byte aligned");
  hipLaunchKernelGGL(small_linear_dx_kernel, dim3(K >> 6, cdiv(rows, 64)), dim3(256), 0, (hipStream_t)stream, g, y, w, (int)rows, N, K, dx);
  return check_launch("linear_small_train_dx");
}

int unopose_linear_small_train_dwdb(const float *g, const float *y, const float *x, long rows, int N, int K, float *workspace, long workspace_floats,
                                    float *dw, float *db, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(g && x && workspace && dw, "linear_small_train_dwdb: null pointer");
  UNOPOSE_REQUIRE(small_domain(rows, N, K), "linear_small_train_dwdb: outside the domain 1 <= rows <= 16383, N and K multiples of 64 in [64, 512] (rows=%ld N=%d K=%d)",
                  rows, N, K);
  UNOPOSE_REQUIRE(workspace_floats >= unopose_linear_small_train_ws_floats(rows, N, K), "linear_small_train_dwdb: workspace of %ld floats, %d needed",
                  workspace_floats, unopose_linear_small_train_ws_floats(rows, N, K));
  UNOPOSE_REQUIRE(aligned16(g) && aligned16(y) && aligned16(x) && aligned16(workspace) && aligned16(dw), "linear_small_train_dwdb: tensors must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int slices = small_slices((int)rows, N, K), per = small_slice_rows((int)rows, slices);
  hipLaunchKernelGGL(small_wgrad_kernel, dim3((N >> 6) * (K >> 6), slices), dim3(256), 0, s, g, y, x, (int)rows, N, K, per, workspace);
  if (check_launch("linear_small_train_dwdb")) return UNOPOSE_ELAUNCH;
  hipLaunchKernelGGL(small_wgrad_combine_kernel, dim3(cdiv((long)N * K + N, 256)), dim3(256), 0, s, (const float *)workspace, slices, N * K, N, dw, db);
  return check_launch("linear_small_train_dwdb_combine");
}

int unopose_linear_small_train_backward(const float *g, const float *y, const float *x, const float *w, long rows, int N, int K, float *workspace,
                                        long workspace_floats, float *dx, float *dw, float *db, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(g && x && w && workspace && dx && dw, "linear_small_train_backward: null pointer");
  UNOPOSE_REQUIRE(small_domain(rows, N, K), "linear_small_train_backward: outside the domain 1 <= rows <= 16383, N and K multiples of 64 in [64, 512] (rows=%ld N=%d K=%d)",
                  rows, N, K);
  UNOPOSE_REQUIRE(workspace_floats >= unopose_linear_small_train_ws_floats(rows, N, K), "linear_small_train_backward: workspace of %ld floats, %d needed",
                  workspace_floats, unopose_linear_small_train_ws_floats(rows, N, K));
  UNOPOSE_REQUIRE(aligned16(g) && aligned16(y) && aligned16(x) && aligned16(w) && aligned16(workspace) && aligned16(dx) && aligned16(dw),
                  "linear_small_train_backward: tensors must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int slices = small_slices((int)rows, N, K), per = small_slice_rows((int)rows, slices);
  const int grid = (N >> 6) * (K >> 6) * slices + (K >> 6) * cdiv(rows, 64);
  hipLaunchKernelGGL(small_backward_kernel, dim3(grid), dim3(256), 0, s, g, y, x, w, (int)rows, N, K, per, slices, dx, workspace);
  if (check_launch("linear_small_train_backward")) return UNOPOSE_ELAUNCH;
  hipLaunchKernelGGL(small_wgrad_combine_kernel, dim3(cdiv((long)N * K + N, 256)), dim3(256), 0, s, (const float *)workspace, slices, N * K, N, dw, db);
  return check_launch("linear_small_train_backward_combine");
}

}  // extern "C"
