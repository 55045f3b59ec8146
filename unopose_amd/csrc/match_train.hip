// The match head of the training step without the (B, R, C) similarity (C ABI part 2, gfx950): for unit rows a (B, R, 256), b (B, C, 256)
// and S = tau a b^T the row / column log-sum-exps, the saliency sums, the labelled entries and the row arg max (forward), and the
// gradients of a, b, s1, s2 (backward), each from sweeps that recompute S tile by tile (DESIGN.md "Matching losses under autograd").
//
// ONE row-owner design, launched twice per direction: a wave owns 16 rows of X, a workgroup (4 waves) 64; the rows of Y go through LDS in
// tiles of MT_CT = 32, already split into bf16 hi / lo planes by `match_split_kernel`.  The column quantities are the row quantities of
// S^T, so the column launch is the row launch with (X, Y) and the per-row / per-column vectors swapped.  Every output element is written
// by one lane of one workgroup; there are no atomics.
//
// Fragment layout.  The S tile is formed TRANSPOSED (Y rows as the MFMA's A operand, the owned rows as its B operand): a lane then holds,
// for the owned row `lane & 15`, the four columns 4 (lane >> 4) + r of each 16-column sub-tile -- all row reductions stay inside the lane
// until the end of the sweep, where the four lanes of a row are merged once.  In the backward those 8 values (two sub-tiles) are exactly the
// A operand of the next product dX += G Y when the sum index k = 8 (lane >> 4) + e is read as column (e < 4 ? 4 g + e : 16 + 4 g + e - 4):
// the Y^T planes are read in that order (two 8-byte pieces per plane), and G never leaves the registers.
#include "common.h"

namespace unopose {

constexpr int MT_D = 256;            // feature width
constexpr int MT_ROWS = 64;          // rows of X per workgroup (16 per wave)
constexpr int MT_CT = 32;            // rows of Y per LDS tile
constexpr int MT_PAD = 64;           // the planes' row counts are padded to a multiple of this (zero rows)
constexpr int MT_LDB = MT_D + 8;     // u16 stride of a row-plane line in LDS (528 B: the 16 rows of a ds_read_b128 group on distinct banks)
constexpr int MT_LDT = MT_CT + 8;    // u16 stride of a transposed-plane line in LDS (80 B: conflict-free 8-byte reads)
constexpr float MT_BIG = 3e38f;
constexpr int MT_SPLIT_ROWS = MT_CT;  // rows per workgroup of the split pass = one tile of the transposed planes

// x (B, N, 256) fp32 -> planes: [rows hi | rows lo] each (B, Np, 256) u16, [T hi | T lo] each (B, Np / 32, 256, 32) u16 (per 32-row tile the
// transposed block, so that a tile of either kind is ONE contiguous 16 KiB piece per plane); rows >= N are zero.
// with_t == 0: only the two row planes are written (and `planes` holds only them).
__global__ __launch_bounds__(256) void match_split_kernel(const float *__restrict__ x, int N, int Np, int with_t, u16 *__restrict__ planes) {
  __shared__ u16 Th[MT_SPLIT_ROWS][MT_D + 2], Tl[MT_SPLIT_ROWS][MT_D + 2];
  const int b = blockIdx.y, r0 = blockIdx.x * MT_SPLIT_ROWS, tid = threadIdx.x;
  const size_t plane = (size_t)gridDim.y * Np * MT_D;
  u16 *Rh = planes, *Rl = planes + plane, *Xh = planes + 2 * plane, *Xl = planes + 3 * plane;
#pragma unroll
  for (int i = 0; i < MT_SPLIT_ROWS * (MT_D / 4) / 256; ++i) {
    const int e = tid + i * 256, row = e >> 6, c4 = e & 63;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r0 + row < N) v = *reinterpret_cast<const float4 *>(x + ((size_t)b * N + r0 + row) * MT_D + c4 * 4);
    uint2 h, l;
    h.x = cvt_pk_bf16_f32(v.x, v.y);
    h.y = cvt_pk_bf16_f32(v.z, v.w);
    l.x = cvt_pk_bf16_lo(v.x, v.y, h.x);
    l.y = cvt_pk_bf16_lo(v.z, v.w, h.y);
    const size_t o = ((size_t)b * Np + r0 + row) * MT_D + c4 * 4;
    *reinterpret_cast<uint2 *>(Rh + o) = h;
    *reinterpret_cast<uint2 *>(Rl + o) = l;
    uint32_t *th = reinterpret_cast<uint32_t *>(&Th[row][c4 * 4]), *tl = reinterpret_cast<uint32_t *>(&Tl[row][c4 * 4]);
    th[0] = h.x;
    th[1] = h.y;
    tl[0] = l.x;
    tl[1] = l.y;
  }
  if (!with_t) return;
  __syncthreads();
  // thread = feature: 32 consecutive rows of the transposed planes (64 B per plane)
  uint32_t ph[MT_SPLIT_ROWS / 2], pl[MT_SPLIT_ROWS / 2];
#pragma unroll
  for (int j = 0; j < MT_SPLIT_ROWS / 2; ++j) {
    ph[j] = (uint32_t)Th[2 * j][tid] | ((uint32_t)Th[2 * j + 1][tid] << 16);
    pl[j] = (uint32_t)Tl[2 * j][tid] | ((uint32_t)Tl[2 * j + 1][tid] << 16);
  }
  const size_t ot = (((size_t)b * (Np / MT_SPLIT_ROWS) + blockIdx.x) * MT_D + tid) * MT_SPLIT_ROWS;
#pragma unroll
  for (int q = 0; q < MT_SPLIT_ROWS / 8; ++q) {
    *reinterpret_cast<uint4 *>(Xh + ot + q * 8) = make_uint4(ph[4 * q], ph[4 * q + 1], ph[4 * q + 2], ph[4 * q + 3]);
    *reinterpret_cast<uint4 *>(Xl + ot + q * 8) = make_uint4(pl[4 * q], pl[4 * q + 1], pl[4 * q + 2], pl[4 * q + 3]);
  }
}

// The owned rows' fragments: lane (li = lane & 15, g = lane >> 4) holds elements ks * 32 + g * 8 .. + 7 of row `row` (clamped by the caller).
__device__ __forceinline__ void mt_load_rows(const u16 *__restrict__ Rh, const u16 *__restrict__ Rl, size_t row, int g, bf16x8_hl (&xf)[8]) {
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) {
    const size_t o = row * MT_D + ks * 32 + g * 8;
    xf[ks].hi = *reinterpret_cast<const bf16x8 *>(Rh + o);
    xf[ks].lo = *reinterpret_cast<const bf16x8 *>(Rl + o);
  }
}

// Rows j0 .. j0 + 31 of Y's row planes: global -> registers (all loads in flight together) and registers -> LDS, as two steps, so that a
// caller can put work between them.  The planes are zero-padded: no bounds.
constexpr int MT_STAGE = 2 * MT_CT * (MT_D / 8) / 256;  // 16-byte pieces per thread and pair of planes
typedef uint32_t mt_u32x4 __attribute__((ext_vector_type(4)));  // (a native vector: an array of HIP's uint4 struct stays in scratch memory)
__device__ __forceinline__ void mt_fetch_rows(const u16 *__restrict__ Yh, const u16 *__restrict__ Yl, size_t row0, int tid, mt_u32x4 (&buf)[MT_STAGE]) {
#pragma unroll
  for (int i = 0; i < MT_STAGE; ++i) {
    const int e = tid + i * 256, pl = e >> 10, row = (e >> 5) & 31, c = e & 31;
    buf[i] = *reinterpret_cast<const mt_u32x4 *>((pl ? Yl : Yh) + (row0 + row) * MT_D + c * 8);
  }
}
__device__ __forceinline__ void mt_store_rows(const mt_u32x4 (&buf)[MT_STAGE], u16 *Bh, u16 *Bl, int tid) {
#pragma unroll
  for (int i = 0; i < MT_STAGE; ++i) {
    const int e = tid + i * 256, pl = e >> 10, row = (e >> 5) & 31, c = e & 31;
    *reinterpret_cast<mt_u32x4 *>((pl ? Bl : Bh) + row * MT_LDB + c * 8) = buf[i];
  }
}
// The tile's transposed block (contiguous per plane in global memory), the same way.
__device__ __forceinline__ void mt_fetch_t(const u16 *__restrict__ YTh, const u16 *__restrict__ YTl, size_t tile, int tid, mt_u32x4 (&buf)[MT_STAGE]) {
#pragma unroll
  for (int i = 0; i < MT_STAGE; ++i) {
    const int e = tid + i * 256, pl = e >> 10;
    buf[i] = *reinterpret_cast<const mt_u32x4 *>((pl ? YTl : YTh) + tile * (MT_D * MT_CT) + (size_t)(e & 1023) * 8);
  }
}
__device__ __forceinline__ void mt_store_t(const mt_u32x4 (&buf)[MT_STAGE], u16 *Th, u16 *Tl, int tid) {
#pragma unroll
  for (int i = 0; i < MT_STAGE; ++i) {
    const int e = tid + i * 256, pl = e >> 10, f = (e >> 2) & 255, c = e & 3;
    *reinterpret_cast<mt_u32x4 *>((pl ? Tl : Th) + f * MT_LDT + c * 8) = buf[i];
  }
}

// S^T of the tile, unscaled: s[t][r] = x_(row of lane & 15) . y_(j0 + 16 t + 4 g + r)
__device__ __forceinline__ void mt_scores(const u16 *Bh, const u16 *Bl, const bf16x8_hl (&xf)[8], int li, int g, f32x4 (&s)[2]) {
  s[0] = f32x4{0.f, 0.f, 0.f, 0.f};
  s[1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < 8; ++ks)
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int off = (t * 16 + li) * MT_LDB + ks * 32 + g * 8;
      const bf16x8_hl yf{*reinterpret_cast<const bf16x8 *>(Bh + off), *reinterpret_cast<const bf16x8 *>(Bl + off)};
      s[t] = mfma3_hh_hl_lh_16x16(yf, xf[ks], s[t]);
    }
}

// Workgroups are dealt round-robin over the 8 XCDs (each with its own L2).  All row blocks of a batch element stream the SAME rows of Y, so
// the linear workgroup index is remapped (bijectively) to give every XCD a contiguous run of (batch, row block) pairs: at 8 x 4097 one
// batch element per XCD, whose Y tiles the 64 co-running workgroups then find in that L2.
constexpr int MT_XCD = 8;
__device__ __forceinline__ void mt_block(int nblk, int &b, int &blk) {
  const int total = (int)gridDim.x, lin = (int)blockIdx.x, k = lin % MT_XCD, q = total / MT_XCD, r = total % MT_XCD;
  const int v = k * q + min(k, r) + lin / MT_XCD;
  b = v / nblk;
  blk = v - b * nblk;
}

__device__ __forceinline__ float mt_xor16(float v) { return __shfl_xor(v, 16); }
__device__ __forceinline__ float mt_xor32(float v) { return __shfl_xor(v, 32); }
// sum over the four lanes of a row (lanes li, li + 16, li + 32, li + 48); the same value in all four
__device__ __forceinline__ float mt_sum4(float v) {
  v += mt_xor16(v);
  return v + mt_xor32(v);
}

// ---- forward sweep: rows i = 1 .. R - 1 of X against all rows j of Y.  Per row i: L = lse_{j >= 0} S_ij, F = lse_{j >= 1} S_ij,
// m = sum_{j >= 1} exp(S_ij - F) sv_j, pred = arg max_{j >= 0} S_ij (may be null), picked = S_{i, lab_i}.  Outputs are (B, R - 1).
__global__ __launch_bounds__(256, 2) void match_fwd_kernel(const u16 *__restrict__ Xh, const u16 *__restrict__ Xl, const u16 *__restrict__ Yh,
                                                        const u16 *__restrict__ Yl, int R, int Rp, int C, int Cp, float tau,
                                                        const float *__restrict__ sv, const int *__restrict__ lab, float *__restrict__ L,
                                                        float *__restrict__ F, float *__restrict__ m, int *__restrict__ pred,
                                                        float *__restrict__ picked) {
  __shared__ __attribute__((aligned(16))) u16 Bh[MT_CT * MT_LDB], Bl[MT_CT * MT_LDB];
  __shared__ __attribute__((aligned(16))) float Sv[MT_CT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, g = lane >> 4;
  int b, blk;
  mt_block((R - 1 + MT_ROWS - 1) / MT_ROWS, b, blk);
  const int i = 1 + blk * MT_ROWS + wave * 16 + li;
  const bool row_ok = i < R;
  bf16x8_hl xf[8];
  mt_load_rows(Xh, Xl, (size_t)b * Rp + min(i, Rp - 1), g, xf);
  const int label = row_ok ? lab[(size_t)b * (R - 1) + i - 1] : -1;
  float mF = -MT_BIG, sF = 0.f, wF = 0.f, s0 = 0.f, pk = 0.f, best = -MT_BIG;
  int besti = 0;
  mt_u32x4 pre[MT_STAGE];  // the next tile, fetched while the current one is multiplied
  mt_fetch_rows(Yh, Yl, (size_t)b * Cp, tid, pre);
  for (int j0 = 0; j0 < C; j0 += MT_CT) {
    __syncthreads();
    mt_store_rows(pre, Bh, Bl, tid);
    if (tid < MT_CT) {
      const int j = j0 + tid;
      Sv[tid] = (j >= 1 && j < C) ? sv[(size_t)b * (C - 1) + j - 1] : 0.f;
    }
    __syncthreads();
    if (j0 + MT_CT < C) mt_fetch_rows(Yh, Yl, (size_t)b * Cp + j0 + MT_CT, tid, pre);
    f32x4 s[2];
    mt_scores(Bh, Bl, xf, li, g, s);
    float x[8], v[8];
    float mt = -MT_BIG;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const float4 sv4 = *reinterpret_cast<const float4 *>(&Sv[t * 16 + g * 4]);
      v[t * 4 + 0] = sv4.x, v[t * 4 + 1] = sv4.y, v[t * 4 + 2] = sv4.z, v[t * 4 + 3] = sv4.w;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = j0 + t * 16 + g * 4 + r;
        const float xv = s[t][r] * tau;
        if (j < C && xv > best) best = xv, besti = j;  // columns ascend within the lane: the first maximum is kept
        if (j == label) pk = xv;
        if (j == 0) s0 = xv;
        x[t * 4 + r] = (j >= 1 && j < C) ? xv : -MT_BIG;
        mt = fmaxf(mt, x[t * 4 + r]);
      }
    }
    const float mn = fmaxf(mF, mt), alpha = __expf(mF - mn);
    float ps = 0.f, pw = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float p = x[e] > -MT_BIG ? __expf(x[e] - mn) : 0.f;
      ps += p;
      pw += p * v[e];
    }
    sF = sF * alpha + ps;
    wF = wF * alpha + pw;
    mF = mn;
  }
  // merge the four lanes of a row
  {
    float M = fmaxf(mF, mt_xor16(mF));
    M = fmaxf(M, mt_xor32(M));
    const float sc = __expf(mF - M);  // a lane that saw no column >= 1 has sF = wF = 0
    sF = mt_sum4(sF * sc);
    wF = mt_sum4(wF * sc);
    mF = M;
    s0 = mt_sum4(s0);
    pk = mt_sum4(pk);
#pragma unroll
    for (int sh = 16; sh <= 32; sh *= 2) {
      const float ob = __shfl_xor(best, sh);
      const int oi = __shfl_xor(besti, sh);
      if (ob > best || (ob == best && oi < besti)) best = ob, besti = oi;
    }
  }
  if (g == 0 && row_ok) {
    const float Fv = mF + logf(sF), M = fmaxf(Fv, s0);
    const size_t o = (size_t)b * (R - 1) + i - 1;
    F[o] = Fv;
    L[o] = M + logf(expf(Fv - M) + expf(s0 - M));
    m[o] = wF / sF;
    picked[o] = pk;
    if (pred) pred[o] = besti;
  }
}

// ---- backward sweep: rows i = 0 .. R - 1 of X.  With the row scalars (Lr, Fr, mr, gr, sr, labr: (B, R - 1), rows >= 1) and the column
// vectors (Lc, Fc, mc, gc, sc, labc: (B, C - 1), columns >= 1), wr = gL / (2 (R - 1)), wc = gL / (2 (C - 1)):
//   G_ij = [i >= 1] wr (e^{S - Lr_i} - [j == labr_i]) + [j >= 1] wc (e^{S - Lc_j} - [i == labc_j])
//        + [i >= 1, j >= 1] (gr_i e^{S - Fr_i} (sc_j - mr_i) + gc_j e^{S - Fc_j} (sr_i - mc_j))
//   dX_i = tau sum_j G_ij y_j  (B, R, 256),   dsr_i = sum_{j >= 1} gc_j e^{S_ij - Fc_j}  (B, R - 1)
constexpr int MT_NV = 6;  // column vectors staged per tile
__global__ __launch_bounds__(256, 2) void match_bwd_kernel(const u16 *__restrict__ Xh, const u16 *__restrict__ Xl, const u16 *__restrict__ Yh,
                                                           const u16 *__restrict__ Yl, const u16 *__restrict__ YTh,
                                                           const u16 *__restrict__ YTl, int R, int Rp, int C, int Cp, float tau,
                                                           const float *__restrict__ Lr, const float *__restrict__ Fr,
                                                           const float *__restrict__ mr, const float *__restrict__ gr,
                                                           const float *__restrict__ sr, const int *__restrict__ labr,
                                                           const float *__restrict__ Lc, const float *__restrict__ Fc,
                                                           const float *__restrict__ mc, const float *__restrict__ gc,
                                                           const float *__restrict__ sc, const int *__restrict__ labc,
                                                           const float *__restrict__ gL, float *__restrict__ dX, float *__restrict__ dsr) {
  extern __shared__ __attribute__((aligned(16))) unsigned char mt_smem[];
  u16 *Bh = reinterpret_cast<u16 *>(mt_smem), *Bl = Bh + MT_CT * MT_LDB, *Th = Bl + MT_CT * MT_LDB, *Tl = Th + MT_D * MT_LDT;
  float *Cv = reinterpret_cast<float *>(Tl + MT_D * MT_LDT);  // [MT_NV][MT_CT]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, g = lane >> 4;
  int b, blk;
  mt_block((R + MT_ROWS - 1) / MT_ROWS, b, blk);
  const int row0 = blk * MT_ROWS + wave * 16, i = row0 + li;
  const bool fg = i >= 1 && i < R;
  bf16x8_hl xf[8];
  mt_load_rows(Xh, Xl, (size_t)b * Rp + min(i, Rp - 1), g, xf);
  const size_t ro = (size_t)b * (R - 1) + (fg ? i - 1 : 0);
  const float gl = gL[b];
  const float Lri = fg ? Lr[ro] : MT_BIG, Fri = fg ? Fr[ro] : MT_BIG, mri = fg ? mr[ro] : 0.f, gri = fg ? gr[ro] : 0.f, sri = fg ? sr[ro] : 0.f;
  const int labi = fg ? labr[ro] : -1;
  const float wr = fg ? gl * (0.5f / (float)(R - 1)) : 0.f, wc = i < R ? gl * (0.5f / (float)(C - 1)) : 0.f;
  f32x4 acc[16];
#pragma unroll
  for (int f = 0; f < 16; ++f) acc[f] = f32x4{0.f, 0.f, 0.f, 0.f};
  float ds = 0.f;
  for (int j0 = 0; j0 < C; j0 += MT_CT) {
    {  // one memory round trip per kind of tile, each with all its loads in flight together (32 registers, free between two tiles)
      mt_u32x4 buf[MT_STAGE];
      mt_fetch_rows(Yh, Yl, (size_t)b * Cp + j0, tid, buf);
      __syncthreads();
      mt_store_rows(buf, Bh, Bl, tid);
      mt_fetch_t(YTh, YTl, (size_t)b * (Cp / MT_CT) + j0 / MT_CT, tid, buf);
      mt_store_t(buf, Th, Tl, tid);
    }
    if (tid < MT_NV * MT_CT) {
      const int v = tid >> 5, j = j0 + (tid & 31);
      const bool ok = j >= 1 && j < C;
      const size_t co = (size_t)b * (C - 1) + (ok ? j - 1 : 0);
      float val;
      if (v == 0) val = ok ? Lc[co] : MT_BIG;
      else if (v == 1) val = ok ? Fc[co] : MT_BIG;
      else if (v == 2) val = ok ? mc[co] : 0.f;
      else if (v == 3) val = ok ? gc[co] : 0.f;
      else if (v == 4) val = ok ? sc[co] : 0.f;
      else val = __int_as_float(ok ? labc[co] : -1);
      Cv[v * MT_CT + (tid & 31)] = val;
    }
    __syncthreads();
    f32x4 s[2];
    mt_scores(Bh, Bl, xf, li, g, s);
    float G[8];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int q = t * 16 + g * 4;
      const float4 Lc4 = *reinterpret_cast<const float4 *>(&Cv[0 * MT_CT + q]), Fc4 = *reinterpret_cast<const float4 *>(&Cv[1 * MT_CT + q]);
      const float4 mc4 = *reinterpret_cast<const float4 *>(&Cv[2 * MT_CT + q]), gc4 = *reinterpret_cast<const float4 *>(&Cv[3 * MT_CT + q]);
      const float4 sc4 = *reinterpret_cast<const float4 *>(&Cv[4 * MT_CT + q]), lc4 = *reinterpret_cast<const float4 *>(&Cv[5 * MT_CT + q]);
      const float Lcv[4] = {Lc4.x, Lc4.y, Lc4.z, Lc4.w}, Fcv[4] = {Fc4.x, Fc4.y, Fc4.z, Fc4.w}, mcv[4] = {mc4.x, mc4.y, mc4.z, mc4.w};
      const float gcv[4] = {gc4.x, gc4.y, gc4.z, gc4.w}, scv[4] = {sc4.x, sc4.y, sc4.z, sc4.w}, lcv[4] = {lc4.x, lc4.y, lc4.z, lc4.w};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = j0 + q + r;
        const float x = j < C ? s[t][r] * tau : -MT_BIG;  // a padded column: every exponential below is 0
        const float er = __expf(x - Lri), ec = __expf(x - Lcv[r]), efr = __expf(x - Fri), efc = __expf(x - Fcv[r]);
        const float dc = fg ? gcv[r] * efc : 0.f;
        float gv = wr * (er - (j == labi ? 1.f : 0.f)) + wc * (ec - (i == __float_as_int(lcv[r]) ? 1.f : 0.f));
        gv += (j >= 1 ? gri * efr * (scv[r] - mri) : 0.f) + dc * (sri - mcv[r]);
        ds += dc;
        G[t * 4 + r] = gv;
      }
    }
    const bf16x8_hl gf = split8_bf16(G);
#pragma unroll
    for (int f = 0; f < 16; ++f) {
      const int off = (f * 16 + li) * MT_LDT + g * 4;
      union {
        bf16x8 v;
        uint2 h2[2];
      } YH, YL;
      YH.h2[0] = *reinterpret_cast<const uint2 *>(Th + off);
      YH.h2[1] = *reinterpret_cast<const uint2 *>(Th + off + 16);
      YL.h2[0] = *reinterpret_cast<const uint2 *>(Tl + off);
      YL.h2[1] = *reinterpret_cast<const uint2 *>(Tl + off + 16);
      acc[f] = mfma3_hh_hl_lh_16x16(gf, bf16x8_hl{YH.v, YL.v}, acc[f]);
    }
  }
  ds = mt_sum4(ds);
  if (g == 0 && fg) dsr[ro] = ds;
  // acc[f][r]: row row0 + 4 g + r, feature 16 f + li
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = row0 + g * 4 + r;
    if (row < R) {
      float *o = dX + ((size_t)b * R + row) * MT_D + li;
#pragma unroll
      for (int f = 0; f < 16; ++f) o[f * 16] = acc[f][r] * tau;
    }
  }
}

constexpr size_t MT_BWD_LDS = (size_t)(2 * MT_CT * MT_LDB + 2 * MT_D * MT_LDT) * sizeof(u16) + MT_NV * MT_CT * sizeof(float);
static_assert(2 * MT_BWD_LDS <= 160 * 1024, "two backward workgroups per CU");

}  // namespace unopose

using namespace unopose;

extern "C" {

int unopose_match_train_pad(void) { return MT_PAD; }

int unopose_match_train_split(const float *x, int B, int N, int Np, int with_t, void *planes, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(x && planes, "match_train_split: null pointer");
  UNOPOSE_REQUIRE(B >= 0 && B <= 65535 && N >= 1 && Np >= N && Np % MT_PAD == 0, "match_train_split: bad sizes (B=%d N=%d Np=%d)", B, N, Np);
  if (B == 0) return UNOPOSE_OK;
  hipLaunchKernelGGL(match_split_kernel, dim3(Np / MT_SPLIT_ROWS, B), dim3(256), 0, (hipStream_t)stream, x, N, Np, with_t, (u16 *)planes);
  return check_launch("match_train_split");
}

int unopose_match_train_forward(const void *xplanes, const void *yplanes, int B, int R, int Rp, int C, int Cp, float tau, const float *sv,
                                const int *lab, float *L, float *F, float *m, int *pred, float *picked, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(xplanes && yplanes && sv && lab && L && F && m && picked, "match_train_forward: null pointer");
  UNOPOSE_REQUIRE(B >= 0 && B <= 65535 && R >= 2 && C >= 2 && Rp >= R && Cp >= C && Rp % MT_PAD == 0 && Cp % MT_PAD == 0,
                  "match_train_forward: bad sizes (B=%d R=%d Rp=%d C=%d Cp=%d)", B, R, Rp, C, Cp);
  UNOPOSE_REQUIRE((long)B * cdiv(R - 1, MT_ROWS) <= 0x7FFFFFFFL, "match_train_forward: too many workgroups");
  if (B == 0) return UNOPOSE_OK;
  const u16 *X = (const u16 *)xplanes, *Y = (const u16 *)yplanes;
  const size_t px = (size_t)B * Rp * MT_D, py = (size_t)B * Cp * MT_D;
  hipLaunchKernelGGL(match_fwd_kernel, dim3(cdiv(R - 1, MT_ROWS) * B), dim3(256), 0, (hipStream_t)stream, X, X + px, Y, Y + py, R, Rp, C, Cp, tau,
                     sv, lab, L, F, m, pred, picked);
  return check_launch("match_train_forward");
}

int unopose_match_train_backward(const void *xplanes, const void *yplanes, int B, int R, int Rp, int C, int Cp, float tau, const float *Lr,
                                 const float *Fr, const float *mr, const float *gr, const float *sr, const int *labr, const float *Lc,
                                 const float *Fc, const float *mc, const float *gc, const float *sc, const int *labc, const float *gL,
                                 float *dX, float *dsr, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(xplanes && yplanes && Lr && Fr && mr && gr && sr && labr && Lc && Fc && mc && gc && sc && labc && gL && dX && dsr,
                  "match_train_backward: null pointer");
  UNOPOSE_REQUIRE(B >= 0 && B <= 65535 && R >= 2 && C >= 2 && Rp >= R && Cp >= C && Rp % MT_PAD == 0 && Cp % MT_PAD == 0,
                  "match_train_backward: bad sizes (B=%d R=%d Rp=%d C=%d Cp=%d)", B, R, Rp, C, Cp);
  UNOPOSE_REQUIRE((long)B * cdiv(R, MT_ROWS) <= 0x7FFFFFFFL, "match_train_backward: too many workgroups");
  if (B == 0) return UNOPOSE_OK;
  static bool optin[64];
  const int rc = lds_optin(optin, (const void *)match_bwd_kernel, MT_BWD_LDS, "match_train_backward");
  if (rc != UNOPOSE_OK) return rc;
  const u16 *X = (const u16 *)xplanes, *Y = (const u16 *)yplanes;
  const size_t px = (size_t)B * Rp * MT_D, py = (size_t)B * Cp * MT_D;
  hipLaunchKernelGGL(match_bwd_kernel, dim3(cdiv(R, MT_ROWS) * B), dim3(256), MT_BWD_LDS, (hipStream_t)stream, X, X + px, Y, Y + py, Y + 2 * py,
                     Y + 3 * py, R, Rp, C, Cp, tau, Lr, Fr, mr, gr, sr, labr, Lc, Fc, mc, gc, sc, labc, gL, dX, dsr);
  return check_launch("match_train_backward");
}

}  // extern "C"
