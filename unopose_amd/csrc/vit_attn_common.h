// What the ViT patch attention kernels share (vit_attn.hip: vit_attn_kernel<QB, NBUF, NW> and vit_attn_kernel_dma<NW>; vit_attn_f32s.hip:
// vit_attn_f32s_kernel<NW>; attn_f32.hip: the split-layout store of vit_attn_f32_kernel<true>): the chunk and V-image geometry, the workgroup
// mapping, every stage of a 32-key tile, the output stages, the LDS-DMA chunk loop and the launcher.  A kernel keeps only what is its own:
// how K / V reach LDS and how a K fragment is addressed.
#pragma once
#include "common.h"
#include "gemm_common.h"

namespace unopose {

typedef short s16x4 __attribute__((ext_vector_type(4)));

constexpr int VA_CHUNK = 128;    // keys staged per LDS chunk
constexpr float VA_DEFER = 8.f;  // log2 of the largest P the deferred rescale lets through
// V chunk image (one per bf16 plane), in bytes: 4 sub-tiles [128 keys][16 channels] (row = 32 B), sub-tile stride 4224 B.  Read with the
// gfx950 transpose read ds_read_b64_tr_b16: a 16-lane group fetches a [4 keys][16 channels] block (128 contiguous bytes = 32 banks) and
// lane c receives the 4 keys of channel c -- the A fragment of V^T without ever transposing V in LDS.  Lanes 16-31 read the next
// sub-tile, 4224 B = 32 banks further on.
constexpr int VA_VROWB = 32;                            // one key row of a sub-tile
constexpr int VA_VSUBB = VA_CHUNK * VA_VROWB + 128;     // sub-tile stride (4096 B + 128 B bank skew)
constexpr int VA_VIMGB = 4 * VA_VSUBB;                  // the whole image
// this lane's slot in the transpose read: sub-tile (lane>>4)&1, key row 4 hb + ((lane&15)>>2), 8-byte chunk lane&3
__device__ __forceinline__ int va_vlane_off(int lane) {
  return ((lane >> 4) & 1) * VA_VSUBB + (4 * (lane >> 5) + ((lane & 15) >> 2)) * VA_VROWB + (lane & 3) * 8;
}
// K chunk of the LDS-DMA kernels: [key][64 channels] bf16 rows of 128 B without padding, 16-byte chunk c of row r at c ^ ((r >> 1) & 7)
// (conflict-free ds_read_b128; the DMA applies the swizzle on its SOURCE address).  The register-staged kernel pads its rows instead.
constexpr int VA_KROWB = 128;
constexpr int VA_KPLANEB = VA_CHUNK * VA_KROWB;
__device__ __forceinline__ int va_kswz(int chunk, int row) { return chunk ^ ((row >> 1) & 7); }
// K fragment of key row kt + col (kt a multiple of 32), k-step ks: 16-byte chunk 2 ks + hb, swizzled by the row
__device__ __forceinline__ void va_koff(int col, int hb, uint32_t (&koff)[4]) {
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) koff[ks] = (uint32_t)(col * VA_KROWB + (va_kswz(2 * ks + hb, col) << 4));
}
// key (score tile) or channel (output tile) of accumulator register r in the 32x32 C/D layout, for the lanes of half 0; + 4 hb, added
// last so that it stays the variable part of an address
__device__ __forceinline__ int va_row(int r) { return (r & 3) + 8 * (r >> 2); }

// Workgroup -> (image, head, query block): the linear id is dealt round-robin over the 8 XCDs by the dispatcher, so id%8 picks the XCD
// and all query blocks of one (image, head) are given the same id%8: its K / V are then fetched into ONE XCD's L2 instead of every L2.
// false: a workgroup of the padding past the last (image, head).
__device__ __forceinline__ bool va_block(int nq, int BH, int &bh, int &qblk) {
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  bh = (slot / nq) * 8 + xcd;
  qblk = slot % nq;
  return bh < BH;
}
inline long va_block_count(int BH, int nq) { return (long)cdiv(BH, 8) * nq * 8; }

// Online softmax of one 32-key score tile of one query block (a lane holds 16 keys of ONE query; the other 16 are in lane ^ 32).
//  * Deferred reference point: a query's reference m_run moves only when its tile maximum exceeds it by more than 2^VA_DEFER; until then
//    P = exp2(s - m_run) may reach 2^VA_DEFER instead of 1 -- harmless in the fp32 accumulators, bf16 rounds P with the same RELATIVE error
//    at any magnitude, and O / l does not depend on the reference point.  The choice is a per-lane select, not a branch.
//  * l is kept exact branch-free: l = l * alpha + sum(P) with alpha = exp2(m_old - m_new) (= 1 if unmoved).
// s becomes P; returns whether this query's reference moved.
__device__ __forceinline__ bool va_softmax(f32x16 &s, float &m_run, float &l_run, float scale_log2e, float &alpha) {
  float mx = s[0];
#pragma unroll
  for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s[r]);
  const auto sm = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
  mx = fmaxf(__uint_as_float(sm[0]), __uint_as_float(sm[1])) * scale_log2e;  // scale > 0: max commutes with it
  const bool grow = mx > m_run + VA_DEFER;
  const float m_use = grow ? mx : m_run;
  alpha = __builtin_amdgcn_exp2f(m_run - m_use);
  m_run = m_use;
  float ls = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    s[r] = __builtin_amdgcn_exp2f(fmaf(s[r], scale_log2e, -m_use));
    ls += s[r];
  }
  const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(ls), __float_as_uint(ls), false, false);
  l_run = fmaf(l_run, alpha, __uint_as_float(sw[0]) + __uint_as_float(sw[1]));
  return grow;
}

// A fragment of V^T for k-step s2 (= accumulator registers 8*s2 .. 8*s2+7 of S, a permuted key order that these reads follow) and channel
// half t: row = channel t*32 + col, keys kt + 16 s2 + 4 hb + {0..3}, + 8.  vt = chunk buffer + V image + va_vlane_off + kt * VA_VROWB.
__device__ __forceinline__ bf16x8 va_v_frag(const char *vt, int s2, int t) {
  const char *vp = vt + t * 2 * VA_VSUBB + s2 * 16 * VA_VROWB;
  union { bf16x8 v; s16x4 h4[2]; } vf;
  vf.h4[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3))) *)(vp));
  vf.h4[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3))) *)(vp + 8 * VA_VROWB));
  return vf.v;
}
// the same from a hi image and the lo image VA_VIMGB behind it
__device__ __forceinline__ bf16x8_hl va_v_frag_hl(const char *vt, int s2, int t) {
  return bf16x8_hl{va_v_frag(vt, s2, t), va_v_frag(vt + VA_VIMGB, s2, t)};
}

// End-of-tile fix-up of an accumulator whose query moved its reference: O was accumulated as if alpha were 1; with D = this tile's P.V,
// O = (O - D) * alpha + D.  (O - D) is the old accumulator up to one rounding of the much larger new terms, and it is scaled by
// alpha <= 2^-VA_DEFER (or by 0 on the first tile, where O - D is exactly 0).
__device__ __forceinline__ void va_rereference(f32x16 &o, const f32x16 &d, float alpha) {
#pragma unroll
  for (int r = 0; r < 16; ++r) o[r] = fmaf(o[r] - d[r], alpha, d[r]);
}

union VaP {  // P of one 16-key k-step, packed as the B operand
  bf16x8 v;
  uint32_t w[4];
};

// O^T += V^T P^T for the QB query blocks of a wave; if ANY query of the wave moved (first tile, then rare) the fix-up recomputes this
// tile's P.V into a scratch accumulator D and re-references the accumulators.
template <int QB>
__device__ __forceinline__ void va_pv(const char *vt, const VaP (&pf)[QB][2], f32x16 (&o)[QB][2], const float (&alpha)[QB], bool moved) {
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const bf16x8 vf = va_v_frag(vt, s2, t);
#pragma unroll
      for (int qb = 0; qb < QB; ++qb) o[qb][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf[qb][s2].v, o[qb][t], 0, 0, 0);
    }
  if (__builtin_expect(__any(moved), 0)) {  // rare after the first tile: re-reference the accumulators of the queries that moved
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const bf16x8 v0 = va_v_frag(vt, 0, t), v1 = va_v_frag(vt, 1, t);
#pragma unroll
      for (int qb = 0; qb < QB; ++qb) {
        f32x16 d;
#pragma unroll
        for (int r = 0; r < 16; ++r) d[r] = 0.f;
        d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(v0, pf[qb][0].v, d, 0, 0, 0);
        d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(v1, pf[qb][1].v, d, 0, 0, 0);
        va_rereference(o[qb][t], d, alpha[qb]);
      }
    }
  }
}

// ---- the bf16 kernels: a wave's QB blocks of 32 queries ----------------------------------------------------------------------------
template <int QB>
struct VaWave {
  bf16x8 qf[QB][4];  // Q fragments (B operand of S^T = K Q^T)
  f32x16 o[QB][2];   // O^T, two 32-channel halves
  float m_run[QB], l_run[QB];  // running max in the exp2 domain (score * scale * log2 e) and running sum
};

// base: the image's token rows of C3 = 3 H 64 bf16; the wave's queries are q0 + 32 qb + col, clamped to the sequence
template <int QB>
__device__ __forceinline__ void va_wave_init(VaWave<QB> &w, const u16 *base, int C3, int h, int q0, int col, int hb, int T) {
#pragma unroll
  for (int qb = 0; qb < QB; ++qb) {
    const int tq = min(q0 + qb * 32 + col, T - 1);
    const u16 *qp = base + (size_t)tq * C3 + h * 64 + hb * 8;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) w.qf[qb][ks] = *reinterpret_cast<const bf16x8 *>(qp + ks * 16);
  }
  // Pin the Q loads as complete HERE: otherwise the compiler waits for them with vmcnt(0) at their first
  // use inside the tile loop, which also drains the K / V chunk prefetch issued in the meantime.
#pragma unroll
  for (int qb = 0; qb < QB; ++qb)
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) asm volatile("" : "+v"(w.qf[qb][ks]));
#pragma unroll
  for (int qb = 0; qb < QB; ++qb) {
    w.m_run[qb] = -3e38f;
    w.l_run[qb] = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) w.o[qb][t][r] = 0.f;
  }
}

// One 32-key tile: S^T = K Q^T (rows = 32 keys, cols = 32 queries, for every query block of the wave) -> tail mask -> softmax -> pack P
// -> P.V, written so that the COMMON path is one basic block from the score MFMAs to the P.V MFMAs (a wave-uniform rescale branch in the
// middle of the tile cost 1/3 of the kernel by ablation: it splits the block the scheduler interleaves MFMA, exp and VALU work in).
// kf[ks]: the K fragment of key row (tile's first key) + col, k-step ks, read by the kernel; k0: the tile's first key in the sequence.
// (The fragments come as values, the mask is spelled out here: with a fragment functor or a mask helper the compiler serialised the K
// reads of vit_attn_kernel_dma's full tiles behind lgkmcnt(0) waits.)
template <int QB>
__device__ __forceinline__ void va_tile(VaWave<QB> &w, const bf16x8 (&kf)[4], const char *vt, int k0, bool partial, int hb, int T, float scale_log2e) {
  f32x16 s[QB];
#pragma unroll
  for (int qb = 0; qb < QB; ++qb)
#pragma unroll
    for (int r = 0; r < 16; ++r) s[qb][r] = 0.f;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks)
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) s[qb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[ks], w.qf[qb][ks], s[qb], 0, 0, 0);
  if (partial) {  // the one partial tile of the sequence: keys >= T are masked out
#pragma unroll
    for (int qb = 0; qb < QB; ++qb)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (k0 + va_row(r) + 4 * hb >= T) s[qb][r] = -3e38f;
  }
  VaP pf[QB][2];
  float alpha[QB];
  bool moved = false;
#pragma unroll
  for (int qb = 0; qb < QB; ++qb) {
    moved |= va_softmax(s[qb], w.m_run[qb], w.l_run[qb], scale_log2e, alpha[qb]);
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
      for (int e = 0; e < 4; ++e) pf[qb][s2].w[e] = cvt_pk_bf16_f32(s[qb][s2 * 8 + 2 * e], s[qb][s2 * 8 + 2 * e + 1]);
  }
  va_pv<QB>(vt, pf, w.o, alpha, moved);
}

// normalise, transpose through the wave's 32 x 72 u16 of LDS, store token rows (out: (B, T, H*64) bf16)
template <int QB>
__device__ __forceinline__ void va_store_bf16(const VaWave<QB> &w, u16 (*Otw)[72], u16 *out, int b, int h, int H, int q0, int lane, int col, int hb,
                                              int T) {
#pragma unroll
  for (int qb = 0; qb < QB; ++qb) {
    const float inv = 1.f / w.l_run[qb];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) Otw[col][t * 32 + va_row(r) + 4 * hb] = f2bf(w.o[qb][t][r] * inv);
    wave_lds_handover();
    // 32 rows x 128 B: each lane moves 16 B; 8 lanes cover one row
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int row = it * 8 + (lane >> 3), seg = lane & 7;
      const int tq = q0 + qb * 32 + row;
      if (tq < T) {
        const uint4 v = *reinterpret_cast<const uint4 *>(&Otw[row][seg * 8]);
        *reinterpret_cast<uint4 *>(out + ((size_t)b * T + tq) * (H * 64) + h * 64 + seg * 8) = v;
      }
    }
    wave_lds_handover();
  }
}

// A wave's 32 x 64 fp32 output tile (32 x 68 floats of LDS) -> token rows in the split layout of gemm_f32.hip (per token and 32-channel
// block one 128-byte line [hi (32 bf16) | lo (32 bf16)]): 16 lanes per row, 4 channels each -> 8 bytes of hi and 8 bytes of lo.
// rows: the head's 256 bytes in the wave's first token row; rowb: bytes per token row; nrows: rows of the tile inside the sequence.
__device__ __forceinline__ void va_store_split(const float (*Otw)[68], char *rows, size_t rowb, int nrows, int lane) {
#pragma unroll
  for (int it = 0; it < 8; ++it) {
    const int row = it * 4 + (lane >> 4), seg = lane & 15;
    if (row < nrows) {
      const float4 v = *reinterpret_cast<const float4 *>(&Otw[row][seg * 4]);
      uint2 hi, lo;
      hi.x = cvt_pk_bf16_f32(v.x, v.y);
      hi.y = cvt_pk_bf16_f32(v.z, v.w);
      lo.x = cvt_pk_bf16_lo(v.x, v.y, hi.x);
      lo.y = cvt_pk_bf16_lo(v.z, v.w, hi.y);
      const int c = seg * 4;  // channel inside the head
      char *line = rows + row * rowb + (c >> 5) * 128 + (c & 31) * 2;
      *reinterpret_cast<uint2 *>(line) = hi;
      *reinterpret_cast<uint2 *>(line + 64) = lo;
    }
  }
}

// The chunk loop of the LDS-DMA kernels over two buffers; chunk 0 has been issued into buffer 0.  issue(c, slot): this wave's pieces of
// chunk c into buffer `slot`; compute(c): the wave's tiles against chunk c in buffer c & 1.  One counted wait + barrier per chunk.
template <class Issue, class Compute>
__device__ __forceinline__ void va_dma_chunks(int nchunks, Issue issue, Compute compute) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // chunk 0 landed; every wave's pieces visible after the barrier
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  for (int c = 0; c < nchunks; ++c) {
    if (c + 1 < nchunks) issue(c + 1, (c + 1) & 1);  // (that buffer was last read in chunk c - 1, before the barrier that ended it)
    compute(c);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  }
}

// One launch of KERNEL(qkv, T, H, BH, nq, scale * log2 e, out) with NW wavefronts of QW queries each per workgroup and `lds` bytes of
// dynamic LDS; `name`: the entry point, for the error texts.
template <auto KERNEL, typename E, int NW, int QW>
static int va_launch(const char *name, size_t lds, const void *qkv, int B, int T, int H, void *out, hipStream_t stream) {
  static bool opt[64];  // > 64 KiB of LDS needs the opt-in, per device (idempotent; benign if raced)
  if (lds_optin(opt, reinterpret_cast<const void *>(KERNEL), lds, name) != UNOPOSE_OK) return UNOPOSE_ELAUNCH;
  const int BH = B * H, nq = cdiv(T, QW * NW);
  const float scale_log2e = 0.125f * 1.4426950408889634f;  // 1/sqrt(64) * log2(e)
  hipLaunchKernelGGL(KERNEL, dim3((unsigned)va_block_count(BH, nq)), dim3(NW * 64), lds, stream, (const E *)qkv, T, H, BH, nq, scale_log2e,
                     (E *)out);
  return check_launch(name);
}

}  // namespace unopose
