// DINOv2 ViT patch attention on fp32-class data for gfx950 (C ABI part 2): the reference's default precision
// (configs/main_cfg.py:87-89, no autocast; timm Attention core at core/unopose/model/oneref_feature_extraction.py:38-41).
//
// Input AND output are in the SPLIT layout of csrc/gemm_f32.hip (per token and 32-channel block one 128-byte line
// [hi (32 bf16) | lo (32 bf16)], x = hi + lo to 2^-17): the qkv GEMM writes it in its epilogue and the projection GEMM reads it, so
// this kernel never sees fp32 data and never splits an operand itself -- round 3's kernel (attn_f32.hip) read fp32 qkv and every one
// of the 11 workgroups of an (image, head) re-split the whole K / V on its way into LDS, V^T through 2-byte LDS stores.
// Structure: 12 waves x 32 queries per workgroup (3 waves per SIMD); K / V of a 128-key chunk (hi and lo planes, 65 KiB) arrive in
// double-buffered LDS by LDS-DMA (`buffer_load_dwordx4 ... lds`, 64 pieces of 1 KiB per chunk, per-lane source addresses pick the planes
// apart; the K rows are XOR-swizzled on the SOURCE address, the V image is the [sub-tile][key][16 channels] form ds_read_b64_tr_b16
// wants) -- no staging registers, no LDS stores, one counted wait + barrier per chunk; S^T = K Q^T with the operands swapped so that a
// lane holds 16 keys of ONE query, deferred reference point + end-of-tile fix-up (vit_attn_common.h), P from registers (split into hi / lo
// there), three MFMAs per product (hi.hi + hi.lo + lo.hi, fp32 accumulation) in both contractions.
// Round 4: 1293 us (8 waves, register-staged chunks) -> 1086 us at 64 images x 12 heads x 1374 tokens, same box.
#include "vit_attn_common.h"

namespace unopose {

// a chunk buffer: K hi | K lo (swizzled planes, VA_KPLANEB each) | V hi | V lo (V images, VA_VIMGB each)
constexpr int VS_VOFF = 2 * VA_KPLANEB;
constexpr int VS_BUFB = 2 * VA_KPLANEB + 2 * VA_VIMGB;  // 66560 B
constexpr int VS_NW = 12;  // wavefronts per workgroup = 3 per SIMD (154 VGPRs); 8: 1189 us, 12: 1086 us at 64 x 12 x 1374

// qkv_s: (B, T) token rows of 3 * H * 64 values in the split layout (3 * H * 256 bytes per token: q blocks | k blocks | v blocks,
// head h = blocks 2h, 2h + 1 of each third); out_s: (B, T) rows of H * 64 values in the split layout.
template <int NW>
__global__ __launch_bounds__(NW * 64, 1) void vit_attn_f32s_kernel(const char *__restrict__ qkv_s, int T, int H, int BH, int nq, float scale_log2e,
                                                                   char *__restrict__ out_s) {
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  float (*Ot)[32][68] = reinterpret_cast<float (*)[32][68]>(smem);
  static_assert(NW * 32 * 68 * 4 <= 2 * VS_BUFB, "output staging must fit the chunk buffers");
  constexpr int NT = NW * 64;
  static_assert(NT == 384 || NT == 512 || NT == 768 || NT == 1024, "6, 8, 12 or 16 wavefronts per workgroup");
  int bh, qblk;
  if (!va_block(nq, BH, bh, qblk)) return;
  const int b = bh / H, h = bh % H;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q0 = (qblk * NW + wave) * 32;
  const bool active = q0 < T;  // inactive waves still help staging and hit every barrier
  const int col = lane & 31, hb = lane >> 5;
  const size_t RB = (size_t)3 * H * 256;  // bytes per token row
  const char *base = qkv_s + (size_t)b * T * RB;
  const int qoff = h * 256, koff = (H + h) * 256, voff = (2 * H + h) * 256;  // the head's 2 blocks = 256 contiguous bytes [hi0 lo0 hi1 lo1]
  // ---- LDS-DMA staging: per chunk 32 pieces of K (2 planes x 16 groups of 8 key rows) and 32 of V (2 planes x 4 sub-tiles x 4 groups of
  //      32 keys), 1 KiB each; wave w issues K pieces 4w .. 4w + 3 and V pieces 4w .. 4w + 3.  Rows past the image arrive as zeros.
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char *)smem;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)base, 0, (int)((size_t)T * RB), 0x00020000);
  constexpr int NPC = VA_CHUNK / 4, KP = VA_CHUNK / 8, VG = VA_CHUNK / 32;  // pieces of K (and of V) per chunk; K pieces / V key groups per plane
  constexpr int NP = (NPC + NW - 1) / NW;  // pieces of K (and of V) per wave: piece ids wave, wave + NW, ... < NPC
  uint32_t kvo[NP], vvo[NP], kdst[NP], vdst[NP];
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int kp = min(wave + i * NW, NPC - 1), p = kp / KP, rg = kp % KP;
    const int krow = 8 * rg + (lane >> 3), gch = va_kswz(lane & 7, krow);
    kvo[i] = (uint32_t)(krow * (int)RB + koff + (gch >> 2) * 128 + (gch & 3) * 16 + p * 64);
    kdst[i] = (uint32_t)(p * VA_KPLANEB + rg * 1024);
    const int pv = kp / (4 * VG), sub = (kp / VG) & 3, kq = kp % VG, vkey = 32 * kq + (lane >> 1), ch = sub * 16 + (lane & 1) * 8;
    vvo[i] = (uint32_t)(vkey * (int)RB + voff + (ch >> 5) * 128 + (ch & 31) * 2 + pv * 64);
    vdst[i] = (uint32_t)(VS_VOFF + pv * VA_VIMGB + sub * VA_VSUBB + kq * 1024);
  }
  auto issue_chunk = [&](int c, int bslot) {
    const uint32_t b0 = lds0 + bslot * VS_BUFB, ro = (uint32_t)(c * VA_CHUNK) * (uint32_t)RB;
#pragma unroll
    for (int i = 0; i < NP; ++i)
      if (wave + i * NW < NPC) gemm_dma16(b0 + kdst[i], kvo[i] + ro, rs, 0);  // (wave-uniform)
#pragma unroll
    for (int i = 0; i < NP; ++i)
      if (wave + i * NW < NPC) gemm_dma16(b0 + vdst[i], vvo[i] + ro, rs, 0);
  };
  const int nchunks = (T + VA_CHUNK - 1) / VA_CHUNK;
  issue_chunk(0, 0);
  bf16x8_hl qf[4];
  {
    const char *qp = base + (size_t)min(q0 + col, T - 1) * RB + qoff;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int c = ks * 16 + hb * 8;  // channels c .. c + 7
      const char *p = qp + (c >> 5) * 128 + (c & 31) * 2;
      qf[ks].hi = *reinterpret_cast<const bf16x8 *>(p);
      qf[ks].lo = *reinterpret_cast<const bf16x8 *>(p + 64);
    }
  }
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) asm volatile("" : "+v"(qf[ks].hi), "+v"(qf[ks].lo));  // the Q loads are complete HERE (see va_wave_init)
  f32x16 o[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[t][r] = 0.f;
  float m_run = -3e38f, l_run = 0.f;

  const uint32_t vlane_off = (uint32_t)(VS_VOFF + va_vlane_off(lane));
  uint32_t kfo[4];
  va_koff(col, hb, kfo);

  auto qk_tile = [&](const char *buf, int c0, int kt, bool partial, f32x16 &s) {
    // S^T = K Q^T: rows = 32 keys, cols = 32 queries
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
    // all eight K fragments first, then the twelve MFMAs (the compiler otherwise reads every k-step's pair right in front of its MFMAs:
    // four exposed LDS round trips instead of one)
    bf16x8_hl kf[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const char *kp = buf + kt * VA_KROWB + kfo[ks];
      kf[ks].hi = *reinterpret_cast<const bf16x8 *>(kp);
      kf[ks].lo = *reinterpret_cast<const bf16x8 *>(kp + VA_KPLANEB);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) s = mfma3_lh_hl_hh_32x32(kf[ks], qf[ks], s);
    if (partial) {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (c0 + kt + va_row(r) + 4 * hb >= T) s[r] = -3e38f;
    }
  };
  auto softmax_pv_tile = [&](const char *buf, int kt, f32x16 &s) {
    // the tile's V fragments are read before the softmax arithmetic (measured: each read in front of its MFMAs 1101 us, all fragments of a
    // product before its MFMAs 1086 us, the V fragments before the softmax 1079 us)
    const char *vt = buf + vlane_off + kt * VA_VROWB;
    bf16x8_hl vfe[2][2];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
      for (int t = 0; t < 2; ++t) vfe[s2][t] = va_v_frag_hl(vt, s2, t);
    __builtin_amdgcn_sched_barrier(0);
    // online softmax with the deferred reference point: per-lane select, no branch before the P.V MFMAs
    float alpha;
    const bool grow = va_softmax(s, m_run, l_run, scale_log2e, alpha);
    // P = hi + lo, packed as the B operand of the two 16-key k-steps
    bf16x8_hl pf[2];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      float pv[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) pv[e] = s[s2 * 8 + e];
      pf[s2] = split8_bf16(pv);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
      for (int t = 0; t < 2; ++t) o[t] = mfma3_lh_hl_hh_32x32(vfe[s2][t], pf[s2], o[t]);
    if (__builtin_expect(__any(grow), 0)) {  // rare after the first tile: O = (O - D) alpha + D with D = this tile's P.V
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        f32x16 d;
#pragma unroll
        for (int r = 0; r < 16; ++r) d[r] = 0.f;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) d = mfma3_lh_hl_hh_32x32(va_v_frag_hl(vt, s2, t), pf[s2], d);
        va_rereference(o[t], d, alpha);
      }
    }
  };

  va_dma_chunks(nchunks, issue_chunk, [&](int c) {
    if (!active) return;
    const int c0 = c * VA_CHUNK, nk = min(VA_CHUNK, T - c0);
    const char *buf = smem + (c & 1) * VS_BUFB;
    const int nt = (nk + 31) >> 5;  // tiles of this chunk; only the sequence's last one can be partial
    // (measured and not kept: the score MFMAs of tile t + 1 issued before the softmax of tile t -- slower at 3 waves / SIMD)
    for (int t = 0; t < nt; ++t) {
      f32x16 s;
      qk_tile(buf, c0, t * 32, (t + 1) * 32 > nk, s);
      softmax_pv_tile(buf, t * 32, s);
    }
  });
  if (!active) return;
  // ---- normalise, transpose through LDS, store token rows in the split layout
  const float inv = 1.f / l_run;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) Ot[wave][col][t * 32 + va_row(r) + 4 * hb] = o[t][r] * inv;
  wave_lds_handover();
  const size_t ORB = (size_t)H * 256;
  va_store_split(Ot[wave], out_s + ((size_t)b * T + q0) * ORB + h * 256, ORB, T - q0, lane);
}

}  // namespace unopose

using namespace unopose;

extern "C" {

int unopose_vit_attention_f32_ss(const void *qkv_split, int B, int T, int H, void *out_split, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(qkv_split && out_split, "vit_attention_f32_ss: null pointer");
  UNOPOSE_REQUIRE(B >= 0 && T >= 1 && H >= 1 && (long)B * H * cdiv(T, 256) < (1L << 28), "vit_attention_f32_ss: bad sizes");
  if (B == 0) return UNOPOSE_OK;
  return va_launch<&vit_attn_f32s_kernel<VS_NW>, char, VS_NW, 32>("vit_attention_f32_ss", (size_t)2 * VS_BUFB, qkv_split, B, T, H, out_split,
                                                                 (hipStream_t)stream);
}

}  // extern "C"
