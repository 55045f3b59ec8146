// DINOv2 ViT patch attention for gfx950 (C ABI part 2).
//
// Replaces timm's Attention core, softmax(q k^T / sqrt(64)) v per head, that the reference drives at
// core/unopose/model/oneref_feature_extraction.py:38-41 (12 heads x 64, T = 5 + (S/14)^2 tokens).
// Flash-style: the T x T score matrix never exists in memory.  One wavefront owns 32 query tokens of one
// (image, head) and walks the keys in tiles of 32 with an online softmax:
//   * S^T = K Q^T on v_mfma_f32_32x32x16_bf16 ("swapped" product): in the C/D layout a lane then holds
//     16 keys of ONE query, so the softmax reductions are in-register plus one cross-half exchange;
//   * O^T += V^T P^T with P fed straight from those registers: accumulator registers 8s..8s+7 are one
//     16-key MFMA k-step in a fixed permuted key order, and V^T (transposed on its way into LDS) is
//     read in the same order, so P never moves between lanes;
//   * K / V of a 128-key chunk are staged once per workgroup in LDS and shared by its 4 waves;
//   * O^T is transposed through 4 KiB of LDS so every token row is stored as 128 contiguous bytes.
// The stages of a tile, the V image, the workgroup mapping, the output pass and the launcher are vit_attn_common.h's; the two kernels
// here differ in how K / V reach LDS and in how a K fragment is addressed.
#include "vit_attn_common.h"

namespace unopose {

constexpr int VA_LDK = 64 + 8;                         // padded row of the K chunk  [key][channel], u16
constexpr int VA_KPADB = VA_CHUNK * VA_LDK * 2;        // bytes of the padded K chunk; the V image follows it
constexpr int VA_BUF = (VA_KPADB + VA_VIMGB) / 2;      // u16 per chunk buffer (K rows + V image)

// qkv: (B, T, 3, H, 64) bf16 (the fused qkv Linear output); out: (B, T, H*64) bf16.
// The 4 waves of a workgroup share one (image, head): K and V of a 128-key chunk are loaded once with
// coalesced 16-byte reads, K kept row-major and V transposed on the way into LDS (so the caller needs no
// V^T copy), then every wave runs its 32 queries against the chunk.

// QB = 32-query blocks per wave (a workgroup owns 128 QB queries of one (image, head)); NBUF = LDS chunk
// buffers.  QB = 2 reads every K / V fragment once for two independent score tiles -- half the LDS traffic
// per MFMA and two dependency chains per wave for the scheduler to interleave (QK^T of one block under
// the softmax VALU work of the other); it takes ~2x the registers, so it runs 2 waves/SIMD with a
// double-buffered chunk (one barrier per chunk).  QB = 1 keeps short sequences (T = 261) from wasting
// half-empty workgroups.
// NW = wavefronts per workgroup: the K / V chunk staged in LDS is shared by NW * 32 QB queries, so a
// larger workgroup amortises the staging (global loads, LDS writes, barriers: ~1/3 of the kernel at NW = 4
// by ablation) over twice the MFMA work.
template <int QB, int NBUF, int NW>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(QB == 1 ? 3 : 2, QB == 1 ? 4 : 2))) void vit_attn_kernel(const u16 *__restrict__ qkv, int T, int H, int BH, int nq,
                                                       float scale_log2e, u16 *__restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) u16 smem[];
  u16 (*Ot)[32][72] = reinterpret_cast<u16 (*)[32][72]>(smem);
  static_assert(NW * 32 * 72 <= NBUF * VA_BUF, "output staging must fit the chunk buffers");
  constexpr int NT = NW * 64;  // threads
  int bh, qblk;
  if (!va_block(nq, BH, bh, qblk)) return;
  const int b = bh / H, h = bh % H;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q0 = (qblk * NW + wave) * (32 * QB);
  const bool active = q0 < T;  // inactive waves still help staging and hit every barrier
  const int col = lane & 31, hb = lane >> 5;
  const int C3 = 3 * H * 64;
  const u16 *base = qkv + (size_t)b * T * C3;
  VaWave<QB> w;
  va_wave_init(w, base, C3, h, q0, col, hb, T);

  // register-staged prefetch of a chunk: 128 keys x 128 B of K and of V.
  //   K: 8 lanes per key row (contiguous 128 B; the 16-byte LDS stores of 8 lanes cover all 32 banks)
  //   V: 8 lanes = 4 keys x the two 16-byte halves of one 16-channel sub-tile row (same property)
  // (named registers, not arrays: an array captured by the lambdas below ends up in scratch)
  uint4 pk0, pk1, pk2, pk3, pv0, pv1, pv2, pv3;
#define VA_LOAD(i, PK, PV)                                                                                       \
  {                                                                                                              \
    const int e = tid + i * NT, key = e >> 3, c8 = e & 7;                                                        \
    PK = *reinterpret_cast<const uint4 *>(base + (size_t)min(c0 + key, T - 1) * C3 + H * 64 + h * 64 + c8 * 8);  \
    const int vkey = (e >> 5) * 4 + ((e >> 1) & 3), vc = ((e >> 3) & 3) * 16 + (e & 1) * 8;                      \
    PV = *reinterpret_cast<const uint4 *>(base + (size_t)min(c0 + vkey, T - 1) * C3 + 2 * H * 64 + h * 64 + vc); \
  }
#define VA_STORE(i, PK, PV)                                                                             \
  {                                                                                                     \
    const int e = tid + i * NT, key = e >> 3, c8 = e & 7;                                               \
    *reinterpret_cast<uint4 *>(buf + key * VA_LDK + c8 * 8) = PK;                                       \
    const int vkey = (e >> 5) * 4 + ((e >> 1) & 3);                                                     \
    /* keys beyond T contribute V = 0 (their P is 0 as well) */                                         \
    *reinterpret_cast<uint4 *>(reinterpret_cast<char *>(buf) + VA_KPADB + ((e >> 3) & 3) * VA_VSUBB + vkey * VA_VROWB + (e & 1) * 16) = \
        c0 + vkey < T ? PV : make_uint4(0u, 0u, 0u, 0u);                                                \
  }
  // 1024 16-byte pieces of K and of V per chunk: 1024 / NT per thread
  auto chunk_load = [&](int c0) {
    VA_LOAD(0, pk0, pv0) VA_LOAD(1, pk1, pv1)
    if (NT == 256) { VA_LOAD(2, pk2, pv2) VA_LOAD(3, pk3, pv3) }
  };
  auto chunk_store = [&](int c0, u16 *buf) {
    VA_STORE(0, pk0, pv0) VA_STORE(1, pk1, pv1)
    if (NT == 256) { VA_STORE(2, pk2, pv2) VA_STORE(3, pk3, pv3) }
  };
  static_assert(NT == 256 || NT == 512, "4 or 8 wavefronts per workgroup");
#undef VA_LOAD
#undef VA_STORE
  const int vlane_off = VA_KPADB + va_vlane_off(lane);

  auto chunk_compute = [&](int c0, const u16 *buf) {
    const int nk = min(VA_CHUNK, T - c0);  // valid keys of this chunk
    auto tile = [&](int kt, bool partial) {
      bf16x8 kf[4];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) kf[ks] = *reinterpret_cast<const bf16x8 *>(buf + (kt + col) * VA_LDK + ks * 16 + hb * 8);
      va_tile(w, kf, reinterpret_cast<const char *>(buf) + vlane_off + kt * VA_VROWB, c0 + kt, partial, hb, T, scale_log2e);
    };
    int kt = 0;
    for (; kt + 32 <= nk; kt += 32) tile(kt, false);  // full tiles: no masking, no branch between the MFMA groups
    if (kt < nk) tile(kt, true);                      // the one partial tile of the sequence
  };

  const int nchunks = (T + VA_CHUNK - 1) / VA_CHUNK;
  if (NBUF == 1) {
    chunk_load(0);
    for (int c = 0; c < nchunks; ++c) {
      __syncthreads();  // previous chunk fully consumed
      chunk_store(c * VA_CHUNK, smem);
      if (c + 1 < nchunks) chunk_load((c + 1) * VA_CHUNK);  // in flight under this chunk's MFMAs
      __syncthreads();
      if (active) chunk_compute(c * VA_CHUNK, smem);
    }
  } else {
    chunk_load(0);
    chunk_store(0, smem);
    if (nchunks > 1) chunk_load(VA_CHUNK);
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
      if (active) chunk_compute(c * VA_CHUNK, smem + (c & 1) * VA_BUF);
      if (c + 1 < nchunks) {  // the other buffer was last read before the previous barrier
        chunk_store((c + 1) * VA_CHUNK, smem + ((c + 1) & 1) * VA_BUF);
        if (c + 2 < nchunks) chunk_load((c + 2) * VA_CHUNK);
      }
      __syncthreads();
    }
  }
  __syncthreads();  // every wave is done with the K / V chunks before they become the output buffer
  if (active) va_store_bf16(w, Ot[wave], out, b, h, H, q0, lane, col, hb, T);
}


// ------------------------------------------------------------------------------------------------------------------------------
// Round 4: the long-sequence form (T >= 1024).  Same arithmetic as vit_attn_kernel<2, ...> above -- 64 queries per wave, swapped
// product, deferred reference point, end-of-tile fix-up -- with two structural changes:
//  * K / V chunks arrive by LDS-DMA (`buffer_load_dwordx4 ... lds`: 32 one-KiB pieces per 128-key chunk; the per-lane source addresses
//    swizzle the K rows (16-byte chunk c of row r at c ^ ((r >> 1) & 7): conflict-free ds_read_b128 without padding) and lay V out as
//    the [sub-tile][key][16 channels] image ds_read_b64_tr_b16 wants -- the SAME image the register-staged kernel writes; keys past the
//    sequence fall outside the buffer descriptor and arrive as zeros): no staging registers (233 -> 213 VGPRs), no ds_write, one counted
//    wait + barrier per chunk;
//  * 4 waves per workgroup and TWO workgroups per CU (66.5 KiB of LDS each): with one 8-wave workgroup per CU the Q loads, the first
//    chunk and the output pass of every workgroup ran with nothing else on the CU -- 9 workgroups per CU and launch, ~10 % of the time.
// Same box, 64 x 12 x 1374: 489.6 us (vit_attn_kernel<2, 2, 8>) -> 472 (8 waves, LDS-DMA, 2 buffers) -> 450-469 us (this kernel);
// a third chunk buffer (one workgroup per CU again): 622 us; results equal to the old kernel's.
constexpr int VD_BUFB = VA_KPLANEB + VA_VIMGB;  // 33 280 B per chunk buffer: swizzled K chunk, V image

template <int NW>
__global__ __launch_bounds__(NW * 64, 2) void vit_attn_kernel_dma(const u16 *__restrict__ qkv, int T, int H, int BH, int nq, float scale_log2e,
                                                               u16 *__restrict__ out) {
  constexpr int QB = 2, NBUF = 2, NPC = 32 / NW;  // NPC: LDS-DMA pieces per wave and chunk, half of them K, half V
  extern __shared__ __attribute__((aligned(1024))) char smemd[];
  u16 (*Ot)[32][72] = reinterpret_cast<u16 (*)[32][72]>(smemd);
  static_assert(NW * 32 * 72 * 2 <= NBUF * VD_BUFB, "output staging must fit the chunk buffers");
  int bh, qblk;
  if (!va_block(nq, BH, bh, qblk)) return;
  const int b = bh / H, h = bh % H;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q0 = (qblk * NW + wave) * (32 * QB);
  const bool active = q0 < T;  // inactive waves still issue their DMA pieces and hit every barrier
  const int col = lane & 31, hb = lane >> 5;
  const int C3 = 3 * H * 64;
  const u16 *base = qkv + (size_t)b * T * C3;
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char *)smemd;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)base, 0, (int)((size_t)T * C3 * 2), 0x00020000);
  uint32_t kvo[NPC / 2], vvo[NPC / 2], kdst[NPC / 2], vdst[NPC / 2];
#pragma unroll
  for (int i = 0; i < NPC / 2; ++i) {
    const int p = (NPC / 2) * wave + i;  // piece 0 .. 15 of K and of V
    const int krow = 8 * p + (lane >> 3), gch = va_kswz(lane & 7, krow);
    kvo[i] = (uint32_t)(krow * C3 * 2 + (H * 64 + h * 64) * 2 + gch * 16);
    kdst[i] = (uint32_t)(p * 1024);
    const int sub = p >> 2, vkey = 32 * (p & 3) + (lane >> 1);
    vvo[i] = (uint32_t)(vkey * C3 * 2 + (2 * H * 64 + h * 64 + sub * 16 + (lane & 1) * 8) * 2);
    vdst[i] = (uint32_t)(VA_KPLANEB + sub * VA_VSUBB + (p & 3) * 1024);
  }
  auto issue_chunk = [&](int c, int bslot) {  // (the key-row offset rides in the VGPR offset: the descriptor's range check covers it)
    const uint32_t b0 = lds0 + bslot * VD_BUFB, ro = (uint32_t)(c * VA_CHUNK) * (uint32_t)(C3 * 2);
#pragma unroll
    for (int i = 0; i < NPC / 2; ++i) gemm_dma16(b0 + kdst[i], kvo[i] + ro, rs, 0);
#pragma unroll
    for (int i = 0; i < NPC / 2; ++i) gemm_dma16(b0 + vdst[i], vvo[i] + ro, rs, 0);
  };
  const int nchunks = (T + VA_CHUNK - 1) / VA_CHUNK;
  issue_chunk(0, 0);

  VaWave<QB> w;
  va_wave_init(w, base, C3, h, q0, col, hb, T);
  uint32_t koff[4];
  va_koff(col, hb, koff);
  const uint32_t vlane_off = (uint32_t)(VA_KPLANEB + va_vlane_off(lane));

  va_dma_chunks(nchunks, issue_chunk, [&](int c) {
    if (!active) return;
    const int c0 = c * VA_CHUNK, nk = min(VA_CHUNK, T - c0);
    const char *buf = smemd + (c & 1) * VD_BUFB;
    auto tile = [&](int kt, bool partial) {
      bf16x8 kf[4];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) kf[ks] = *reinterpret_cast<const bf16x8 *>(buf + kt * VA_KROWB + koff[ks]);
      va_tile(w, kf, buf + vlane_off + kt * VA_VROWB, c0 + kt, partial, hb, T, scale_log2e);
    };
    int kt = 0;
    for (; kt + 32 <= nk; kt += 32) tile(kt, false);
    if (kt < nk) tile(kt, true);
  });
  if (active) va_store_bf16(w, Ot[wave], out, b, h, H, q0, lane, col, hb, T);
}

}  // namespace unopose

using namespace unopose;

// The one place that picks the kernel for a (T, H): 0 = vit_attn_kernel<1, 1, 4>, 1 = <2, 2, 4>, 2 = vit_attn_kernel_dma<4>, 3 = <2, 2, 8>.
// tests/test_vit_attention_probes_gpu.py::test_dispatch_thresholds_are_where_the_probe_lengths_assume pins the thresholds (512, 1024, the
// 2-GiB image) through unopose_vit_attention_route: its sequence lengths sit on both sides of each one, so whoever moves a threshold
// re-chooses those lengths there.
static int vit_attn_route(int T, int H) {
  // T >= 1024: LDS-DMA staging, 4-wave workgroups, two per CU; a qkv image past 2 GiB per crop (32-bit DMA offsets): the register-staged kernel
  if (T >= 1024) return (size_t)T * 3 * H * 64 * 2 < (1UL << 31) ? 2 : 3;
  return T >= 512 ? 1 : 0;
}

template <int QB, int NBUF, int NW>
static int launch_vit_attn(const void *qkv, int B, int T, int H, void *out, hipStream_t stream) {
  return va_launch<&vit_attn_kernel<QB, NBUF, NW>, u16, NW, 32 * QB>("vit_attention", NBUF * VA_BUF * sizeof(u16), qkv, B, T, H, out, stream);
}

extern "C" {

int unopose_vit_attention_route(int T, int H) { return vit_attn_route(T, H); }

int unopose_vit_attention(const void *qkv, int B, int T, int H, void *out, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(qkv && out, "vit_attention: null pointer");
  UNOPOSE_REQUIRE(B >= 0 && T >= 1 && H >= 1 && (long)B * H * cdiv(T, 128) < (1L << 31), "vit_attention: bad sizes");
  if (B == 0) return UNOPOSE_OK;
  switch (vit_attn_route(T, H)) {
    case 3: return launch_vit_attn<2, 2, 8>(qkv, B, T, H, out, (hipStream_t)stream);
    case 2: return va_launch<&vit_attn_kernel_dma<4>, u16, 4, 64>("vit_attention", (size_t)2 * VD_BUFB, qkv, B, T, H, out, (hipStream_t)stream);
    case 1: return launch_vit_attn<2, 2, 4>(qkv, B, T, H, out, (hipStream_t)stream);
    default: return launch_vit_attn<1, 1, 4>(qkv, B, T, H, out, (hipStream_t)stream);
  }
}

}  // extern "C"
