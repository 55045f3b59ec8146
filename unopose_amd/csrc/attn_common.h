// What the bf16 (attn.hip) and the fp32-class (attn_f32.hip) token attention kernels share: the key-tile geometry their
// callers size V^T, K^T and the saved P by, and the softmax's 16-lane row reductions.
#pragma once
#include "common.h"

namespace unopose {

constexpr int TA_NT = 14;          // key tiles of 16 -> up to 224 keys
constexpr int TA_MP = TA_NT * 16;  // padded key count (V^T, K^T, the saved P and the P staging use this stride): unopose_token_attention_key_pad()

template <int XOR>
__device__ __forceinline__ float swz_xor(float v) {  // butterfly step inside a 16-lane row, no LDS memory touched
  // (DPP rather than ds_swizzle through the LDS crossbar: DESIGN.md section 7)
  // DPP: quad_perm [1,0,3,2] / [2,3,0,1] for xor 1 / 2; row_half_mirror / row_mirror for xor 4 / 8 -- applied in this order every
  // lane's partner group holds the value the xor partner would (the groups are uniform by then), so sums and maxima are unchanged
  constexpr int ctrl = XOR == 1 ? 0xB1 : XOR == 2 ? 0x4E : XOR == 4 ? 0x141 : 0x140;
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), ctrl, 0xF, 0xF, false));
}
__device__ __forceinline__ float row16_max(float v) {
  v = fmaxf(v, swz_xor<1>(v));
  v = fmaxf(v, swz_xor<2>(v));
  v = fmaxf(v, swz_xor<4>(v));
  v = fmaxf(v, swz_xor<8>(v));
  return v;
}
__device__ __forceinline__ float row16_sum(float v) {
  v += swz_xor<1>(v);
  v += swz_xor<2>(v);
  v += swz_xor<4>(v);
  v += swz_xor<8>(v);
  return v;
}

__device__ __forceinline__ bf16x8 zero8() {
  bf16x8 z;
#pragma unroll
  for (int i = 0; i < 8; ++i) z[i] = (__bf16)0.f;
  return z;
}

}  // namespace unopose
