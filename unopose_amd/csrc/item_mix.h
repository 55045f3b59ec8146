// The integer finaliser behind every keyed random number of the online training pairs (provider_online._mix): train_items.hip draws
// point indices with it, scene.hip holes, edge drop-outs, depth noise and the background's texture.
#pragma once
#include "common.h"

namespace unopose {

constexpr unsigned long long ITEM_GOLD = 0x9e3779b97f4a7c15ull;

__device__ __forceinline__ unsigned long long item_mix(unsigned long long z) {  // splitmix64's finaliser
  z ^= z >> 30, z *= 0xbf58476d1ce4e5b9ull;
  z ^= z >> 27, z *= 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

}  // namespace unopose
