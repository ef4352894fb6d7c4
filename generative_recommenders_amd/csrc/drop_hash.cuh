// The counter-based dropout generator shared by the row kernels (norm_kernels.inc: dropout of the output stage) and the
// softmax attention (softmax_attn.hip: dropout on P).  The mask of an element is a pure function of (seed, element
// index), so a backward regenerates it instead of storing it.  One hash gives 32 bits = two 16-bit uniforms for the
// elements 2j and 2j + 1 (pair index pe = e >> 1): keep iff r16 >= thr, thr = round(p 65536) clamped to [1, 65535],
// survivors scaled by 65536 / (65536 - thr), the exact inverse of the keep probability.  The hash is ONE 32-bit
// multiply-xorshift finaliser (murmur3 fmix32) of the pair index's low word xor a key made of both seed words and the
// index's high word.  The CPU checker of the tests (dropout_keep_mask) restates it bit for bit.
#pragma once
#include <stdint.h>

#include "hstu_common.cuh"

namespace hstu {

HSTU_DEV uint32_t drop_key(uint32_t hi, uint32_t s0, uint32_t s1) {
  const uint32_t k = s1 + hi * 0x9e3779b9u;
  return s0 ^ ((k << 16) | (k >> 16));
}
HSTU_DEV uint32_t drop_hash(uint32_t lo, uint32_t key, uint32_t s0, uint32_t s1) {
  // (both seed words enter once more BEHIND the first multiply, as a wave-uniform addend: with the seed only XORed into the index, the masks of two
  // seeds were index-XOR permutations of one table -- mask_B[i] = mask_A[i ^ d] -- and seeds with equal keys gave equal masks;
  // one add per element pair, no multiply: round 5's advisor)
  uint32_t h = lo ^ key;
  h ^= h >> 16; h *= 0x85ebca6bu; h += s1 ^ ((s0 << 13) | (s0 >> 19)); h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
  return h;
}
// the 16-bit uniform of element e
HSTU_DEV uint32_t drop_r16(uint64_t e, uint32_t s0, uint32_t s1) {
  const uint64_t pe = e >> 1;
  const uint32_t h = drop_hash((uint32_t)pe, drop_key((uint32_t)(pe >> 32), s0, s1), s0, s1);
  return (e & 1) ? (h >> 16) : (h & 0xffffu);
}

// host side: threshold (0 = no dropout) and survivor scale of a ratio
inline uint32_t drop_threshold(float ratio) {
  const double t = (double)ratio * 65536.0 + 0.5;
  return ratio > 0.f ? (uint32_t)(t < 1.0 ? 1.0 : (t > 65535.0 ? 65535.0 : t)) : 0u;
}
inline float drop_scale(uint32_t thr) { return 65536.0f / (float)(65536u - thr); }

}  // namespace hstu
