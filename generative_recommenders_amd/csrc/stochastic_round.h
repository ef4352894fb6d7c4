// Stochastic rounding of fp32 to fp16 / bf16, and the counter-based random bits behind it: the rule by which 16-bit embedding
// tables are written back (embedding_optim.hip) and fp32 tables are cast (hstu_stochastic_round).  Plain C++ on integers:
// g++ compiles this header as it stands (tests/test_embedding_lowp_host.py does, and compares it with the numpy
// restatement of tests/embedding_lowp_ref.py bit for bit); under hipcc the functions are __host__ __device__.
//
// RANDOM BITS.  A pure function of (seed: uint64, row: the TABLE row id, col: the column) -- never of the batch position,
// the chunk, the wave or the grid.  One 32-bit hash serves the two columns 2p and 2p + 1 of a row (pair p = col >> 1),
// 16 bits each; the hash is drop_hash.cuh's (murmur3's fmix32 with both seed words added behind the first multiply), the
// row id standing where the dropout has the high word of its element index.  With s0 = seed & 0xffffffff, s1 = seed >> 32,
// rotl = rotate left, all arithmetic modulo 2^32:
//     k   = s1 + row * 0x9e3779b9                          key = s0 ^ rotl(k, 16)
//     h   = pair ^ key;  h ^= h >> 16;  h *= 0x85ebca6b;  h += s1 ^ rotl(s0, 13);  h ^= h >> 13;  h *= 0xc2b2ae35;  h ^= h >> 16
//     r   = col & 1 ? h >> 16 : h & 0xffff                 (16 uniform bits)
//
// RULE, on b = the bits of the fp32 x, a = b & 0x7fffffff, s = the sign bit moved to bit 15:
//   inf / NaN (a >= 0x7f800000): +-inf stays +-inf; NaN becomes the quiet NaN s | 0x7e00 (fp16), (b >> 16) | 0x0040 (bf16).
//   bf16:  o = (b + r) >> 16; a result past the largest finite value is clamped to s | 0x7f7f.
//   fp16, a >= 0x38800000 (|x| >= 2^-14):  o = ((a + (r & 0x1fff)) >> 13) - 0x1c000, clamped to 0x7bff (65504); s | o.
//   fp16, below:  t = |x| 2^24 = i + f with i = floor(t); the magnitude is (i + 1) 2^-24 iff r 2^-16 < f, else i 2^-24; the
//          encoding of a magnitude m 2^-24, m <= 1024, is m itself.  Done on the integer significand: |x| = sig 2^(e - 150),
//          so t = sig / 2^sh with sh = 126 - e >= 14, and r 2^-16 < f  <=>  r 2^sh < (sig mod 2^sh) 2^16.
// Consequences: the result is one of the two 16-bit neighbours of x (away from zero with the probability below, else
// towards it); a representable x has fraction 0 and is returned unchanged for every r; P(away) is the position of |x|
// between its neighbours -- exactly (bf16: a multiple of 2^-16; fp16 above 2^-14: of 2^-13), or rounded up to a multiple
// of 2^-16 (fp16 below 2^-14, where fp32 can hold finer positions);
// +-0 stays +-0; a finite x never becomes infinite.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define HSTU_SR_FN __host__ __device__ inline
#else
#define HSTU_SR_FN inline
#endif

// the 32 random bits of columns 2 * pair and 2 * pair + 1 of table row `row`
HSTU_SR_FN uint32_t hstu_sr_hash(uint64_t seed, uint32_t row, uint32_t pair) {
  const uint32_t s0 = (uint32_t)seed, s1 = (uint32_t)(seed >> 32);
  const uint32_t k = s1 + row * 0x9e3779b9u;
  uint32_t h = pair ^ (s0 ^ ((k << 16) | (k >> 16)));
  h ^= h >> 16; h *= 0x85ebca6bu; h += s1 ^ ((s0 << 13) | (s0 >> 19)); h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
  return h;
}
// the 16 random bits of column `col`
HSTU_SR_FN uint32_t hstu_sr_bits(uint64_t seed, uint32_t row, uint32_t col) {
  const uint32_t h = hstu_sr_hash(seed, row, col >> 1);
  return (col & 1) ? (h >> 16) : (h & 0xffffu);
}

// fp32 bits -> bf16 bits, r: 16 random bits
HSTU_SR_FN uint16_t hstu_sr_bf16(uint32_t b, uint32_t r) {
  const uint32_t a = b & 0x7fffffffu;
  if (a >= 0x7f800000u) return (uint16_t)(a > 0x7f800000u ? (b >> 16) | 0x0040u : b >> 16);
  uint32_t o = (b + r) >> 16;
  if ((o & 0x7fffu) >= 0x7f80u) o = (o & 0x8000u) | 0x7f7fu;
  return (uint16_t)o;
}

// fp32 bits -> fp16 bits, r: 16 random bits
HSTU_SR_FN uint16_t hstu_sr_f16(uint32_t b, uint32_t r) {
  const uint32_t s = (b >> 16) & 0x8000u, a = b & 0x7fffffffu;
  if (a >= 0x7f800000u) return (uint16_t)(s | (a > 0x7f800000u ? 0x7e00u : 0x7c00u));
  if (a >= 0x38800000u) {
    uint32_t o = ((a + (r & 0x1fffu)) >> 13) - 0x1c000u;
    if (o > 0x7bffu) o = 0x7bffu;
    return (uint16_t)(s | o);
  }
  uint32_t e = a >> 23;
  const uint32_t sig = e ? (a & 0x7fffffu) | 0x800000u : a;
  if (!e) e = 1;
  const uint32_t sh = 126u - e;                     // 14 .. 125
  if (sh >= 40u) return (uint16_t)(s | (r == 0u && sig != 0u ? 1u : 0u));   // t < 2^-16: up only on r == 0
  const uint64_t i = (uint64_t)sig >> sh, frac = (uint64_t)sig & (((uint64_t)1 << sh) - 1);
  const uint32_t up = ((uint64_t)r << sh) < (frac << 16) ? 1u : 0u;
  return (uint16_t)(s | ((uint32_t)i + up));
}
