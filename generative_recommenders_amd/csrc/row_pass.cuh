// Device toolkit of the row-pass ops (norm_kernels.inc, multitask_ops.hip, time_ln_ops.hip, loss_ops.hip): one wavefront
// owns a row, lanes own fixed columns, a row is read and written as 16-byte pieces held as fp32, and a column sum goes per
// lane -> LDS over the workgroup's waves -> one fp32 partial row per workgroup -> a fixed-order finish kernel.  A new
// row-pass op includes this header (and asks capi_internal.h's resident_row_blocks for its grid); it does not copy them.
#pragma once
#include "hstu_common.cuh"

namespace hstu {

// a 16-byte piece as loaded -> its VEC elements as fp32
template <typename T, int VEC>
HSTU_DEV void expand_piece(float (&v)[VEC], u32x4 x) {
  static_assert(VEC * sizeof(T) == 16, "a 16-byte piece");
  typedef T tv __attribute__((ext_vector_type(VEC)));
  const tv t = __builtin_bit_cast(tv, x);
#pragma unroll
  for (int i = 0; i < VEC; ++i) v[i] = (float)t[i];
}

// VEC elements at p as fp32: zeros when !ok, one element when VEC == 1, else one 16-byte load
template <typename T, int VEC>
HSTU_DEV void load_piece(float (&v)[VEC], const T* p, bool ok) {
  if (!ok) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) v[i] = 0.f;
    return;
  }
  if constexpr (VEC == 1) {
    v[0] = (float)p[0];
  } else {
    expand_piece<T, VEC>(v, *reinterpret_cast<const u32x4*>(p));
  }
}

// the reverse; NONTEMPORAL: the 16-byte store carries the non-temporal hint -- the caller's choice, per op as measured
// (norm_kernels.inc's store_vec records the numbers).  A single element is always a plain store.
template <typename T, int VEC, bool NONTEMPORAL>
HSTU_DEV void store_piece(const float (&v)[VEC], T* p) {
  if constexpr (VEC == 1) {
    p[0] = (T)v[0];
  } else {
    static_assert(VEC * sizeof(T) == 16, "a 16-byte piece");
    typedef T tv __attribute__((ext_vector_type(VEC)));
    tv t;
#pragma unroll
    for (int i = 0; i < VEC; ++i) t[i] = (T)v[i];
    if constexpr (NONTEMPORAL) __builtin_nontemporal_store(__builtin_bit_cast(u32x4, t), reinterpret_cast<u32x4*>(p));
    else *reinterpret_cast<u32x4*>(p) = __builtin_bit_cast(u32x4, t);
  }
}

// VEC consecutive fp32 parameters (16-byte loads when the row is read in pieces: the class asks for their alignment)
template <int VEC>
HSTU_DEV void load_param(float (&v)[VEC], const float* p, bool ok) {
  if (!ok) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) v[i] = 0.f;
    return;
  }
  if constexpr (VEC == 1) {
    v[0] = p[0];
  } else {
#pragma unroll
    for (int q = 0; q < VEC / 4; ++q) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(p + 4 * q);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[4 * q + i] = t[i];
    }
  }
}

// the sum over the wave's 64 lanes, in every lane
HSTU_DEV float wave_sum(float x) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
  return x;
}

// lane j's value in every lane (j a constant of an unrolled loop: one v_readlane, no LDS crossbar)
HSTU_DEV float lane_value(float v, int j) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), j));
}

// sum over the workgroup's WAVES waves, in wave order, of one per-lane array of column partials -> out[c0 .. c0 + 64 VEC)
// (columns < dim); lds: WAVES * 64 * VEC floats; reached by every thread of the workgroup
template <int VEC, int WAVES>
HSTU_DEV void block_sum_cols(const float (&acc)[VEC], float* lds, float* out, int c0, int dim) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < VEC; ++i) lds[wave * 64 * VEC + lane * VEC + i] = acc[i];
  __syncthreads();
  for (int c = threadIdx.x; c < 64 * VEC; c += 64 * WAVES) {
    float s = 0.f;
#pragma unroll
    for (int w2 = 0; w2 < WAVES; ++w2) s += lds[w2 * 64 * VEC + c];
    if (c0 + c < dim) out[c0 + c] = s;
  }
  __syncthreads();
}

}  // namespace hstu
