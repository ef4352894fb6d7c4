// int8 row-wise quantized embedding tables for inference: the quantize pass over a float table and the dequantizing row
// gather.  Row format and launch geometry: quant_embedding_dispatch.h (all host decisions live there).
//
//   mn = min(x), mx = max(x), range = mx - mn;  scale = range / 255, bias = mn, inv = 255 / (range + 1e-8)
//   code = clamp(rint((x - mn) * inv), 0, 255);  value = code * scale + bias
//
// Both kernels split the workgroup's 256 threads into (rows in flight) x (lanes per row) with the slot rule of row_slots.h
// on the row's pieces, so small rows keep several rows in flight per wave.  A lane's piece is what it STORES with one
// 16-byte instruction: 16 codes in the quantize pass, 4 (fp32) or 8 (16-bit) output elements in the gather -- the lanes of
// a row write consecutive 16-byte pieces.  (A first gather whose lanes loaded 16 codes each and stored 64 bytes of fp32 as
// four 16-byte pieces 64 bytes apart ran at 0.95 TB/s, a third of index_select on the fp32 table: DESIGN 4.14.)  No LDS,
// no atomics; every output byte is written once, by one lane.
#include "capi_internal.h"
#include "hstu_common.cuh"
#include "quant_embedding_dispatch.h"

namespace hstu {
namespace {

namespace qe = quant_embedding;

// the 16 columns [c0, c0 + 16) of a source row as fp32 (exact widening); columns >= dim are not read.  `vec`: every row
// starts 16-byte aligned, so a piece that lies wholly inside the row is read as 16-byte loads
template <typename T>
HSTU_DEV void load_cols16(float (&x)[16], const T* __restrict__ row, int c0, int dim, bool vec) {
  constexpr int N = 16 / sizeof(T);         // elements per 16-byte load
  if (vec && c0 + 16 <= dim) {
    typedef T tv __attribute__((ext_vector_type(N)));
#pragma unroll
    for (int q = 0; q < 16 / N; ++q) {
      const tv t = __builtin_bit_cast(tv, *reinterpret_cast<const u32x4*>(row + c0 + q * N));
#pragma unroll
      for (int e = 0; e < N; ++e) x[q * N + e] = (float)t[e];
    }
  } else {
#pragma unroll
    for (int e = 0; e < 16; ++e) x[e] = c0 + e < dim ? (float)row[c0 + e] : 0.f;
  }
}

// min / max over the lanes of a row (lanes_per_row consecutive lanes, a power of two <= 64), in every lane of it: the wave
// sum's exchange with fminf / fmaxf
HSTU_DEV void row_min_max(float& mn, float& mx, int lanes_per_row) {
  for (int d = lanes_per_row >> 1; d >= 1; d >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, d, 64));
    mx = fmaxf(mx, __shfl_xor(mx, d, 64));
  }
}

// dword w of a quantized row: the packed codes, or scale / bias where the meta data lies (meta is a multiple of 4 >= dim: a
// meta dword holds no code)
HSTU_DEV uint32_t row_dword(uint32_t codes, int w, int meta, float scale, float bias) {
  return 4 * w == meta ? __builtin_bit_cast(uint32_t, scale) : (4 * w == meta + 4 ? __builtin_bit_cast(uint32_t, bias) : codes);
}

template <typename T, int PASSES>
__global__ __launch_bounds__(qe::kThreads) void quantize_rows_int8_kernel(const T* __restrict__ src, int64_t src_rs, int64_t rows, int dim,
                                                                          uint8_t* __restrict__ dst, int64_t dst_rs, int lpr, int meta,
                                                                          int code_pieces, int row_pieces, bool vec) {
  const int lane = threadIdx.x & (lpr - 1), slot = threadIdx.x / lpr, rpw = qe::kThreads / lpr;
  const int64_t chunks = (rows + rpw - 1) / rpw;
  for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    const int64_t r = c * rpw + slot;
    const bool live = r < rows;               // (no early exit: every lane of the wave takes part in the exchange)
    const T* __restrict__ row = src + (live ? r : 0) * src_rs;
    float x[PASSES][16];
    float mn = INFINITY, mx = -INFINITY;
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      const int q = p * lpr + lane;
      if (live && q < code_pieces) {
        load_cols16<T>(x[p], row, 16 * q, dim, vec);
#pragma unroll
        for (int e = 0; e < 16; ++e)
          if (16 * q + e < dim) {
            mn = fminf(mn, x[p][e]);
            mx = fmaxf(mx, x[p][e]);
          }
      }
    }
    row_min_max(mn, mx, lpr);
    const float range = mx - mn;
    const float scale = range / 255.0f, inv = 255.0f / (range + 1e-8f);
    if (!live) continue;
    uint8_t* __restrict__ out = dst + r * dst_rs;
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      const int q = p * lpr + lane;
      if (q >= code_pieces) continue;
      u32x4 w;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        uint32_t codes = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int e = 4 * j + b;
          const float t = (x[p][e] - mn) * inv;                      // subtract, then multiply: two fp32 roundings
          const float k = fminf(fmaxf(rintf(t), 0.f), 255.f);        // rint: to nearest, ties to even
          if (16 * q + e < dim) codes |= (uint32_t)k << (8 * b);
        }
        w[j] = row_dword(codes, 4 * q + j, meta, scale, mn);
      }
      *reinterpret_cast<u32x4*>(out + 16 * q) = w;
    }
    if (lane == 0 && row_pieces > code_pieces) {                     // the one piece behind the codes: meta data and pad
      u32x4 w;
#pragma unroll
      for (int j = 0; j < 4; ++j) w[j] = row_dword(0u, 4 * code_pieces + j, meta, scale, mn);
      *reinterpret_cast<u32x4*>(out + 16 * code_pieces) = w;
    }
  }
}

// the codes of one output piece: 4 (fp32 out) or 8 (16-bit out) bytes, as dwords
template <int G> struct CodeWords;
template <> struct CodeWords<4> { typedef uint32_t type; };
template <> struct CodeWords<8> { typedef u32x2 type; };
HSTU_DEV uint32_t code_word(uint32_t w, int) { return w; }
HSTU_DEV uint32_t code_word(u32x2 w, int j) { return w[j]; }

template <typename I>
HSTU_DEV int64_t gather_row(const I* __restrict__ idx, int64_t i, int64_t table_rows) {
  int64_t r = idx ? (int64_t)idx[i] : i;
  r = r < 0 ? 0 : r;
  return r >= table_rows ? table_rows - 1 : r;     // memory safety only: an id outside the table is the caller's error
}

// G = 16 / sizeof(O) codes per lane and pass -> one 16-byte non-temporal store (single elements at the row's ragged end; the
// output is written once and not read here).  A loop step takes U chunks of rows: their ids, then their codes, scale and
// bias are all requested before the first conversion, so a lane has U (x PASSES) narrow loads in flight.
template <typename O, typename I, int PASSES, int U>
__global__ __launch_bounds__(qe::kThreads) void gather_rows_int8_kernel(const uint8_t* __restrict__ table, int64_t table_rs,
                                                                        int64_t table_rows, int dim, const I* __restrict__ idx, int64_t n,
                                                                        O* __restrict__ out, int64_t out_rs, int lpr, int meta, int pieces) {
  constexpr int G = 16 / sizeof(O);
  typedef typename CodeWords<G>::type words_t;
  typedef O ov __attribute__((ext_vector_type(G)));
  const int lane = threadIdx.x & (lpr - 1), slot = threadIdx.x / lpr, rpw = qe::kThreads / lpr;
  const int64_t per_step = (int64_t)rpw * U;
  const int64_t steps = (n + per_step - 1) / per_step;
  for (int64_t s = blockIdx.x; s < steps; s += gridDim.x) {
    const uint8_t* __restrict__ row[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = (s * U + u) * rpw + slot;
      row[u] = table + (i < n ? gather_row(idx, i, table_rows) : 0) * table_rs;      // (row 0 stands in: read, never stored)
    }
    words_t w[U][PASSES];
    float scale[U], bias[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int p = 0; p < PASSES; ++p) {
        const int q = p * lpr + lane;
        w[u][p] = *reinterpret_cast<const words_t*>(row[u] + G * (q < pieces ? q : 0));
      }
      scale[u] = *reinterpret_cast<const float*>(row[u] + meta);
      bias[u] = *reinterpret_cast<const float*>(row[u] + meta + 4);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = (s * U + u) * rpw + slot;
      if (i >= n) continue;
      O* __restrict__ o = out + i * out_rs;
#pragma unroll
      for (int p = 0; p < PASSES; ++p) {
        const int q = p * lpr + lane;
        if (q >= pieces) continue;
        ov t;
#pragma unroll
        for (int e = 0; e < G; ++e)
          t[e] = (O)((float)(uint8_t)(code_word(w[u][p], e >> 2) >> (8 * (e & 3))) * scale[u] + bias[u]);
        const int c = G * q;
        if (c + G <= dim) {
          __builtin_nontemporal_store(__builtin_bit_cast(u32x4, t), reinterpret_cast<u32x4*>(o + c));
        } else {
#pragma unroll
          for (int e = 0; e < G; ++e)
            if (c + e < dim) o[c + e] = t[e];
        }
      }
    }
  }
}

template <typename T>
int launch_quantize(const void* src, int64_t src_rs, int64_t rows, int dim, void* dst, int64_t dst_rs, hipStream_t st, const char* what) {
  const qe::Split s = qe::quantize_split(dim);
  const int grid = qe::grid(rows, s, cu_count());
  const bool vec = !((uintptr_t)src & 15) && (src_rs * (int64_t)sizeof(T)) % 16 == 0;
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(qe::kThreads), 0, st, (const T*)src, src_rs, rows, dim, (uint8_t*)dst, dst_rs,
                       s.lanes, qe::meta_offset(dim), s.pieces, qe::row_pieces(dim), vec);
    return check_launch(what);
  };
  return s.passes == 1 ? go(quantize_rows_int8_kernel<T, 1>) : go(quantize_rows_int8_kernel<T, 2>);
}

template <typename O, typename I>
int launch_gather(const void* table, int64_t table_rs, int64_t table_rows, int dim, const void* idx, int64_t n, void* out, int64_t out_rs,
                  hipStream_t st, const char* what) {
  const qe::Split s = qe::gather_split(dim, (int)sizeof(O));
  const int grid = qe::grid(n, s, cu_count());
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(qe::kThreads), 0, st, (const uint8_t*)table, table_rs, table_rows, dim,
                       (const I*)idx, n, (O*)out, out_rs, s.lanes, qe::meta_offset(dim), s.pieces);
    return check_launch(what);
  };
  if constexpr (sizeof(O) == 4)       // (2048 columns are 256 pieces of a 16-bit output: one pass of the workgroup)
    if (s.passes == 2) return go(gather_rows_int8_kernel<O, I, 2, qe::kGatherChunks>);
  return go(gather_rows_int8_kernel<O, I, 1, qe::kGatherChunks>);
}

template <typename O>
int launch_gather_index(int index_type, const void* table, int64_t table_rs, int64_t table_rows, int dim, const void* idx, int64_t n,
                        void* out, int64_t out_rs, hipStream_t st, const char* what) {
  if (idx && index_type == HSTU_INDEX_I64) return launch_gather<O, int64_t>(table, table_rs, table_rows, dim, idx, n, out, out_rs, st, what);
  return launch_gather<O, int32_t>(table, table_rs, table_rows, dim, idx, n, out, out_rs, st, what);
}

// the checks both entry points share: dim, and the quantized table's base and row stride
int check_table(const char* what, const char* name, const void* table, int64_t row_stride, int dim) {
  if (dim < 1) return set_error(HSTU_EINVAL, "%s: dim must be at least 1 (got %d)", what, dim);
  if (dim > qe::kMaxDim) return set_error(HSTU_EUNSUPPORTED, "%s: rows of %d columns > %d", what, dim, qe::kMaxDim);
  if ((uintptr_t)table & 15) return set_error(HSTU_EINVAL, "%s: %s must be 16-byte aligned", what, name);
  if (row_stride < qe::row_stride(dim) || row_stride % 16)
    return set_error(HSTU_EINVAL, "%s: the row stride of %s must be a multiple of 16 and at least hstu_int8_row_stride(%d) = %d (got %lld)",
                     what, name, dim, qe::row_stride(dim), (long long)row_stride);
  return HSTU_OK;
}

}  // namespace
}  // namespace hstu

using namespace hstu;

extern "C" {

int hstu_int8_row_stride(int32_t dim) {
  if (dim < 1) return set_error(HSTU_EINVAL, "hstu_int8_row_stride: dim must be at least 1 (got %d)", dim);
  if (dim > qe::kMaxDim) return set_error(HSTU_EUNSUPPORTED, "hstu_int8_row_stride: rows of %d columns > %d", dim, qe::kMaxDim);
  return qe::row_stride(dim);
}

int hstu_quantize_rows_int8(const void* src, int64_t src_row_stride, int64_t rows, int32_t dim, void* dst, int64_t dst_row_stride,
                            int src_dtype, void* stream) {
  const char* what = "hstu_quantize_rows_int8";
  if (!is_float_dtype(src_dtype)) return set_error(HSTU_EINVAL, "%s: src_dtype must be bf16, fp16 or fp32", what);
  if (const int e = check_table(what, "dst", dst, dst_row_stride, dim)) return e;
  if (rows < 0 || rows > 0x7fffffffLL) return set_error(HSTU_EINVAL, "%s: rows must be in [0, 2^31)", what);
  if (src_row_stride < dim) return set_error(HSTU_EINVAL, "%s: src_row_stride %lld < dim %d", what, (long long)src_row_stride, dim);
  if (rows == 0) return HSTU_OK;
  if (!src || !dst) return set_error(HSTU_EINVAL, "%s: NULL input", what);
  hipStream_t st = (hipStream_t)stream;
  switch (src_dtype) {
    case HSTU_DTYPE_BF16: return launch_quantize<bf16_t>(src, src_row_stride, rows, dim, dst, dst_row_stride, st, what);
    case HSTU_DTYPE_F16: return launch_quantize<f16_t>(src, src_row_stride, rows, dim, dst, dst_row_stride, st, what);
    default: return launch_quantize<float>(src, src_row_stride, rows, dim, dst, dst_row_stride, st, what);
  }
}

int hstu_gather_rows_int8(const void* table, int64_t table_row_stride, int64_t table_rows, int32_t dim, const void* idx, int index_type,
                          int64_t n, void* out, int64_t out_row_stride, int out_dtype, void* stream) {
  const char* what = "hstu_gather_rows_int8";
  if (!is_float_dtype(out_dtype)) return set_error(HSTU_EINVAL, "%s: out_dtype must be bf16, fp16 or fp32", what);
  if (idx && index_type != HSTU_INDEX_I32 && index_type != HSTU_INDEX_I64)
    return set_error(HSTU_EINVAL, "%s: index_type must be HSTU_INDEX_I32 or HSTU_INDEX_I64", what);
  if (const int e = check_table(what, "table", table, table_row_stride, dim)) return e;
  if (n < 0 || n > 0x7fffffffLL || table_rows < 0 || table_rows > 0x7fffffffLL)
    return set_error(HSTU_EINVAL, "%s: n and table_rows must be in [0, 2^31)", what);
  if (out_row_stride < dim || (out_row_stride * dtype_bytes(out_dtype)) % 16 || ((uintptr_t)out & 15))
    return set_error(HSTU_EINVAL, "%s: every out row must start 16-byte aligned and hold dim columns (out_row_stride %lld elements)", what,
                     (long long)out_row_stride);
  if (n == 0) return HSTU_OK;
  if (table_rows == 0) return set_error(HSTU_EINVAL, "%s: %lld rows asked of an empty table", what, (long long)n);
  if (!idx && n > table_rows) return set_error(HSTU_EINVAL, "%s: idx == NULL takes rows 0 .. n - 1, n %lld > table_rows %lld", what,
                                              (long long)n, (long long)table_rows);
  if (!table || !out) return set_error(HSTU_EINVAL, "%s: NULL input", what);
  hipStream_t st = (hipStream_t)stream;
  switch (out_dtype) {
    case HSTU_DTYPE_BF16: return launch_gather_index<bf16_t>(index_type, table, table_row_stride, table_rows, dim, idx, n, out, out_row_stride, st, what);
    case HSTU_DTYPE_F16: return launch_gather_index<f16_t>(index_type, table, table_row_stride, table_rows, dim, idx, n, out, out_row_stride, st, what);
    default: return launch_gather_index<float>(index_type, table, table_row_stride, table_rows, dim, idx, n, out, out_row_stride, st, what);
  }
}

}  // extern "C"
