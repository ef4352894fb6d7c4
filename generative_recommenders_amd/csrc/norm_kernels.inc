// Row kernels of norm_ops.hip and their host-side launchers.  Included TWICE by norm_ops.hip, inside namespaces hstu::nw1
// (NORM_WIDE = 1: rows of up to 1024 elements, 16-byte pieces in registers) and hstu::nw4 (NORM_WIDE = 4: up to 4096).

#ifndef NORM_PREFETCH
#define NORM_PREFETCH 0   // 1: u * GroupNorm(attn) requests the next row's pieces before working on the current one.  Measured with the
#endif                    // resident grid (204800 rows of 512 bf16): forward 125 vs 122 us, backward 209 vs 202 -- no gain, off
constexpr int kNormThreads = 256;
constexpr int kNormWaves = kNormThreads / 64;
// register-resident pieces per lane: 16-bit x8 -> dim <= 1024, fp32 x4 -> dim <= 1024, scalar -> dim <= 512
// (NORM_WIDE: this file is compiled twice -- rows up to 1024 elements keep the register budget of the metric shapes, the
// wide instance holds 4x the pieces per lane for rows up to 4096)
// (the kernels of the layer's own row passes take the chunk count as a template parameter MC and are also instantiated
// with MC = 1 -- a row of up to 64 pieces, e.g. 512 bf16 -- where the second chunk's registers would only cost occupancy)
template <int VEC> constexpr int max_chunks() { return NORM_WIDE * (VEC == 8 ? 2 : (VEC == 4 ? 4 : 8)); }
// (norm_dispatch.h picks the instance from these capacities: the two must not drift apart)
static_assert(max_chunks<8>() == norm_dispatch::pieces_per_lane(8, NORM_WIDE == 4) && max_chunks<4>() == norm_dispatch::pieces_per_lane(4, NORM_WIDE == 4) &&
              max_chunks<1>() == norm_dispatch::pieces_per_lane(1, NORM_WIDE == 4), "norm_dispatch.h and max_chunks() disagree");
constexpr int kMaxNormBlocks = 2048;

template <typename T, int VEC> struct RowVec {
  float v[VEC];
};

// The pieces are row_pass.cuh's.  A row's pieces are loaded with load_piece<T, VEC>(r.v, ..) itself: a load_vec wrapper
// around it -- one more level of inlining around its early return -- changes the register allocation of 71 of this
// file's 254 kernels.  (The non-temporal hint on the loads: mixed, norm_mul bwd +6 %; profiles/r04_norm_nt.txt)

// (stores: non-temporal for the 16-bit dtypes: layer norm fwd 81 -> 68 us, SiLU fwd 81 -> 62 us, the others -1..-3 %, layer step
// unchanged; profiles/r04_norm_nt.txt.  fp32 pieces: plain stores)
template <typename T, int VEC>
HSTU_DEV void store_vec(const RowVec<T, VEC>& r, T* p) { store_piece<T, VEC, sizeof(T) == 2>(r.v, p); }

// 16-byte piece as loaded (prefetch of the next row: 4 registers instead of the 8 of its fp32 expansion) and its expansion
template <typename T> HSTU_DEV u32x4 load_raw16(const T* p) { return *reinterpret_cast<const u32x4*>(p); }
template <typename T, int VEC> HSTU_DEV void expand_raw16(RowVec<T, VEC>& r, u32x4 x) { expand_piece<T, VEC>(r.v, x); }

// ------------------------------------------------------------------ fused dropout of the output stage
// Replaces the Philox dropout inside _ln_mul_dropout_fwd / _group_norm_mul_dropout_fwd (triton_hstu_linear.py:101-120,
// 631-652; backward :196-215, :718-738): the mask of an output element is a pure function of (seed, element index in the
// (rows, out_stride) output), so the backward -- and the forward recompute of y -- regenerate it instead of storing it.
// One hash gives 32 bits = two 16-bit uniforms for the elements 2j and 2j+1: keep iff r16 >= thr, thr = round(p 65536),
// survivors scaled by 65536 / (65536 - thr) (the exact inverse of the keep probability).  The hash is ONE 32-bit
// multiply-xorshift finaliser (murmur3 fmix32) of the pair index xor a key made of both seed words and the index's high
// word: 32-bit integer multiplies issue at a quarter of the VALU rate, and the second round the first four rounds of this
// code carried (lowbias32) bought nothing the tests can see -- keep rate per tensor / row / column, neighbour, row and
// seed correlations, chi-square of the uniforms (tools/dropout_hash_stats.py) -- for 2 of the pair's 5 multiplies.
// The CPU checker of the tests restates it bit for bit (dropout_keep_mask).
struct DropCtx {
  uint32_t thr;        // 0 = no dropout
  float scale;
  uint32_t s0, s1;
};
// drop_key / drop_hash: drop_hash.cuh (shared with the softmax attention)
// v[i] *= keep(e0 + i) ? scale : 0 for i < VEC; e0 = index of v[0] in the output tensor, a multiple of VEC (rows, column
// offsets and the output stride of a vector instantiation are multiples of VEC): the VEC / 2 pair indices of a piece then
// share their high word -- pe0 is a multiple of VEC / 2 -- and the key is formed once per piece
template <typename T, int VEC>
HSTU_DEV void drop_apply(RowVec<T, VEC>& r, int64_t e0, const DropCtx& dc) {
  if constexpr (VEC == 1) {
    const uint64_t pe = (uint64_t)e0 >> 1;
    const uint32_t hi = (uint32_t)(pe >> 32);
    const uint32_t h = drop_hash((uint32_t)pe, drop_key(hi, dc.s0, dc.s1), dc.s0, dc.s1);
    const uint32_t r16 = (e0 & 1) ? (h >> 16) : (h & 0xffffu);
    r.v[0] = r16 >= dc.thr ? r.v[0] * dc.scale : 0.f;
  } else {
    const uint64_t pe0 = (uint64_t)e0 >> 1;
    const uint32_t lo0 = (uint32_t)pe0, hi = (uint32_t)(pe0 >> 32);
    const uint32_t key = drop_key(hi, dc.s0, dc.s1);
#pragma unroll
    for (int j = 0; j < VEC / 2; ++j) {
      const uint32_t h = drop_hash(lo0 + j, key, dc.s0, dc.s1);
      r.v[2 * j] = (h & 0xffffu) >= dc.thr ? r.v[2 * j] * dc.scale : 0.f;
      r.v[2 * j + 1] = (h >> 16) >= dc.thr ? r.v[2 * j + 1] * dc.scale : 0.f;
    }
  }
}
static DropCtx make_drop_ctx(float ratio, uint64_t seed) {
  DropCtx dc;
  dc.thr = drop_threshold(ratio);
  dc.scale = drop_scale(dc.thr);
  dc.s0 = (uint32_t)seed;
  dc.s1 = (uint32_t)(seed >> 32);
  return dc;
}

// ------------------------------------------------------------------ SiLU, shared by its own kernels and the fused u source
// u given as the PRE-activation (the u slice of the uvqk buffer, row stride u_stride): the u * Norm(attn) kernels then
// apply SiLU on the fly -- rounded to T exactly where the separate SiLU kernel would have stored it -- and the backward
// kernel multiplies d u (rounded to T likewise) by SiLU' and writes straight into the u slice of the d uvqk buffer.
struct USrc {
  int64_t u_stride;    // elements between rows of u
  int64_t du_stride;   // ... of d u (backward)
};
// (the sigmoid through the hardware exp2 / rcp, 1 ulp each, as the attention kernels form it; expf and an IEEE divide
// take ~10 more instructions per element)
HSTU_DEV float norm_sigmoid(float x) { return fast_sigmoid(x); }
HSTU_DEV float silu_val(float x) {
  const float sg = norm_sigmoid(x);
  return x * sg;
}
HSTU_DEV float silu_grad_val(float g, float x) {
  const float sg = norm_sigmoid(x);
  return g * sg * (1.f + x * (1.f - sg));
}
// a row piece as T again (8 bf16 = 4 registers instead of the 8 of its fp32 expansion): exact, the values came from T
template <typename T, int VEC> struct PackedVec {
  typedef T tv __attribute__((ext_vector_type(VEC)));
  tv t;
};
template <typename T, int VEC> HSTU_DEV void pack_vec(PackedVec<T, VEC>& p, const RowVec<T, VEC>& r) {
#pragma unroll
  for (int i = 0; i < VEC; ++i) p.t[i] = (T)r.v[i];
}
template <typename T, int VEC> HSTU_DEV void unpack_vec(RowVec<T, VEC>& r, const PackedVec<T, VEC>& p) {
#pragma unroll
  for (int i = 0; i < VEC; ++i) r.v[i] = (float)p.t[i];
}
template <typename T, int VEC> HSTU_DEV void silu_rounded(RowVec<T, VEC>& r) {
#pragma unroll
  for (int i = 0; i < VEC; ++i) r.v[i] = (float)(T)silu_val(r.v[i]);
}
// d (pre-activation) = T(d u) * SiLU'(pre)
template <typename T, int VEC> HSTU_DEV void silu_grad_rounded(RowVec<T, VEC>& d, const RowVec<T, VEC>& pre) {
#pragma unroll
  for (int i = 0; i < VEC; ++i) d.v[i] = silu_grad_val((float)(T)d.v[i], pre.v[i]);
}

// ------------------------------------------------------------------ layer norm
// SWISH: y = x * sigmoid(LayerNorm(x)) (swish_layer_norm, ops/layer_norm.py:79-112; math ops/pytorch/pt_layer_norm.py:41-62;
// Triton: ops/triton/triton_layer_norm.py _swish_layer_norm kernels) -- the same pass with one more multiply per element
template <typename T, int VEC, int MC = max_chunks<VEC>(), bool SWISH = false>
__global__ __launch_bounds__(kNormThreads) void layer_norm_fwd_kernel(const T* x, const T* w, const T* b, T* y,
                                                                      float* mean_out, float* rstd_out, int64_t rows,
                                                                      int dim, float eps) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nch = (dim + 64 * VEC - 1) / (64 * VEC);
  RowVec<T, VEC> wv[MC], bv[MC];
#pragma unroll
  for (int k = 0; k < MC; ++k) {
    const int c = (k * 64 + lane) * VEC;
    load_piece<T, VEC>(wv[k].v, w + c, k < nch && c < dim);
    load_piece<T, VEC>(bv[k].v, b + c, k < nch && c < dim);
  }
  for (int64_t row = (int64_t)blockIdx.x * kNormWaves + wave; row < rows; row += (int64_t)gridDim.x * kNormWaves) {
    RowVec<T, VEC> xv[MC];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < MC; ++k) {
      const int c = (k * 64 + lane) * VEC;
      load_piece<T, VEC>(xv[k].v, x + row * dim + c, k < nch && c < dim);
#pragma unroll
      for (int i = 0; i < VEC; ++i) s += xv[k].v[i];
    }
    const float mean = wave_sum(s) / dim;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < MC; ++k) {
      const int c = (k * 64 + lane) * VEC;
      if (k < nch && c < dim) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) { const float d = xv[k].v[i] - mean; q += d * d; }
      }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / dim + eps);
#pragma unroll
    for (int k = 0; k < MC; ++k) {
      const int c = (k * 64 + lane) * VEC;
      if (k < nch && c < dim) {
        RowVec<T, VEC> o;
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          o.v[i] = (xv[k].v[i] - mean) * rstd * wv[k].v[i] + bv[k].v[i];
          if constexpr (SWISH) o.v[i] = xv[k].v[i] * norm_sigmoid(o.v[i]);
        }
        store_vec<T, VEC>(o, y + row * dim + c);
      }
    }
    if (lane == 0) {
      if (mean_out) mean_out[row] = mean;
      if (rstd_out) rstd_out[row] = rstd;
    }
  }
}

// block-level reduction of per-lane column partials -> one fp32 partial row per workgroup
template <int VEC, int MC = max_chunks<VEC>()>
HSTU_DEV void block_reduce_cols(float (&acc)[MC][VEC], float* lds, float* out_row, int dim, int nch) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // lds: [kNormWaves][dim_padded]
  const int dpad = nch * 64 * VEC;
#pragma unroll
  for (int k = 0; k < MC; ++k)
    if (k < nch)
#pragma unroll
      for (int i = 0; i < VEC; ++i) lds[wave * dpad + (k * 64 + lane) * VEC + i] = acc[k][i];
  __syncthreads();
  for (int c = threadIdx.x; c < dim; c += kNormThreads) {
    float s = 0.f;
#pragma unroll
    for (int w2 = 0; w2 < kNormWaves; ++w2) s += lds[w2 * dpad + c];
    out_row[c] = s;
  }
  __syncthreads();
}

// SWISH (b = the norm's bias, read only then): with s = sigmoid(z), z = xhat w + b, the gradient entering the norm is
// d z = dy x s (1 - s) and dy s reaches x directly (added where `dres` would be: the two are never used together)
template <typename T, int VEC, int MC = max_chunks<VEC>(), bool SWISH = false>
__global__ __launch_bounds__(kNormThreads) void layer_norm_bwd_kernel(const T* dy, const T* x, const T* w,
                                                                      const float* mean_in, const float* rstd_in, T* dx,
                                                                      float* partial, int64_t rows, int dim, const T* dres,
                                                                      const T* b = nullptr) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nch = (dim + 64 * VEC - 1) / (64 * VEC);
  RowVec<T, VEC> wv[MC];
  [[maybe_unused]] RowVec<T, VEC> bv[SWISH ? MC : 1];
  float dw[MC][VEC], db[MC][VEC];
#pragma unroll
  for (int k = 0; k < MC; ++k) {
    const int c = (k * 64 + lane) * VEC;
    load_piece<T, VEC>(wv[k].v, w + c, k < nch && c < dim);
    if constexpr (SWISH) load_piece<T, VEC>(bv[k].v, b + c, k < nch && c < dim);
#pragma unroll
    for (int i = 0; i < VEC; ++i) { dw[k][i] = 0.f; db[k][i] = 0.f; }
  }
  for (int64_t row = (int64_t)blockIdx.x * kNormWaves + wave; row < rows; row += (int64_t)gridDim.x * kNormWaves) {
    const float mean = mean_in[row], rstd = rstd_in[row];
    RowVec<T, VEC> xh[MC], g[MC];
    [[maybe_unused]] RowVec<T, VEC> direct[SWISH ? MC : 1];    // dy s
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < MC; ++k) {
      const int c = (k * 64 + lane) * VEC;
      const bool ok = k < nch && c < dim;
      RowVec<T, VEC> dyv;
      load_piece<T, VEC>(xh[k].v, x + row * dim + c, ok);
      load_piece<T, VEC>(dyv.v, dy + row * dim + c, ok);
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        const float xhat = ok ? (xh[k].v[i] - mean) * rstd : 0.f;
        if constexpr (SWISH) {
          const float sg = norm_sigmoid(xhat * wv[k].v[i] + bv[k].v[i]);
          direct[k].v[i] = dyv.v[i] * sg;
          dyv.v[i] = direct[k].v[i] * xh[k].v[i] * (1.0f - sg);      // d z (padding lanes: dy = 0)
        }
        xh[k].v[i] = xhat;
        g[k].v[i] = dyv.v[i] * wv[k].v[i];
        s1 += g[k].v[i] * xhat;
        s2 += g[k].v[i];
        dw[k][i] += dyv.v[i] * xhat;
        db[k][i] += dyv.v[i];
      }
    }
    const float c1 = wave_sum(s1) / dim, c2 = wave_sum(s2) / dim;
#pragma unroll
    for (int k = 0; k < MC; ++k) {
      const int c = (k * 64 + lane) * VEC;
      if (k < nch && c < dim) {
        RowVec<T, VEC> o;
#pragma unroll
        for (int i = 0; i < VEC; ++i) o.v[i] = rstd * (g[k].v[i] - c2 - xh[k].v[i] * c1);
        if constexpr (SWISH) {
#pragma unroll
          for (int i = 0; i < VEC; ++i) o.v[i] += direct[k].v[i];
        }
        if (dres) {   // kernel-uniform: + the gradient that reaches x around the norm (the layer's residual), as the
                      // framework's add of two T tensors would form it
          RowVec<T, VEC> rv;
          load_piece<T, VEC>(rv.v, dres + row * dim + c, true);
#pragma unroll
          for (int i = 0; i < VEC; ++i) o.v[i] = __fadd_rn((float)(T)o.v[i], rv.v[i]);   // (no contraction with the product above: fp32 rows)
        }
        store_vec<T, VEC>(o, dx + row * dim + c);
      }
    }
  }
  block_reduce_cols<VEC, MC>(dw, lds, partial + (int64_t)blockIdx.x * 2 * dim, dim, nch);
  block_reduce_cols<VEC, MC>(db, lds, partial + (int64_t)blockIdx.x * 2 * dim + dim, dim, nch);
}

// Column sums of the (nparts, 2 * width) partial matrix: columns [0, width) -> out_w, [width, 2 width) -> out_b.
// One 256-thread block per column: thread t adds rows t, t + 256, ... in a fixed order, then the block combines
// the 256 sums in a fixed tree (deterministic).  (One thread per column walking all the rows is latency bound:
// with group norm the width is the number of heads, i.e. 4 threads for ~1000 dependent loads.)
__global__ __launch_bounds__(256) void reduce_partials_kernel(const float* partial, int nparts, int width, float* out_w,
                                                              float* out_b) {
  __shared__ float red[256];
  const int c = blockIdx.x;
  float s = 0.f;
  for (int i = threadIdx.x; i < nparts; i += 256) s += partial[(int64_t)i * (2 * width) + c];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (c < width) out_w[c] = red[0];
    else out_b[c - width] = red[0];
  }
}

// ------------------------------------------------------------------ RMS norm
// y = x rstd w, rstd = 1 / sqrt(mean_j x_j^2 + eps) (RMSNorm, ops/layer_norm.py:139-158; Triton:
// ops/triton/triton_layer_norm.py:525-749): layer norm's pass without the mean and the bias -- one sum per row instead of
// two dependent ones, one parameter piece per column instead of two.  Lanes past the row hold zeros, which add nothing.
template <typename T, int VEC, int MC = max_chunks<VEC>()>
__global__ __launch_bounds__(kNormThreads) void rms_norm_fwd_kernel(const T* x, const T* w, T* y, float* rstd_out,
                                                                    int64_t rows, int dim, float eps) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nch = (dim + 64 * VEC - 1) / (64 * VEC);
  RowVec<T, VEC> wv[MC];
#pragma unroll
  for (int k = 0; k < MC; ++k) {
    const int c = (k * 64 + lane) * VEC;
    load_piece<T, VEC>(wv[k].v, w + c, k < nch && c < dim);
  }
  for (int64_t row = (int64_t)blockIdx.x * kNormWaves + wave; row < rows; row += (int64_t)gridDim.x * kNormWaves) {
    RowVec<T, VEC> xv[MC];
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < MC; ++k) {
      const int c = (k * 64 + lane) * VEC;
      load_piece<T, VEC>(xv[k].v, x + row * dim + c, k < nch && c < dim);
#pragma unroll
      for (int i = 0; i < VEC; ++i) q += xv[k].v[i] * xv[k].v[i];
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / dim + eps);
#pragma unroll
    for (int k = 0; k < MC; ++k) {
      const int c = (k * 64 + lane) * VEC;
      if (k < nch && c < dim) {
        RowVec<T, VEC> o;
#pragma unroll
        for (int i = 0; i < VEC; ++i) o.v[i] = xv[k].v[i] * rstd * wv[k].v[i];
        store_vec<T, VEC>(o, y + row * dim + c);
      }
    }
    if (lane == 0 && rstd_out) rstd_out[row] = rstd;
  }
}

// dx = (w dy - xhat mean_j(xhat w dy)) rstd, xhat = x rstd; dweight = sum_r dy xhat per lane, then block_reduce_cols ->
// columns [0, dim) of this workgroup's partial row (the bias half of the row stays unused) -> reduce_partials_kernel.
// (The reference adds its per-program partials under a spin lock, in the order the programs arrive.)
template <typename T, int VEC, int MC = max_chunks<VEC>()>
__global__ __launch_bounds__(kNormThreads) void rms_norm_bwd_kernel(const T* dy, const T* x, const T* w, const float* rstd_in,
                                                                    T* dx, float* partial, int64_t rows, int dim) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nch = (dim + 64 * VEC - 1) / (64 * VEC);
  RowVec<T, VEC> wv[MC];
  float dw[MC][VEC];
#pragma unroll
  for (int k = 0; k < MC; ++k) {
    const int c = (k * 64 + lane) * VEC;
    load_piece<T, VEC>(wv[k].v, w + c, k < nch && c < dim);
#pragma unroll
    for (int i = 0; i < VEC; ++i) dw[k][i] = 0.f;
  }
  for (int64_t row = (int64_t)blockIdx.x * kNormWaves + wave; row < rows; row += (int64_t)gridDim.x * kNormWaves) {
    const float rstd = rstd_in[row];
    RowVec<T, VEC> xh[MC], g[MC];
    float s1 = 0.f;
#pragma unroll
    for (int k = 0; k < MC; ++k) {
      const int c = (k * 64 + lane) * VEC;
      const bool ok = k < nch && c < dim;
      RowVec<T, VEC> dyv;
      load_piece<T, VEC>(xh[k].v, x + row * dim + c, ok);
      load_piece<T, VEC>(dyv.v, dy + row * dim + c, ok);
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        xh[k].v[i] *= rstd;                         // (padding lanes: x = dy = w = 0)
        g[k].v[i] = dyv.v[i] * wv[k].v[i];
        s1 += g[k].v[i] * xh[k].v[i];
        dw[k][i] += dyv.v[i] * xh[k].v[i];
      }
    }
    const float c1 = wave_sum(s1) / dim;
#pragma unroll
    for (int k = 0; k < MC; ++k) {
      const int c = (k * 64 + lane) * VEC;
      if (k < nch && c < dim) {
        RowVec<T, VEC> o;
#pragma unroll
        for (int i = 0; i < VEC; ++i) o.v[i] = rstd * (g[k].v[i] - xh[k].v[i] * c1);
        store_vec<T, VEC>(o, dx + row * dim + c);
      }
    }
  }
  block_reduce_cols<VEC, MC>(dw, lds, partial + (int64_t)blockIdx.x * 2 * dim, dim, nch);
}

// ------------------------------------------------------------------ y = u * Norm(attn) [, concat]
// LN: statistics over the whole row, weight/bias per column.
// GN: statistics per head (head_dim columns), weight/bias per head.
template <typename T, int VEC, bool GN, bool SILU = false>
__global__ __launch_bounds__(kNormThreads) void norm_mul_fwd_kernel(const T* attn, const T* u, const T* w, const T* b,
                                                                    T* y, float* mean_out, float* rstd_out,
                                                                    int64_t rows, int heads, int hdim, float eps,
                                                                    int concat, DropCtx dc, USrc us) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int dim = heads * hdim;
  const int nch = (dim + 64 * VEC - 1) / (64 * VEC);
  const int ostride = concat ? 3 * dim : dim;
  for (int64_t row = (int64_t)blockIdx.x * kNormWaves + wave; row < rows; row += (int64_t)gridDim.x * kNormWaves) {
    RowVec<T, VEC> xv[max_chunks<VEC>()], uv[max_chunks<VEC>()];
#pragma unroll
    for (int k = 0; k < max_chunks<VEC>(); ++k) {
      const int c = (k * 64 + lane) * VEC;
      const bool ok = k < nch && c < dim;
      load_piece<T, VEC>(xv[k].v, attn + row * dim + c, ok);
      load_piece<T, VEC>(uv[k].v, u + row * us.u_stride + c, ok);
      if constexpr (SILU) silu_rounded<T, VEC>(uv[k]);
    }
    const int ngroups = GN ? heads : 1;
    const int gdim = GN ? hdim : dim;
    for (int gi = 0; gi < ngroups; ++gi) {
      const int lo = gi * gdim, hi = lo + gdim;
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < max_chunks<VEC>(); ++k) {
        const int c = (k * 64 + lane) * VEC;
        if (k < nch && c >= lo && c < hi)
#pragma unroll
          for (int i = 0; i < VEC; ++i) s += xv[k].v[i];
      }
      const float mean = wave_sum(s) / gdim;
      float q = 0.f;
#pragma unroll
      for (int k = 0; k < max_chunks<VEC>(); ++k) {
        const int c = (k * 64 + lane) * VEC;
        if (k < nch && c >= lo && c < hi)
#pragma unroll
          for (int i = 0; i < VEC; ++i) { const float d = xv[k].v[i] - mean; q += d * d; }
      }
      const float rstd = 1.0f / sqrtf(wave_sum(q) / gdim + eps);
      float gw = 0.f, gb = 0.f;
      if (GN) { gw = (float)w[gi]; gb = (float)b[gi]; }
#pragma unroll
      for (int k = 0; k < max_chunks<VEC>(); ++k) {
        const int c = (k * 64 + lane) * VEC;
        if (k < nch && c >= lo && c < hi) {
          RowVec<T, VEC> wv, bv, o;
          if (!GN) { load_piece<T, VEC>(wv.v, w + c, true); load_piece<T, VEC>(bv.v, b + c, true); }
#pragma unroll
          for (int i = 0; i < VEC; ++i) {
            const float n = (xv[k].v[i] - mean) * rstd * (GN ? gw : wv.v[i]) + (GN ? gb : bv.v[i]);
            o.v[i] = uv[k].v[i] * n;
          }
          T* yrow = y + row * ostride;
          if (concat) {
            RowVec<T, VEC> ud = uv[k], xd = xv[k];
            if (dc.thr) {   // kernel-uniform
              drop_apply<T, VEC>(ud, row * ostride + c, dc);
              drop_apply<T, VEC>(xd, row * ostride + dim + c, dc);
              drop_apply<T, VEC>(o, row * ostride + 2 * dim + c, dc);
            }
            store_vec<T, VEC>(ud, yrow + c);
            store_vec<T, VEC>(xd, yrow + dim + c);
            store_vec<T, VEC>(o, yrow + 2 * dim + c);
          } else {
            if (dc.thr) drop_apply<T, VEC>(o, row * ostride + c, dc);
            store_vec<T, VEC>(o, yrow + c);
          }
        }
      }
      if (lane == 0) {
        if (mean_out) mean_out[row * ngroups + gi] = mean;
        if (rstd_out) rstd_out[row * ngroups + gi] = rstd;
      }
    }
  }
}

// backward of the above.  partial row layout per workgroup: [dweight(width) | dbias(width)],
// width = dim (LN) or heads (GN).
template <typename T, int VEC, bool GN, bool SILU = false>
__global__ __launch_bounds__(kNormThreads) void norm_mul_bwd_kernel(const T* dy, const T* attn, const T* u, const T* w,
                                                                    const T* b, const float* mean_in,
                                                                    const float* rstd_in, T* dattn, T* du,
                                                                    float* partial, int64_t rows, int heads, int hdim,
                                                                    int concat, DropCtx dc, USrc us) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int dim = heads * hdim;
  const int nch = (dim + 64 * VEC - 1) / (64 * VEC);
  const int istride = concat ? 3 * dim : dim;
  const int ngroups = GN ? heads : 1;
  const int gdim = GN ? hdim : dim;
  float dw[max_chunks<VEC>()][VEC], db[max_chunks<VEC>()][VEC];   // LN: per column.  GN: slot [0][0..] unused, see ghw/ghb
#pragma unroll
  for (int k = 0; k < max_chunks<VEC>(); ++k)
#pragma unroll
    for (int i = 0; i < VEC; ++i) { dw[k][i] = 0.f; db[k][i] = 0.f; }
  float ghw[16], ghb[16];                             // GN: per-head partials (heads <= 16), lane-local
#pragma unroll
  for (int h = 0; h < 16; ++h) { ghw[h] = 0.f; ghb[h] = 0.f; }

  for (int64_t row = (int64_t)blockIdx.x * kNormWaves + wave; row < rows; row += (int64_t)gridDim.x * kNormWaves) {
    RowVec<T, VEC> xv[max_chunks<VEC>()], uv[max_chunks<VEC>()], gy[max_chunks<VEC>()];
    RowVec<T, VEC> up[SILU ? max_chunks<VEC>() : 1];   // SILU: the pre-activation (uv is reused for d u below)
    const T* dyrow = dy + row * istride;
#pragma unroll
    for (int k = 0; k < max_chunks<VEC>(); ++k) {
      const int c = (k * 64 + lane) * VEC;
      const bool ok = k < nch && c < dim;
      load_piece<T, VEC>(xv[k].v, attn + row * dim + c, ok);
      load_piece<T, VEC>(uv[k].v, u + row * us.u_stride + c, ok);
      if constexpr (SILU) { up[k] = uv[k]; silu_rounded<T, VEC>(uv[k]); }
      load_piece<T, VEC>(gy[k].v, dyrow + (concat ? 2 * dim : 0) + c, ok);
      if (dc.thr && ok) drop_apply<T, VEC>(gy[k], row * istride + (concat ? 2 * dim : 0) + c, dc);   // d y3 -> d y: same mask, same scale
    }
#pragma unroll
    for (int gi = 0; gi < 16; ++gi) {
      if (gi < ngroups) {
        const int lo = gi * gdim, hi = lo + gdim;
        const float mean = mean_in[row * ngroups + gi], rstd = rstd_in[row * ngroups + gi];
        float gw = 0.f, gb = 0.f;
        if (GN) { gw = (float)w[gi]; gb = (float)b[gi]; }
        float s1 = 0.f, s2 = 0.f, hw = 0.f, hb = 0.f;
        RowVec<T, VEC> gg[max_chunks<VEC>()], xh[max_chunks<VEC>()];
#pragma unroll
        for (int k = 0; k < max_chunks<VEC>(); ++k) {
          const int c = (k * 64 + lane) * VEC;
          const bool in = k < nch && c >= lo && c < hi;
          RowVec<T, VEC> wv, bv;
          if (!GN) { load_piece<T, VEC>(wv.v, w + c, in); load_piece<T, VEC>(bv.v, b + c, in); }
#pragma unroll
          for (int i = 0; i < VEC; ++i) {
            const float xhat = in ? (xv[k].v[i] - mean) * rstd : 0.f;
            const float gam = GN ? gw : wv.v[i];
            const float bet = GN ? gb : bv.v[i];
            const float dyu = in ? gy[k].v[i] * uv[k].v[i] : 0.f;   // d(norm out)
            xh[k].v[i] = xhat;
            gg[k].v[i] = dyu * gam;
            s1 += gg[k].v[i] * xhat;
            s2 += gg[k].v[i];
            if (GN) { hw += dyu * xhat; hb += dyu; }
            else if (in) { dw[k][i] += dyu * xhat; db[k][i] += dyu; }
            if (in) uv[k].v[i] = gy[k].v[i] * (gam * xhat + bet);      // du contribution dy * n_hat (reuses uv)
          }
        }
        if (GN) { ghw[gi] += hw; ghb[gi] += hb; }
        const float c1 = wave_sum(s1) / gdim, c2 = wave_sum(s2) / gdim;
#pragma unroll
        for (int k = 0; k < max_chunks<VEC>(); ++k) {
          const int c = (k * 64 + lane) * VEC;
          if (k < nch && c >= lo && c < hi) {
            RowVec<T, VEC> o, o2, e1, e2;
            if (concat) {
              load_piece<T, VEC>(e1.v, dyrow + c, true);          // d u   from the concat slot
              load_piece<T, VEC>(e2.v, dyrow + dim + c, true);    // d attn from the concat slot
              if (dc.thr) {
                drop_apply<T, VEC>(e1, row * istride + c, dc);
                drop_apply<T, VEC>(e2, row * istride + dim + c, dc);
              }
            }
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
              o.v[i] = rstd * (gg[k].v[i] - c2 - xh[k].v[i] * c1) + (concat ? e2.v[i] : 0.f);
              o2.v[i] = uv[k].v[i] + (concat ? e1.v[i] : 0.f);
            }
            store_vec<T, VEC>(o, dattn + row * dim + c);
            if constexpr (SILU) silu_grad_rounded<T, VEC>(o2, up[k]);
            store_vec<T, VEC>(o2, du + row * us.du_stride + c);
          }
        }
      }
    }
  }
  if (GN) {
    // per-head partials: reduce over the wave, then over the workgroup's waves
    float* out_row = partial + (int64_t)blockIdx.x * 2 * heads;
#pragma unroll
    for (int h = 0; h < 16; ++h) {
      if (h < heads) {
        const float a = wave_sum(ghw[h]), c = wave_sum(ghb[h]);
        if (lane == 0) { lds[wave * 32 + h] = a; lds[wave * 32 + 16 + h] = c; }
      }
    }
    __syncthreads();
    if (threadIdx.x < heads) {
      float a = 0.f, c = 0.f;
      for (int w2 = 0; w2 < kNormWaves; ++w2) { a += lds[w2 * 32 + threadIdx.x]; c += lds[w2 * 32 + 16 + threadIdx.x]; }
      out_row[threadIdx.x] = a;
      out_row[heads + threadIdx.x] = c;
    }
  } else {
    block_reduce_cols<VEC>(dw, lds, partial + (int64_t)blockIdx.x * 2 * dim, dim, nch);
    block_reduce_cols<VEC>(db, lds, partial + (int64_t)blockIdx.x * 2 * dim + dim, dim, nch);
  }
}

// ------------------------------------------------------------------ group norm * u, fast path
// Group norm with head_dim / VEC lanes per head (a power of two <= 64, e.g. 128 / 8 = 16): every lane's 16-byte
// piece lies inside ONE head, so all heads of a row are normalised at once with segmented (xor-shuffle) sums over
// the lanes of a head.  The general kernels above walk the heads one after the other with the other lanes
// masked (heads x the arithmetic) and fetch the concat slots in a second round trip per row.
HSTU_DEV float seg_sum(float x, int lanes_per_head) {
  for (int d = 1; d < lanes_per_head; d <<= 1) x += __shfl_xor(x, d, 64);
  return x;
}

template <typename T, int VEC, int MC = max_chunks<VEC>(), bool SILU = false>
__global__ __launch_bounds__(kNormThreads) void norm_mul_fwd_gn_kernel(const T* attn, const T* u, const T* w, const T* b,
                                                                       T* y, float* mean_out, float* rstd_out,
                                                                       int64_t rows, int heads, int hdim, float eps,
                                                                       int concat, DropCtx dc, USrc us) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int dim = heads * hdim;
  const int nch = (dim + 64 * VEC - 1) / (64 * VEC);
  const int lph = hdim / VEC;
  const int ostride = concat ? 3 * dim : dim;
  const float inv = 1.0f / hdim;
  // NORM_PREFETCH (single-chunk rows of 16-byte pieces): the next row's pieces are requested before this row is worked
  // on, so a wave always has a row in flight; the row past the end is a clamped re-read (no branch around the loads).
  constexpr bool kPre = NORM_PREFETCH && MC == 1 && VEC * sizeof(T) == 16;
  const int64_t row_step = (int64_t)gridDim.x * kNormWaves;
  const int c0 = lane * VEC < dim ? lane * VEC : 0;    // lanes past the row re-read its first piece (their results are dropped)
  u32x4 xr = {0, 0, 0, 0}, ur = {0, 0, 0, 0};
  if constexpr (kPre) {
    const int64_t r0 = (int64_t)blockIdx.x * kNormWaves + wave;
    if (r0 < rows) { xr = load_raw16(attn + r0 * dim + c0); ur = load_raw16(u + r0 * us.u_stride + c0); }
  }
  for (int64_t row = (int64_t)blockIdx.x * kNormWaves + wave; row < rows; row += row_step) {
    RowVec<T, VEC> xv[MC], uv[MC];
    if constexpr (kPre) {
      // (expanded first: the raw registers are dead before the next row's loads are issued, so the loop-carried pair
      // needs no copy at the back edge -- a copy of a register still being loaded would wait for the load right there)
      expand_raw16<T, VEC>(xv[0], xr);
      expand_raw16<T, VEC>(uv[0], ur);
      const int64_t nrow = row + row_step < rows ? row + row_step : row;
      xr = load_raw16(attn + nrow * dim + c0);
      ur = load_raw16(u + nrow * us.u_stride + c0);
    } else {
#pragma unroll
      for (int k = 0; k < MC; ++k) {
        const int c = (k * 64 + lane) * VEC;
        const bool ok = k < nch && c < dim;
        load_piece<T, VEC>(xv[k].v, attn + row * dim + c, ok);
        load_piece<T, VEC>(uv[k].v, u + row * us.u_stride + c, ok);
      }
    }
    if constexpr (SILU) {
#pragma unroll
      for (int k = 0; k < MC; ++k) silu_rounded<T, VEC>(uv[k]);
    }
#pragma unroll
    for (int k = 0; k < MC; ++k) {
      const int c = (k * 64 + lane) * VEC;
      if (k < nch) {               // wave-uniform; lanes past dim take part in the shuffles with zeros
        const bool ok = c < dim;
        const int h = ok ? c / hdim : 0;
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < VEC; ++i) s += xv[k].v[i];
        const float mean = seg_sum(s, lph) * inv;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < VEC; ++i) { const float d = xv[k].v[i] - mean; q += d * d; }
        const float rstd = 1.0f / sqrtf(seg_sum(q, lph) * inv + eps);
        if (ok) {
          const float gw = (float)w[h], gb = (float)b[h];
          RowVec<T, VEC> o;
#pragma unroll
          for (int i = 0; i < VEC; ++i) o.v[i] = uv[k].v[i] * ((xv[k].v[i] - mean) * rstd * gw + gb);
          T* yrow = y + row * ostride;
          if (concat) {
            if (dc.thr) {   // kernel-uniform
              drop_apply<T, VEC>(uv[k], row * ostride + c, dc);
              drop_apply<T, VEC>(xv[k], row * ostride + dim + c, dc);
              drop_apply<T, VEC>(o, row * ostride + 2 * dim + c, dc);
            }
            store_vec<T, VEC>(uv[k], yrow + c);
            store_vec<T, VEC>(xv[k], yrow + dim + c);
            store_vec<T, VEC>(o, yrow + 2 * dim + c);
          } else {
            if (dc.thr) drop_apply<T, VEC>(o, row * ostride + c, dc);
            store_vec<T, VEC>(o, yrow + c);
          }
          if (c % hdim == 0) {
            if (mean_out) mean_out[row * heads + h] = mean;
            if (rstd_out) rstd_out[row * heads + h] = rstd;
          }
        }
      }
    }
  }
}

// (single-chunk instance: 5 workgroups per CU asked for -- the SiLU variant sits at 98 registers, two above the 96 of a
// fifth wave per SIMD)
template <typename T, int VEC, int MC = max_chunks<VEC>(), bool SILU = false>
__global__ __launch_bounds__(kNormThreads, (MC == 1 ? 5 : 1)) void norm_mul_bwd_gn_kernel(const T* dy, const T* attn, const T* u, const T* w,
                                                                       const T* b, const float* mean_in,
                                                                       const float* rstd_in, T* dattn, T* du,
                                                                       float* partial, int64_t rows, int heads, int hdim,
                                                                       int concat, DropCtx dc, USrc us) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int dim = heads * hdim;
  const int nch = (dim + 64 * VEC - 1) / (64 * VEC);
  const int lph = hdim / VEC;
  const int istride = concat ? 3 * dim : dim;
  const float inv = 1.0f / hdim;
  // this lane's head per chunk never changes: its dweight / dbias partial sums stay in two registers per chunk
  float hw[MC], hb[MC], gw[MC], gb[MC];
  int head[MC];
#pragma unroll
  for (int k = 0; k < MC; ++k) {
    const int c = (k * 64 + lane) * VEC;
    const bool ok = k < nch && c < dim;
    head[k] = ok ? c / hdim : 0;
    gw[k] = ok ? (float)w[head[k]] : 0.f;
    gb[k] = ok ? (float)b[head[k]] : 0.f;
    hw[k] = 0.f;
    hb[k] = 0.f;
  }
  // NORM_PREFETCH: as in the forward kernel -- attn, u, d y and the two statistics of the next row are requested before
  // this row is worked on (the concat slots, when present, are read in the row's own iteration)
  constexpr bool kPre = NORM_PREFETCH && MC == 1 && VEC * sizeof(T) == 16;
  const int64_t row_step = (int64_t)gridDim.x * kNormWaves;
  const int c0 = lane * VEC < dim ? lane * VEC : 0;
  const int gy_off = concat ? 2 * dim : 0;
  u32x4 xr = {0, 0, 0, 0}, ur = {0, 0, 0, 0}, gr = {0, 0, 0, 0};
  float mr = 0.f, rr = 0.f;
  if constexpr (kPre) {
    const int64_t r0 = (int64_t)blockIdx.x * kNormWaves + wave;
    if (r0 < rows) {
      xr = load_raw16(attn + r0 * dim + c0);
      ur = load_raw16(u + r0 * us.u_stride + c0);
      gr = load_raw16(dy + r0 * istride + gy_off + c0);
      mr = mean_in[r0 * heads + head[0]];
      rr = rstd_in[r0 * heads + head[0]];
    }
  }
  for (int64_t row = (int64_t)blockIdx.x * kNormWaves + wave; row < rows; row += row_step) {
    RowVec<T, VEC> xv[MC], uv[MC], gy[MC], e1[MC], e2[MC];
    float mean[MC], rstd[MC];
    const T* dyrow = dy + row * istride;
    if constexpr (kPre) {
      const bool ok = lane * VEC < dim;
      expand_raw16<T, VEC>(xv[0], xr);
      expand_raw16<T, VEC>(uv[0], ur);
      expand_raw16<T, VEC>(gy[0], gr);
      mean[0] = ok ? mr : 0.f;
      rstd[0] = ok ? rr : 0.f;
      if (!ok) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) { xv[0].v[i] = 0.f; uv[0].v[i] = 0.f; gy[0].v[i] = 0.f; }
      }
      const int64_t nrow = row + row_step < rows ? row + row_step : row;
      xr = load_raw16(attn + nrow * dim + c0);
      ur = load_raw16(u + nrow * us.u_stride + c0);
      gr = load_raw16(dy + nrow * istride + gy_off + c0);
      mr = mean_in[nrow * heads + head[0]];
      rr = rstd_in[nrow * heads + head[0]];
      load_piece<T, VEC>(e1[0].v, dyrow + c0, ok && concat);           // d u    from the concat slot
      load_piece<T, VEC>(e2[0].v, dyrow + dim + c0, ok && concat);     // d attn from the concat slot
    } else {
#pragma unroll
      for (int k = 0; k < MC; ++k) {   // every load of the row is issued before anything is used
        const int c = (k * 64 + lane) * VEC;
        const bool ok = k < nch && c < dim;
        load_piece<T, VEC>(xv[k].v, attn + row * dim + c, ok);
        load_piece<T, VEC>(uv[k].v, u + row * us.u_stride + c, ok);
        load_piece<T, VEC>(gy[k].v, dyrow + (concat ? 2 * dim : 0) + c, ok);
        load_piece<T, VEC>(e1[k].v, dyrow + c, ok && concat);           // d u    from the concat slot
        load_piece<T, VEC>(e2[k].v, dyrow + dim + c, ok && concat);     // d attn from the concat slot
        mean[k] = ok ? mean_in[row * heads + head[k]] : 0.f;
        rstd[k] = ok ? rstd_in[row * heads + head[k]] : 0.f;
      }
    }
    PackedVec<T, VEC> up[SILU ? MC : 1];   // SILU: the pre-activation, kept (as T: half the registers) for SiLU' at the store
    if constexpr (SILU) {
#pragma unroll
      for (int k = 0; k < MC; ++k) { pack_vec<T, VEC>(up[k], uv[k]); silu_rounded<T, VEC>(uv[k]); }
    }
    if (dc.thr) {   // kernel-uniform: d y3 -> the gradients of the three slices before dropout (same masks, same scale)
#pragma unroll
      for (int k = 0; k < MC; ++k) {
        const int c = (k * 64 + lane) * VEC;
        if (k < nch && c < dim) {
          drop_apply<T, VEC>(gy[k], row * istride + (concat ? 2 * dim : 0) + c, dc);
          if (concat) {
            drop_apply<T, VEC>(e1[k], row * istride + c, dc);
            drop_apply<T, VEC>(e2[k], row * istride + dim + c, dc);
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < MC; ++k) {
      const int c = (k * 64 + lane) * VEC;
      if (k < nch) {
        const bool ok = c < dim;
        float s1 = 0.f, s2 = 0.f;
        RowVec<T, VEC> gg, xh, o, o2;
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          const float xhat = (xv[k].v[i] - mean[k]) * rstd[k];
          const float dyu = gy[k].v[i] * uv[k].v[i];               // d(norm out)
          xh.v[i] = xhat;
          gg.v[i] = dyu * gw[k];
          s1 += gg.v[i] * xhat;
          s2 += gg.v[i];
          hw[k] += dyu * xhat;
          hb[k] += dyu;
          o2.v[i] = gy[k].v[i] * (gw[k] * xhat + gb[k]) + e1[k].v[i];
        }
        const float c1 = seg_sum(s1, lph) * inv, c2 = seg_sum(s2, lph) * inv;
        if (ok) {
#pragma unroll
          for (int i = 0; i < VEC; ++i) o.v[i] = rstd[k] * (gg.v[i] - c2 - xh.v[i] * c1) + e2[k].v[i];
          store_vec<T, VEC>(o, dattn + row * dim + c);
          if constexpr (SILU) {
            RowVec<T, VEC> pre;
            unpack_vec<T, VEC>(pre, up[k]);
            silu_grad_rounded<T, VEC>(o2, pre);
          }
          store_vec<T, VEC>(o2, du + row * us.du_stride + c);
        }
      }
    }
  }
  // per-head partials: lanes of a head -> its first lane -> LDS[wave][head] (a head lives in exactly one chunk) ->
  // fixed-order sum over the waves
  for (int i = threadIdx.x; i < kNormWaves * 32; i += kNormThreads) lds[i] = 0.f;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < MC; ++k) {
    const int c = (k * 64 + lane) * VEC;
    if (k < nch) {
      const float a = seg_sum(hw[k], lph), cc = seg_sum(hb[k], lph);
      if (c < dim && c % hdim == 0) { lds[wave * 32 + head[k]] = a; lds[wave * 32 + 16 + head[k]] = cc; }
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < heads) {
    float a = 0.f, cc = 0.f;
    for (int w2 = 0; w2 < kNormWaves; ++w2) { a += lds[w2 * 32 + threadIdx.x]; cc += lds[w2 * 32 + 16 + threadIdx.x]; }
    float* out_row = partial + (int64_t)blockIdx.x * 2 * heads;
    out_row[threadIdx.x] = a;
    out_row[heads + threadIdx.x] = cc;
  }
}

// ------------------------------------------------------------------ SiLU on a column slice
template <typename T, bool BWD>
__global__ void silu_kernel(const T* dout, const T* in, T* out, int64_t rows, int cols, int64_t s_dout, int64_t s_in,
                            int64_t s_out) {
  const int64_t n = rows * cols;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / cols;
    const int c = (int)(i % cols);
    const float x = (float)in[r * s_in + c];
    if (BWD) out[r * s_out + c] = (T)silu_grad_val((float)dout[r * s_dout + c], x);
    else out[r * s_out + c] = (T)silu_val(x);
  }
}

// ------------------------------------------------------------------ host-side dispatch
// The launchers below take the class of the call (piece width, chunk class, group-norm path) from norm_ops.hip, which
// decided it -- and this instance, and whether the row is accepted at all -- with norm_dispatch.h; nothing is derived here.
using norm_dispatch::RowClass;

// Launch of a row kernel on the grid that is resident at once (nb: out, the bwd launchers hand it to the reduction).
// (kMaxNormBlocks = 2048 workgroups on 256 CUs ask for 8 per CU; a kernel of 69 registers holds 7 -- the 256 left over ran
// as a second round at one seventh of the occupancy.)
#define ROW_LAUNCH(NB, LDS, K, ...)                                                        \
  do {                                                                                     \
    NB = resident_row_blocks(K, kNormThreads, LDS, rows, kNormWaves, kMaxNormBlocks);      \
    hipLaunchKernelGGL(K, dim3(NB), dim3(kNormThreads), LDS, st, __VA_ARGS__);             \
  } while (0)

template <typename T, bool SWISH = false>
static int ln_fwd(const RowClass& cls, const void* x, const void* w, const void* b, void* y, float* mean, float* rstd,
                  int64_t rows, int dim, float eps, hipStream_t st) {
  const char* who = SWISH ? "swish_layer_norm_fwd" : "layer_norm_fwd";
  const int v = cls.vec;
  constexpr int VV = sizeof(T) == 2 ? 8 : 4;
  int nb;
#define LN_ARGS (const T*)x, (const T*)w, (const T*)b, (T*)y, mean, rstd, rows, dim, eps
  if (v == 1) ROW_LAUNCH(nb, 0, (layer_norm_fwd_kernel<T, 1, max_chunks<1>(), SWISH>), LN_ARGS);
  else if (cls.one_chunk) ROW_LAUNCH(nb, 0, (layer_norm_fwd_kernel<T, VV, 1, SWISH>), LN_ARGS);
  else ROW_LAUNCH(nb, 0, (layer_norm_fwd_kernel<T, VV, max_chunks<VV>(), SWISH>), LN_ARGS);
#undef LN_ARGS
  return check_launch(who);
}

template <typename T, bool SWISH = false>
static int ln_bwd(const RowClass& cls, const void* dy, const void* x, const void* w, const float* mean, const float* rstd,
                  void* dx, float* dweight, float* dbias, float* partial, int64_t rows, int dim, const void* dres,
                  hipStream_t st, const void* b = nullptr) {
  const char* who = SWISH ? "swish_layer_norm_bwd" : "layer_norm_bwd";
  const int v = cls.vec;
  constexpr int VV = sizeof(T) == 2 ? 8 : 4;
  const int nch = (dim + 64 * v - 1) / (64 * v);
  const size_t lds = (size_t)kNormWaves * nch * 64 * v * sizeof(float);
  int nb;
#define LN_ARGS (const T*)dy, (const T*)x, (const T*)w, mean, rstd, (T*)dx, partial, rows, dim, (const T*)dres, (const T*)b
  if (v == 1) ROW_LAUNCH(nb, lds, (layer_norm_bwd_kernel<T, 1, max_chunks<1>(), SWISH>), LN_ARGS);
  else if (cls.one_chunk) ROW_LAUNCH(nb, lds, (layer_norm_bwd_kernel<T, VV, 1, SWISH>), LN_ARGS);
  else ROW_LAUNCH(nb, lds, (layer_norm_bwd_kernel<T, VV, max_chunks<VV>(), SWISH>), LN_ARGS);
#undef LN_ARGS
  if (int e = check_launch(who)) return e;
  hipLaunchKernelGGL(reduce_partials_kernel, dim3(2 * dim), dim3(256), 0, st, partial, nb, dim, dweight, dbias);
  return check_launch(who);
}

template <typename T>
static int rms_fwd(const RowClass& cls, const void* x, const void* w, void* y, float* rstd, int64_t rows, int dim, float eps,
                   hipStream_t st) {
  constexpr int VV = sizeof(T) == 2 ? 8 : 4;
  int nb;
#define RMS_ARGS (const T*)x, (const T*)w, (T*)y, rstd, rows, dim, eps
  if (cls.vec == 1) ROW_LAUNCH(nb, 0, (rms_norm_fwd_kernel<T, 1, max_chunks<1>()>), RMS_ARGS);
  else if (cls.one_chunk) ROW_LAUNCH(nb, 0, (rms_norm_fwd_kernel<T, VV, 1>), RMS_ARGS);
  else ROW_LAUNCH(nb, 0, (rms_norm_fwd_kernel<T, VV, max_chunks<VV>()>), RMS_ARGS);
#undef RMS_ARGS
  return check_launch("rms_norm_fwd");
}

template <typename T>
static int rms_bwd(const RowClass& cls, const void* dy, const void* x, const void* w, const float* rstd, void* dx,
                   float* dweight, float* partial, int64_t rows, int dim, hipStream_t st) {
  const int v = cls.vec;
  constexpr int VV = sizeof(T) == 2 ? 8 : 4;
  const int nch = (dim + 64 * v - 1) / (64 * v);
  const size_t lds = (size_t)kNormWaves * nch * 64 * v * sizeof(float);
  int nb;
#define RMS_ARGS (const T*)dy, (const T*)x, (const T*)w, rstd, (T*)dx, partial, rows, dim
  if (v == 1) ROW_LAUNCH(nb, lds, (rms_norm_bwd_kernel<T, 1, max_chunks<1>()>), RMS_ARGS);
  else if (cls.one_chunk) ROW_LAUNCH(nb, lds, (rms_norm_bwd_kernel<T, VV, 1>), RMS_ARGS);
  else ROW_LAUNCH(nb, lds, (rms_norm_bwd_kernel<T, VV, max_chunks<VV>()>), RMS_ARGS);
#undef RMS_ARGS
  if (int e = check_launch("rms_norm_bwd")) return e;
  // the weight half of the partial rows only: `dim` columns of the 2 * dim wide matrix, no bias output
  hipLaunchKernelGGL(reduce_partials_kernel, dim3(dim), dim3(256), 0, st, partial, nb, dim, dweight, (float*)nullptr);
  return check_launch("rms_norm_bwd(reduce)");
}

template <typename T>
static int nm_fwd(const RowClass& cls, const void* attn, const void* u, const void* w, const void* b, void* y, float* mean, float* rstd,
                  int64_t rows, int heads, int hdim, float eps, int gn, int concat, DropCtx dc, int64_t u_stride, bool silu,
                  hipStream_t st) {
  const int v = cls.vec;
  const USrc us{u_stride, 0};
  if (gn && heads > 16) return set_error(HSTU_EUNSUPPORTED, "norm_mul: group norm supports at most 16 heads");
  constexpr int VV = sizeof(T) == 2 ? 8 : 4;
  int nb;
#define NM_ARGS (const T*)attn, (const T*)u, (const T*)w, (const T*)b, (T*)y, mean, rstd, rows, heads, hdim, eps, concat, dc, us
#define NM_PICK(S)                                                                                                              \
  if (cls.gn_fast && cls.one_chunk) ROW_LAUNCH(nb, 0, (norm_mul_fwd_gn_kernel<T, VV, 1, S>), NM_ARGS);              \
  else if (cls.gn_fast) ROW_LAUNCH(nb, 0, (norm_mul_fwd_gn_kernel<T, VV, max_chunks<VV>(), S>), NM_ARGS);            \
  else if (v == 1 && gn) ROW_LAUNCH(nb, 0, (norm_mul_fwd_kernel<T, 1, true, S>), NM_ARGS);                                         \
  else if (v == 1) ROW_LAUNCH(nb, 0, (norm_mul_fwd_kernel<T, 1, false, S>), NM_ARGS);                                              \
  else if (gn) ROW_LAUNCH(nb, 0, (norm_mul_fwd_kernel<T, VV, true, S>), NM_ARGS);                                                  \
  else ROW_LAUNCH(nb, 0, (norm_mul_fwd_kernel<T, VV, false, S>), NM_ARGS)
  if (silu) { NM_PICK(true); } else { NM_PICK(false); }
#undef NM_PICK
#undef NM_ARGS
  return check_launch("norm_mul_fwd");
}

template <typename T>
static int nm_bwd(const RowClass& cls, const void* dy, const void* attn, const void* u, const void* w, const void* b, const float* mean,
                  const float* rstd, void* dattn, void* du, float* dweight, float* dbias, float* partial, int64_t rows,
                  int heads, int hdim, int gn, int concat, DropCtx dc, int64_t u_stride, int64_t du_stride, bool silu,
                  hipStream_t st) {
  const int dim = heads * hdim;
  const int v = cls.vec;
  const USrc us{u_stride, du_stride};
  if (gn && heads > 16) return set_error(HSTU_EUNSUPPORTED, "norm_mul: group norm supports at most 16 heads");
  constexpr int VV = sizeof(T) == 2 ? 8 : 4;
  const int nch = (dim + 64 * v - 1) / (64 * v);
  const size_t lds = gn ? kNormWaves * 32 * sizeof(float) : (size_t)kNormWaves * nch * 64 * v * sizeof(float);
  int nb;
#define NM_ARGS (const T*)dy, (const T*)attn, (const T*)u, (const T*)w, (const T*)b, mean, rstd, (T*)dattn, (T*)du, partial, rows, heads, hdim, concat, dc, us
#define NM_PICK(S)                                                                                                              \
  if (cls.gn_fast && cls.one_chunk) ROW_LAUNCH(nb, lds, (norm_mul_bwd_gn_kernel<T, VV, 1, S>), NM_ARGS);            \
  else if (cls.gn_fast) ROW_LAUNCH(nb, lds, (norm_mul_bwd_gn_kernel<T, VV, max_chunks<VV>(), S>), NM_ARGS);          \
  else if (v == 1 && gn) ROW_LAUNCH(nb, lds, (norm_mul_bwd_kernel<T, 1, true, S>), NM_ARGS);                                       \
  else if (v == 1) ROW_LAUNCH(nb, lds, (norm_mul_bwd_kernel<T, 1, false, S>), NM_ARGS);                                            \
  else if (gn) ROW_LAUNCH(nb, lds, (norm_mul_bwd_kernel<T, VV, true, S>), NM_ARGS);                                                \
  else ROW_LAUNCH(nb, lds, (norm_mul_bwd_kernel<T, VV, false, S>), NM_ARGS)
  if (silu) { NM_PICK(true); } else { NM_PICK(false); }
#undef NM_PICK
#undef NM_ARGS
  if (int e = check_launch("norm_mul_bwd")) return e;
  const int width = gn ? heads : dim;
  hipLaunchKernelGGL(reduce_partials_kernel, dim3(2 * width), dim3(256), 0, st, partial, nb, width, dweight, dbias);
  return check_launch("norm_mul_bwd(reduce)");
}

// 16 bytes per lane: a row of the column slice is `cols / VEC` pieces; used when the slice start, the row strides
// and the width are all 16-byte multiples (the u slice of the fused uvqk buffer is)
template <typename T, bool BWD>
__global__ __launch_bounds__(256) void silu_vec_kernel(const T* dout, const T* in, T* out, int64_t rows, int cols,
                                                       int64_t s_dout, int64_t s_in, int64_t s_out) {
  constexpr int VEC = 16 / sizeof(T);
  const int ppr = cols / VEC;                               // pieces per row
  const int64_t n = rows * ppr;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / ppr;
    const int c = (int)(i - r * ppr) * VEC;
    RowVec<T, VEC> x, g, o;
    load_piece<T, VEC>(x.v, in + r * s_in + c, true);
    if (BWD) load_piece<T, VEC>(g.v, dout + r * s_dout + c, true);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      o.v[k] = BWD ? silu_grad_val(g.v[k], x.v[k]) : silu_val(x.v[k]);
    }
    store_vec<T, VEC>(o, out + r * s_out + c);
  }
}

template <typename T, bool BWD>
static int silu_launch(bool vec_ok, const void* dout, const void* in, void* out, int64_t rows, int cols, int64_t s0,
                       int64_t s1, int64_t s2, hipStream_t st) {
  const int64_t n = rows * cols;
  if (n == 0) return HSTU_OK;
  constexpr int VEC = 16 / sizeof(T);
  if (vec_ok) {
    const int64_t pieces = n / VEC;
    int blocks = (int)((pieces + 255) / 256);
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL((silu_vec_kernel<T, BWD>), dim3(blocks), dim3(256), 0, st, (const T*)dout, (const T*)in, (T*)out, rows, cols, s0, s1, s2);
    return check_launch("silu");
  }
  int blocks = (int)((n + 255) / 256);
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL((silu_kernel<T, BWD>), dim3(blocks), dim3(256), 0, st, (const T*)dout, (const T*)in, (T*)out, rows, cols, s0, s1, s2);
  return check_launch("silu");
}

// ------------------------------------------------------------------ row L2 normalisation (output postprocessor)
// y = x / max(||x||_2, eps)   (modules/postprocessors.py:55-69: seq / linalg.norm(seq).clamp(min=1e-6)), one wave per
// row, fp32 math.  Backward: with n = ||x||: n > eps -> dx = (g - y <y, g>) / n;  n <= eps (the clamp is active and
// has zero gradient) -> dx = g / eps.
template <typename T, int VEC, bool BWD>
__global__ __launch_bounds__(kNormThreads) void l2_norm_kernel(const T* x, const T* g, T* out, int64_t rows, int dim, float eps) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nch = (dim + 64 * VEC - 1) / (64 * VEC);
  for (int64_t row = (int64_t)blockIdx.x * kNormWaves + wave; row < rows; row += (int64_t)gridDim.x * kNormWaves) {
    RowVec<T, VEC> xv[max_chunks<VEC>()], gv[max_chunks<VEC>()];
    float ss = 0.f, dot = 0.f;
#pragma unroll
    for (int k = 0; k < max_chunks<VEC>(); ++k) {
      const int c = (k * 64 + lane) * VEC;
      const bool ok = k < nch && c < dim;
      load_piece<T, VEC>(xv[k].v, x + row * dim + c, ok);
      if (BWD) load_piece<T, VEC>(gv[k].v, g + row * dim + c, ok);
#pragma unroll
      for (int i = 0; i < VEC; ++i) { ss += xv[k].v[i] * xv[k].v[i]; if (BWD) dot += xv[k].v[i] * gv[k].v[i]; }
    }
    const float n = sqrtf(wave_sum(ss));
    const bool clamped = n <= eps;
    const float inv = 1.0f / fmaxf(n, eps);
    float coef = 0.f;
    if (BWD) coef = clamped ? 0.f : wave_sum(dot) * inv * inv * inv;   // <y, g> / n * (1/n) applied to x
#pragma unroll
    for (int k = 0; k < max_chunks<VEC>(); ++k) {
      const int c = (k * 64 + lane) * VEC;
      if (k < nch && c < dim) {
        RowVec<T, VEC> o;
#pragma unroll
        for (int i = 0; i < VEC; ++i) o.v[i] = BWD ? gv[k].v[i] * inv - xv[k].v[i] * coef : xv[k].v[i] * inv;
        store_vec<T, VEC>(o, out + row * dim + c);
      }
    }
  }
}

template <typename T, bool BWD>
static int l2_launch(const RowClass& cls, const void* x, const void* g, void* out, int64_t rows, int dim, float eps,
                     hipStream_t st) {
  const int v = cls.vec;
  int nb;
  constexpr int VV = sizeof(T) == 2 ? 8 : 4;
  if (v == 1) ROW_LAUNCH(nb, 0, (l2_norm_kernel<T, 1, BWD>), (const T*)x, (const T*)g, (T*)out, rows, dim, eps);
  else ROW_LAUNCH(nb, 0, (l2_norm_kernel<T, VV, BWD>), (const T*)x, (const T*)g, (T*)out, rows, dim, eps);
  return check_launch("l2_norm");
}

