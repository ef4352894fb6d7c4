// Which instantiation of a row kernel (norm_kernels.inc) a call runs.  Host-only, plain C++: norm_ops.hip decides here,
// once per call, and hands the result to the launchers; tests/test_norm_dispatch_host.py compiles this header alone.
//
// Order of the decision:
//   1. piece width -- the 16-byte vector (8 x 16-bit, 4 x fp32) iff EVERY fact allows it: dim % V == 0, every pointer the
//      kernel touches in 16-byte pieces is 16-byte aligned, the u / du row strides are 16-byte multiples and, with group
//      norm, head_dim % V == 0 (a piece must not straddle two heads); otherwise scalar (1 element per piece);
//   2. instance -- wide (nw4) iff dim exceeds what the narrow instance (nw1) holds in registers AT THAT WIDTH
//      (1024 vector, 512 scalar);
//   3. refusal -- only when dim exceeds what the wide instance holds at that width (4096 vector, 2048 scalar).
#pragma once
#include <cstdint>

namespace hstu {
namespace norm_dispatch {

// elements of a row that the lanes of one wavefront hold in registers: 64 lanes x pieces per lane x piece width
// (pieces per lane of the narrow instance: 2 of 8 x 16-bit, 4 of 4 x fp32, 8 scalars; the wide instance holds 4 x that)
constexpr int pieces_per_lane(int vec, bool wide) { return (wide ? 4 : 1) * (vec == 8 ? 2 : (vec == 4 ? 4 : 8)); }
constexpr int capacity(int vec, bool wide) { return 64 * vec * pieces_per_lane(vec, wide); }

struct RowClass {
  int vec;          // piece width in elements: 16 / elem_bytes, or 1
  bool wide;        // the nw4 instance
  bool one_chunk;   // vector rows of up to 64 pieces: the MC = 1 instantiations
  bool gn_fast;     // group norm, every piece inside one head and head_dim / vec a power of two <= 64: the segmented kernels
  int limit;        // the largest dim accepted at this width (dim > limit is refused; the number in the message)
};

// the facts of one call, gathered with ptr() / stride() by the per-op functions below
struct Facts {
  int dim;
  int elem_bytes;
  uintptr_t addr_bits = 0;   // OR of every pointer read or written in 16-byte pieces (NULL = absent = aligned)
  int64_t stride_bits = 0;   // OR of the row strides (elements) that are not `dim` by construction
  bool group_norm = false;
  int head_dim = 0;
  Facts(int dim_, int elem_bytes_) : dim(dim_), elem_bytes(elem_bytes_) {}
  Facts& ptr(const void* p) { addr_bits |= (uintptr_t)p; return *this; }
  Facts& stride(int64_t s) { stride_bits |= s; return *this; }
  Facts& heads_of(int hd) { group_norm = true; head_dim = hd; return *this; }
};

inline RowClass decide(const Facts& f) {
  const int V = 16 / f.elem_bytes;
  bool vector = f.dim % V == 0 && (f.addr_bits & 15) == 0 && (f.stride_bits * (int64_t)f.elem_bytes) % 16 == 0;
  if (vector && f.group_norm && f.head_dim % V) vector = false;
  RowClass k;
  k.vec = vector ? V : 1;
  k.wide = f.dim > capacity(k.vec, false);
  k.one_chunk = vector && f.dim <= 64 * V;
  k.gn_fast = false;
  if (f.group_norm && vector) {
    const int lph = f.head_dim / V;   // lanes per head
    k.gn_fast = lph <= 64 && (lph & (lph - 1)) == 0;
  }
  k.limit = capacity(k.vec, true);
  return k;
}
inline bool refused(const RowClass& k, int dim) { return dim > k.limit; }

// ---- one function per launcher: the pointers and strides ITS kernels touch in pieces ----
// (group norm reads weight / bias as one scalar per head: their alignment does not matter there)
inline RowClass ln_fwd_class(int dim, int elem_bytes, const void* x, const void* w, const void* b, const void* y) {
  return decide(Facts(dim, elem_bytes).ptr(x).ptr(w).ptr(b).ptr(y));
}
// b: swish layer norm only (else NULL); dres: the fused residual gradient (else NULL)
inline RowClass ln_bwd_class(int dim, int elem_bytes, const void* dy, const void* x, const void* w, const void* b,
                             const void* dres, const void* dx) {
  return decide(Facts(dim, elem_bytes).ptr(dy).ptr(x).ptr(w).ptr(b).ptr(dres).ptr(dx));
}
// RMS norm: layer norm's classes without the bias (and without a fused residual)
inline RowClass rms_fwd_class(int dim, int elem_bytes, const void* x, const void* w, const void* y) {
  return decide(Facts(dim, elem_bytes).ptr(x).ptr(w).ptr(y));
}
inline RowClass rms_bwd_class(int dim, int elem_bytes, const void* dy, const void* x, const void* w, const void* dx) {
  return decide(Facts(dim, elem_bytes).ptr(dy).ptr(x).ptr(w).ptr(dx));
}
inline RowClass nm_fwd_class(int heads, int head_dim, int elem_bytes, bool group_norm, const void* attn, const void* u,
                             int64_t u_stride, const void* w, const void* b, const void* y) {
  Facts f(heads * head_dim, elem_bytes);
  f.ptr(attn).ptr(u).ptr(y).stride(u_stride);
  if (group_norm) f.heads_of(head_dim);
  else f.ptr(w).ptr(b);
  return decide(f);
}
inline RowClass nm_bwd_class(int heads, int head_dim, int elem_bytes, bool group_norm, const void* dy, const void* attn,
                             const void* u, int64_t u_stride, const void* w, const void* b, const void* dattn,
                             const void* du, int64_t du_stride) {
  Facts f(heads * head_dim, elem_bytes);
  f.ptr(dy).ptr(attn).ptr(u).ptr(dattn).ptr(du).stride(u_stride).stride(du_stride);
  if (group_norm) f.heads_of(head_dim);
  else f.ptr(w).ptr(b);
  return decide(f);
}
// g: the backward's incoming gradient (forward: NULL)
inline RowClass l2_class(int dim, int elem_bytes, const void* x, const void* g, const void* out) {
  return decide(Facts(dim, elem_bytes).ptr(x).ptr(g).ptr(out));
}
// the timestamp postprocessor's row pass (time_ln_ops.hip): z0 / y (dy / z0 / dz) rows in `elem_bytes` elements; b, wt,
// ln_w, ln_b are fp32 and read in 16-byte pieces whenever the rows are, so their alignment is a fact of the call too
// (dim % V == 0 keeps every row of wt aligned).  The backward's lanes hold one chunk whatever the width: it uses the
// piece width and the limit of its class.
inline RowClass time_ln_fwd_class(int dim, int elem_bytes, const void* z0, const void* b, const void* wt, const void* ln_w,
                                  const void* ln_b, const void* y) {
  return decide(Facts(dim, elem_bytes).ptr(z0).ptr(b).ptr(wt).ptr(ln_w).ptr(ln_b).ptr(y));
}
inline RowClass time_ln_bwd_class(int dim, int elem_bytes, const void* dy, const void* z0, const void* b, const void* wt,
                                  const void* ln_w, const void* dz) {
  return decide(Facts(dim, elem_bytes).ptr(dy).ptr(z0).ptr(b).ptr(wt).ptr(ln_w).ptr(dz));
}
// SiLU on a column slice is not register-resident (any width): the only choice is 16-byte pieces or scalars.
// dout / s_dout: the backward's incoming gradient (forward: NULL / 0)
inline bool silu_vector(int elem_bytes, int cols, const void* dout, const void* in, const void* out, int64_t s_dout,
                        int64_t s_in, int64_t s_out) {
  const int V = 16 / elem_bytes;
  return cols % V == 0 && s_dout % V == 0 && s_in % V == 0 && s_out % V == 0 &&
         ((((uintptr_t)dout | (uintptr_t)in | (uintptr_t)out) & 15) == 0);
}

}  // namespace norm_dispatch
}  // namespace hstu
