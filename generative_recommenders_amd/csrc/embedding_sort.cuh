// The sort in front of the embedding gradient (embedding_grad.hip) and the in-backward Adagrad (embedding_optim.hip):
// table indices grouped by a rocPRIM radix sort over only the ceil(log2(table_rows)) significant key bits, 32-bit keys and
// 32-bit row numbers from a counting iterator; stable, so the duplicates of an index stay in batch order.  (Its own header:
// rocPRIM stays out of capi_internal.h, which every translation unit includes.)
#pragma once
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

namespace hstu {

inline unsigned sort_key_bits(int table_rows) {
  unsigned bits = 1;
  while ((1u << bits) < (unsigned)table_rows && bits < 31) ++bits;
  return bits;
}

// idx (n) -> sorted_idx and perm, the row number of every sorted position.  temp == nullptr: only temp_bytes is set.
inline hipError_t sort_indices(void* temp, size_t& temp_bytes, const int32_t* idx, int32_t* sorted_idx, int32_t* perm, int64_t n,
                               int table_rows, hipStream_t st) {
  rocprim::counting_iterator<int32_t> rows(0);
  return rocprim::radix_sort_pairs(temp, temp_bytes, idx, sorted_idx, rows, perm, (size_t)n, 0u, sort_key_bits(table_rows), st);
}

inline size_t sort_temp_bytes(int64_t n, int table_rows) {
  size_t bytes = 0;
  (void)sort_indices(nullptr, bytes, nullptr, nullptr, nullptr, n, table_rows, (hipStream_t)0);
  return bytes;
}

}  // namespace hstu
