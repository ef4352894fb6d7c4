// The copy width of the jagged byte-copy kernels (jagged_ops.hip), decided on the host.  Plain C++ with no HIP in it:
// tests/test_host_logic.py compiles it alone and checks it against the restated rule and the class table of
// tests/jagged_class_cases.py -- the hardware serves a misaligned vector access, so a width picked too wide shows in no
// output and can only be seen here.
#pragma once
#include <cstdint>

namespace hstu {
namespace jagged_dispatch {

// the widest vector (16, 8, 4, 2 or 1 bytes) that divides the row size and every base pointer: rows lie row_bytes apart,
// so every row of every tensor is then aligned to it.  A NULL pointer (a role the kernel does not have) constrains nothing.
inline int pick_vec(int row_bytes, const void* a, const void* b, const void* c) {
  uintptr_t bits = (uintptr_t)row_bytes | (uintptr_t)a | (uintptr_t)b | (uintptr_t)c;
  if ((bits & 15) == 0) return 16;
  if ((bits & 7) == 0) return 8;
  if ((bits & 3) == 0) return 4;
  if ((bits & 1) == 0) return 2;
  return 1;
}

}  // namespace jagged_dispatch
}  // namespace hstu
