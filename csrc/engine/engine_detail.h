// xflow-amd: what two of the engine's source files need and no header should show.
#pragma once
#include <cstdint>

namespace xflow {
inline uint64_t next_pow2(uint64_t v) {
  uint64_t p = 1;
  while (p < v) p <<= 1;
  return p;
}
}  // namespace xflow
