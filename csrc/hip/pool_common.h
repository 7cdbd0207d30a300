// xflow-amd: device code shared by the candidate-pool kernels (kernels_pool.hip:
// the score matrix; kernels_pool_topk.hip: score and select in one kernel).
// Included by .hip files only.
#pragma once
#include "hip_util.h"

namespace xflow {
namespace hip {

constexpr int kPoolTileM = 32;     // requests per block (the instruction's M)

using f32x16 = __attribute__((ext_vector_type(16))) float;

// word k of a part's operand: A (ctx) = {g * u, c, 1, 0 ..}, B = {u, 1, c, 0 ..}
__device__ __forceinline__ float pool_operand(const float* v, int k, int Dk, bool ctx, float g) {
  if (k < Dk) return ctx ? __fmul_rn(g, v[1 + k]) : v[1 + k];
  if (k == Dk + (ctx ? 0 : 1)) return v[0];
  return k == Dk + (ctx ? 1 : 0) ? 1.0f : 0.0f;
}

}  // namespace hip
}  // namespace xflow
