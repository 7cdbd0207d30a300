// xflow-amd: device code shared by the candidate-pool kernels (kernels_pool.hip:
// the score matrix; kernels_pool_topk.hip: score and select in one kernel;
// kernels_pool_subset.hip and kernels_pool_cross.hip: a request's own list).
// Included by .hip files only.
#pragma once
#include "hip_util.h"
#include "rank_common.h"

namespace xflow {
namespace hip {

constexpr int kPoolTileM = 32;     // requests per block (the instruction's M)
constexpr int kPoolRowWaves = 4;   // rows per workgroup of the row kernels

using f32x16 = __attribute__((ext_vector_type(16))) float;

// word k of a part's operand: A (ctx) = {g * u, c, 1, 0 ..}, B = {u, 1, c, 0 ..}
__device__ __forceinline__ float pool_operand(const float* v, int k, int Dk, bool ctx, float g) {
  if (k < Dk) return ctx ? __fmul_rn(g, v[1 + k]) : v[1 + k];
  if (k == Dk + (ctx ? 0 : 1)) return v[0];
  return k == Dk + (ctx ? 1 : 0) ? 1.0f : 0.0f;
}

// this lane's share of row rs: occurrences lane, lane + 64, ..
__device__ __forceinline__ RowSpan pool_lane_span(const RowSpan& rs, int lane) {
  RowSpan s;
  s.base = rs.base + (int64_t)lane * rs.step;
  s.step = rs.step * kWave;
  s.len = lane < rs.len ? (rs.len - lane + kWave - 1) / kWave : 0;
  return s;
}

// k_pool_rows_fm's end: the lanes' sums meet in the fixed butterfly, lane 0
// finishes them as the model finishes a row and lane j < W stores word j
template <int D>
__device__ __forceinline__ void pool_rows_fm_store(const PoolRowsArgs& a, int64_t r, int lane,
                                                   float wx, float (&vs)[D], float vp) {
  wx = rank_allsum(wx);
  vp = rank_allsum(vp);
#pragma unroll
  for (int k = 0; k < D; ++k) vs[k] = rank_allsum(vs[k]);
  float out = lane == 0 ? rank_fm_finish<D>(a.model.fm_math, wx, vs, vp) : 0.0f;
  const bool standard = a.model.fm_math == kFmStandard;
  if (standard) {
#pragma unroll
    for (int k = 0; k < D; ++k)
      if (lane == 1 + k) out = vs[k];
  } else {
    float vsum = 0.0f;  // (rank_fm_finish's own sum)
#pragma unroll
    for (int k = 0; k < D; ++k) vsum = __fadd_rn(vsum, vs[k]);
    if (lane == 1) out = vsum;
  }
  const int W = (1 + (standard ? D : 1) + 3) & ~3;
  if (lane < W) a.vec[r * W + lane] = out;
}

// pool subsets: the vector width of KP's models, and the float4 slot of part p
// of row r in a wave's staging region (kernels_pool_subset.hip has the layout)
constexpr int pool_subset_width(int KP) { return (KP + 2) & ~3; }  // pool_width of KP's models
template <int Q>
__device__ __forceinline__ int pool_subset_slot(int r, int p) {
  return r * Q + (Q % 2 == 0 ? p ^ ((r >> 3) & (Q - 1)) : p);
}

}  // namespace hip
}  // namespace xflow
