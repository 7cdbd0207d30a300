// xflow-amd: device code shared by the candidate-pool kernels (kernels_pool.hip:
// the score matrix; kernels_pool_topk.hip: score and select in one kernel;
// kernels_pool_subset.hip and kernels_pool_cross.hip: a request's own list;
// kernels_pool_subset_topk.hip: that list scored and selected in one kernel).
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

// pool row i (-1: none, zeros) of this lane into bv.  STAGED: the wave's 64
// rows are loaded together, whole rows per instruction, into its LDS region
// `mine` (64 * Q float4s) and lane l reads row l back; the barrier inside is
// for every thread of the workgroup.  Otherwise the lane's own Q loads: the
// same values either way.
template <int Q, bool STAGED>
__device__ __forceinline__ void pool_subset_gather(const float4* pool4, int i, int lane,
                                                   float4* mine, float (&bv)[4 * Q]) {
  if constexpr (STAGED) {
#pragma unroll
    for (int j = 0; j < Q; ++j) {
      const int t = lane + kWave * j, r = t / Q, p = t % Q;
      const int ri = __shfl(i, r);
      mine[pool_subset_slot<Q>(r, p)] =
          ri >= 0 ? pool4[(int64_t)ri * Q + p] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();  // (every thread of the workgroup is here)
#pragma unroll
    for (int p = 0; p < Q; ++p) {
      const float4 v = mine[pool_subset_slot<Q>(lane, p)];
      bv[4 * p] = v.x, bv[4 * p + 1] = v.y, bv[4 * p + 2] = v.z, bv[4 * p + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int p = 0; p < Q; ++p) {
      const float4 v = i >= 0 ? pool4[(int64_t)i * Q + p] : make_float4(0.f, 0.f, 0.f, 0.f);
      bv[4 * p] = v.x, bv[4 * p + 1] = v.y, bv[4 * p + 2] = v.z, bv[4 * p + 3] = v.w;
    }
  }
}

// PoolSubsetArgs' score of one pair: the context vector at ctx4 against the
// pool row in bv, acc = fma(A[k], B[k], acc) over pool_operand's words from
// 0.0f, then sigmoid_ref
template <int KP>
__device__ __forceinline__ float pool_subset_score(const float4* ctx4,
                                                   const float (&bv)[pool_subset_width(KP)], int Dk,
                                                   float g) {
  constexpr int W = pool_subset_width(KP), Q = W / 4;
  float av[W];
#pragma unroll
  for (int p = 0; p < Q; ++p) {
    const float4 v = ctx4[p];
    av[4 * p] = v.x, av[4 * p + 1] = v.y, av[4 * p + 2] = v.z, av[4 * p + 3] = v.w;
  }
  float acc = 0.0f;
#pragma unroll
  for (int k = 0; k < KP; ++k)  // (constant k: av and bv stay in registers)
    if (k < Dk + 2)
      acc = __fmaf_rn(pool_operand(av, k, Dk, true, g), pool_operand(bv, k, Dk, false, g), acc);
  return sigmoid_ref(acc);
}

}  // namespace hip
}  // namespace xflow
