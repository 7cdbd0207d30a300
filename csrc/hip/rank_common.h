// xflow-amd: device code shared by the ranking kernels (kernels_rank.hip: the
// plain models; kernels_rank_cross.hip: models with feature crosses).
// Included by .hip files only.
#pragma once
#include "serve_common.h"

namespace xflow {
namespace hip {

// the same bits in every lane: Σ over the wave in a fixed butterfly
__device__ __forceinline__ float rank_allsum(float v) {
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) v = __fadd_rn(v, __shfl_xor(v, o));
  return v;
}

// Calls f(c0, c1, lo, hi) for every request with candidate rows [lo, hi)
// inside the tile [t0, t0 + kServeBlock): [c0, c1) is the request's context in
// ctx_keys, clamped to [0, ctx_nnz].  Wave-uniform; every lane takes part.
template <typename F>
__device__ __forceinline__ void rank_request_walk(const RankArgs& a, int64_t t0, F&& f) {
  const int64_t tend = t0 + kServeBlock < a.cands.rows ? t0 + kServeBlock : a.cands.rows;
  int64_t l0 = 0, l1 = a.R;  // first request that ends past the tile's first row
  while (l0 < l1) {
    const int64_t m = (l0 + l1) >> 1;
    if ((int64_t)a.req_ptr[m + 1] > t0) l1 = m;
    else l0 = m + 1;
  }
  for (int64_t q = l0; q < a.R; ++q) {
    int64_t lo = a.req_ptr[q], hi = a.req_ptr[q + 1];
    if (lo >= tend) break;
    lo = lo > t0 ? lo : t0;
    hi = hi < tend ? hi : tend;
    if (hi <= lo) continue;  // (no candidates: the context is never probed)
    int64_t c0 = a.ctx_ptr[q], c1 = a.ctx_ptr[q + 1];
    c0 = c0 < 0 ? 0 : (c0 > a.ctx_nnz ? a.ctx_nnz : c0);
    c1 = c1 < c0 ? c0 : (c1 > a.ctx_nnz ? a.ctx_nnz : c1);
    f(c0, c1, lo, hi);
  }
}

// this lane's share of the context [c0, c1): occurrences lane, lane + 64, ..
__device__ __forceinline__ RowSpan rank_ctx_span(int64_t c0, int64_t c1) {
  const int64_t lane = threadIdx.x;
  RowSpan cs;
  cs.base = c0 + lane;
  cs.step = kWave;
  cs.len = lane < c1 - c0 ? (int)((c1 - c0 - lane + kWave - 1) / kWave) : 0;
  return cs;
}

// Calls f(cs, lo, hi) for every request with candidate rows [lo, hi) inside
// the tile: cs is this lane's share of the request's context.  Wave-uniform
// but for cs; every lane of the wave takes part.
template <typename F>
__device__ __forceinline__ void rank_requests(const RankArgs& a, int64_t t0, F&& f) {
  rank_request_walk(a, t0, [&](int64_t c0, int64_t c1, int64_t lo, int64_t hi) {
    f(rank_ctx_span(c0, c1), lo, hi);
  });
}

// FM full rows (k_fm's sums): per occurrence of rs wx += w, then vs[k] += v_k
// and vp += v_k * v_k for k in order, continuing whatever the accumulators hold.
template <int D>
__device__ __forceinline__ void rank_fm_sum(const TableView& t, const OptSpec& o, const u64* keys,
                                            const RowSpan& rs, float& wx, float (&vs)[D],
                                            float& vp) {
  constexpr int NW = 1 + D;
  using Probe = ServeProbe<NW>;
  BatchView kb;  // (the probe reads the keys alone)
  kb.keys = keys;
  Probe pr;
  for (int j0 = 0; j0 < rs.len; j0 += Probe::N) {
    pr.load(t, kb, rs, j0);
#pragma unroll 1
    for (int q = 0; q < Probe::N; ++q) {
      if (j0 + q >= rs.len) break;
      float w[NW];
      pr.weights(q, t.L, o, w);
      wx = __fadd_rn(wx, w[0]);
#pragma unroll
      for (int k = 0; k < D; ++k) {
        vs[k] = __fadd_rn(vs[k], w[1 + k]);
        vp = __fadd_rn(vp, __fmul_rn(w[1 + k], w[1 + k]));
      }
    }
  }
}

// k_fm's finish over the full-row sums, in either math
template <int D>
__device__ __forceinline__ float rank_fm_finish(int fm_math, float wx, const float (&vs)[D],
                                                float vp) {
  if (fm_math == kFmStandard) {
    float sq = 0.0f;
#pragma unroll
    for (int k = 0; k < D; ++k) sq = __fadd_rn(sq, __fmul_rn(vs[k], vs[k]));
    return __fadd_rn(wx, __fmul_rn(0.5f, __fsub_rn(sq, vp)));
  }
  float vsum = 0.0f;
#pragma unroll
  for (int k = 0; k < D; ++k) vsum = __fadd_rn(vsum, vs[k]);
  return __fadd_rn(wx, __fsub_rn(__fmul_rn(vsum, vsum), vp));
}

}  // namespace hip
}  // namespace xflow
