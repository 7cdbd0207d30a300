// xflow-amd: candidate ranking from a frozen table (gfx950): one impression
// context scored against many candidate rows in one launch, LR (k_rank_lr) and
// FM (k_rank_fm).  docs/DESIGN.md §2.
//
// Both models decompose over the split of a row into context and candidate
// occurrences: LR's logit is ctx.wx + Σ_cand w, and FM's needs of the context
// only its 2 + D sums (wx, vs[0..D), vp), which the candidate's occurrences
// continue before the model's usual finish.  So the context is probed once
// per tile of candidates instead of once per candidate, and its occurrences
// are probed side by side across the wave instead of in dependent rounds on
// one lane.
//
// One wave per workgroup (kServeBlock); a workgroup owns 64 consecutive
// candidate rows.
//   requests    a binary search of req_ptr finds the request of the tile's
//               first row; the walk from there visits every request that has
//               rows in the tile (usually one).  No grid sync, one launch.
//   context     once per visited request: lane l takes the context's
//               occurrences l, l + 64, .. (a RowSpan of step 64 through the
//               serve kernels' chunked probe, so chains, probe_limit and
//               absent keys are theirs) and sums them in ascending order from
//               0.0f; an xor butterfly over the 64 lanes (strides 1, 2, .. 32,
//               each step an IEEE add of the two partners' values, which is
//               commutative, so both keep the same bits) leaves the request's
//               partial in every lane.  Its association depends on the
//               occurrence's index in the context alone: the partial is a
//               function of the context's keys, whatever tile computes it and
//               whatever else the call holds.
//   candidates  a lane whose row belongs to the request starts from that
//               partial, runs its row as k_serve_lr / k_serve_fm run theirs
//               and finishes over the full-row sums in either FM math.  With
//               an empty context the partial is +0.0f in every component and
//               the chain is the serve kernels' from 0.0f.
// Roundings: a sum of n context and m candidate terms passes at most
// ceil(n / 64) - 1 + 6 + m additions that round (an addition of the +0.0f of
// an empty lane or subtree is exact, so a context of n <= 64 occurrences
// costs at most ceil(log2 n)) -- never more than the n + m of a row summed in
// one chain.
// ctx_ptr values are clamped to [0, ctx_nnz] and request rows to the tile, so
// malformed pointers give wrong scores, never an access outside the arrays.
// No atomics, no scratch memory; the output is pctr[row] alone.
#include "serve_common.h"

namespace xflow {
namespace hip {

// the same bits in every lane: Σ over the wave in a fixed butterfly
__device__ __forceinline__ float rank_allsum(float v) {
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) v = __fadd_rn(v, __shfl_xor(v, o));
  return v;
}

// Calls f(cs, lo, hi) for every request with candidate rows [lo, hi) inside
// the tile [t0, t0 + kServeBlock): cs is this lane's share of the request's
// context, occurrences lane, lane + 64, .. of ctx_keys.  Wave-uniform but for
// cs; every lane of the wave takes part.
template <typename F>
__device__ __forceinline__ void rank_requests(const RankArgs& a, int64_t t0, F&& f) {
  const int64_t tend = t0 + kServeBlock < a.cands.rows ? t0 + kServeBlock : a.cands.rows;
  int64_t l0 = 0, l1 = a.R;  // first request that ends past the tile's first row
  while (l0 < l1) {
    const int64_t m = (l0 + l1) >> 1;
    if ((int64_t)a.req_ptr[m + 1] > t0) l1 = m;
    else l0 = m + 1;
  }
  const int64_t lane = threadIdx.x;
  for (int64_t q = l0; q < a.R; ++q) {
    int64_t lo = a.req_ptr[q], hi = a.req_ptr[q + 1];
    if (lo >= tend) break;
    lo = lo > t0 ? lo : t0;
    hi = hi < tend ? hi : tend;
    if (hi <= lo) continue;  // (no candidates: the context is never probed)
    int64_t c0 = a.ctx_ptr[q], c1 = a.ctx_ptr[q + 1];
    c0 = c0 < 0 ? 0 : (c0 > a.ctx_nnz ? a.ctx_nnz : c0);
    c1 = c1 < c0 ? c0 : (c1 > a.ctx_nnz ? a.ctx_nnz : c1);
    RowSpan cs;
    cs.base = c0 + lane;
    cs.step = kWave;
    cs.len = lane < c1 - c0 ? (int)((c1 - c0 - lane + kWave - 1) / kWave) : 0;
    f(cs, lo, hi);
  }
}

__global__ void __launch_bounds__(kServeBlock) k_rank_lr(RankArgs a) {
  const BatchView& b = a.cands;
  const TableView& t = a.table;
  const int64_t t0 = (int64_t)blockIdx.x * kServeBlock, r = t0 + threadIdx.x;
  float wx = 0.0f;
  rank_requests(a, t0, [&](const RowSpan& cs, int64_t lo, int64_t hi) {
    float cw = 0.0f;
    serve_lr_sum(t, a.ctx_keys, cs, cw);
    cw = rank_allsum(cw);
    if (r >= lo && r < hi) wx = cw;
  });
  if (r < b.rows) {
    serve_lr_sum(t, b.keys, row_span(b, r), wx);
    a.pctr[r] = sigmoid_ref(wx);
  }
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

template <int D>
__global__ void __launch_bounds__(kServeBlock) k_rank_fm(RankArgs a) {
  const BatchView& b = a.cands;
  const TableView& t = a.table;
  const int64_t t0 = (int64_t)blockIdx.x * kServeBlock, r = t0 + threadIdx.x;
  float vs[D];
#pragma unroll
  for (int k = 0; k < D; ++k) vs[k] = 0.0f;
  float wx = 0.0f, vp = 0.0f;
  rank_requests(a, t0, [&](const RowSpan& cs, int64_t lo, int64_t hi) {
    float cv[D];
#pragma unroll
    for (int k = 0; k < D; ++k) cv[k] = 0.0f;
    float cw = 0.0f, cp = 0.0f;
    rank_fm_sum<D>(t, a.opt, a.ctx_keys, cs, cw, cv, cp);
    cw = rank_allsum(cw);
    cp = rank_allsum(cp);
#pragma unroll
    for (int k = 0; k < D; ++k) cv[k] = rank_allsum(cv[k]);
    if (r >= lo && r < hi) {
      wx = cw;
      vp = cp;
#pragma unroll
      for (int k = 0; k < D; ++k) vs[k] = cv[k];
    }
  });
  if (r < b.rows) {
    rank_fm_sum<D>(t, a.opt, b.keys, row_span(b, r), wx, vs, vp);
    float y;  // (k_fm's finish over the full-row sums)
    if (a.model.fm_math == kFmStandard) {
      float sq = 0.0f;
#pragma unroll
      for (int k = 0; k < D; ++k) sq = __fadd_rn(sq, __fmul_rn(vs[k], vs[k]));
      y = __fadd_rn(wx, __fmul_rn(0.5f, __fsub_rn(sq, vp)));
    } else {
      float vsum = 0.0f;
#pragma unroll
      for (int k = 0; k < D; ++k) vsum = __fadd_rn(vsum, vs[k]);
      y = __fadd_rn(wx, __fsub_rn(__fmul_rn(vsum, vsum), vp));
    }
    a.pctr[r] = sigmoid_ref(y);
  }
}

void launch_rank(const RankArgs& a, hipStream_t st) {
  const TableLayout& L = a.table.L;
  const ModelSpec& m = a.model;
  const BatchView& b = a.cands;
  if (m.kind != kLR && m.kind != kFM) throw std::runtime_error("rank: LR or FM");
  if (L.opt != kFrozen || L.has_flag || L.sp != 1 || L.P != m.P() || L.p_w != m.p_w() ||
      L.stride != ((2 + L.P + 3) & ~3))
    throw std::runtime_error("rank: needs the model's frozen table (2 + P words per slot)");
  if (b.rows < 0 || b.rows > 0x7fffffffll || a.R < 0 || a.R > 0x7fffffffll || a.ctx_nnz < 0 ||
      a.ctx_nnz > 0x7fffffffll)
    throw std::runtime_error("rank: rows, requests and context keys are int32 offsets");
  if (b.rows == 0) return;
  if (!a.pctr || !a.req_ptr || !a.ctx_ptr || (a.ctx_nnz > 0 && !a.ctx_keys) ||
      (b.nnz > 0 && !b.keys) || (!b.row_ptr && b.nnz != b.rows * b.nnz_per_row))
    throw std::runtime_error("rank: null array or a fixed-width batch of another size");
  const dim3 g((unsigned)((b.rows + kServeBlock - 1) / kServeBlock)), blk(kServeBlock);
  if (m.kind == kLR) {
    hipLaunchKernelGGL(k_rank_lr, g, blk, 0, st, a);
  } else {
    switch (m.kernel_dim()) {
#define XF_RANK_CASE(DD) \
  case DD: hipLaunchKernelGGL(k_rank_fm<DD>, g, blk, 0, st, a); break;
      XF_RANK_CASE(1) XF_RANK_CASE(2) XF_RANK_CASE(4) XF_RANK_CASE(8) XF_RANK_CASE(10)
      XF_RANK_CASE(16) XF_RANK_CASE(32)
#undef XF_RANK_CASE
      default:
        throw std::runtime_error("rank: unsupported v_dim (1,2,4,8,10,16,32)");
    }
  }
  XF_HIP_CHECK(hipGetLastError());
}

}  // namespace hip
}  // namespace xflow
