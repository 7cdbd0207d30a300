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
#include "rank_common.h"

namespace xflow {
namespace hip {

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
    const float y = rank_fm_finish<D>(a.model.fm_math, wx, vs, vp);
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
  if (a.spec.n != 0) return launch_rank_cross(a, st);  // (kernels_rank_cross.hip)
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
