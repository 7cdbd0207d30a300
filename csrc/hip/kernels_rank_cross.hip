// xflow-amd: candidate ranking of models with feature crosses (gfx950):
// k_rank_lr_x and k_rank_fm_x<D>, kernels_rank.hip's kernels for RankArgs with
// spec.n > 0.  docs/DESIGN.md §2.
//
// A candidate's row is the context's entries, the candidate's, and the C cross
// keys of that concatenated row (backend.h: operand = the raw key of the
// field's first occurrence, the context's before the candidate's, ~0 when
// neither has the field).  The split of kernels_rank.hip survives: a cross
// whose fields all occur in the context is a function of the context alone
// and joins the context's partial, probed once per tile; any other cross
// costs a candidate a few operand reads from LDS, one hash and one probe.  No
// expanded batch, no crossed copy: the output is pctr[row] alone, without
// atomics or scratch memory.
//
// One wave per workgroup, 64 consecutive candidate rows per tile, the request
// walk of kernels_rank.hip (rank_common.h).  An operand slot is 4 c + k
// (cross c, operand k): at most 64, one per lane.  The host passes by value
// the spec's distinct operand fields (nu <= 64) and the slot -> distinct field
// map (RankCrossMap).
//   candidate operands   once per tile: a lane walks its row once, eight
//               entries in flight, and keeps the raw key of the first
//               occurrence of every distinct operand field in LDS, cand[u][lane]
//               (lane-consecutive 8-byte words: no bank conflict); bit u of
//               its `seen` register says the row has the field at all, so a
//               first occurrence whose key is ~0 stays the operand.
//   context operands     once per visited request: the context is staged in
//               chunks of 64 entries (lane l loads entry j0 + l, key and field
//               id, coalesced); lane s scans the chunk with broadcast reads
//               for its slot's field and keeps the first match; the scan ends
//               when a ballot shows every live slot found, or with the
//               context.  The ballot is wave-uniform: cross c is complete iff
//               all of its slots are set.
//   context partial      a lane's occurrences l, l + 64, .. as in k_rank_*;
//               then lane j, j below the number of complete crosses, hashes
//               the j-th complete cross from the slots' operands and adds its
//               probe; then the fixed butterfly.  The partial is a function of
//               the context's keys, its field ids and the spec.
//   candidates  a lane of the request hashes its incomplete crosses in spec
//               order -- an operand from the context's slot if the context has
//               the field, else from its own cand column -- into its column of
//               xk[i][lane]; after the walk it continues the partial with its
//               own occurrences and then with that column, a RowSpan of step
//               64 through the same chunked probe.
// Roundings: a context of n entries and j complete crosses and a candidate of
// m entries and C - j incomplete ones pass at most ceil(n / 64) + 6 + m + C - j
// additions that round, never more than the n + m + C of the expanded row.
// LDS (dynamic): 512 B per distinct field + 512 B per cross + 1408 B.  The
// worst case, 16 crosses of arity 4 over 64 fields, is 32 KB + 8 KB + 1.4 KB =
// 42368 B: 3 one-wave workgroups per CU's 160 KB; 13 pair crosses over 26
// fields take 21 KB (7 per CU), one pair cross 2.9 KB.  A tile is bound by the
// latency of its probe rounds, as in kernels_rank.hip.
// Context indices are clamped as there: malformed pointers give wrong scores,
// never an access outside the arrays.
#include "rank_common.h"

namespace xflow {
namespace hip {

constexpr int kRankSlots = kCrossSlots;
static_assert(kRankSlots == kWave, "one operand slot per lane");

using RankCrossMap = CrossMap;  // backend.h: the spec's distinct operand fields

struct RankCrossLds {
  u64* cand;    // [nu][64] candidate operands
  u64* xk;      // [C][64] a lane's incomplete cross keys
  u64* ck;      // [64] the staged context chunk: keys
  u64* cop;     // [64] the context's operand of every slot
  u64* cxk;     // [16] the complete crosses' keys
  int32_t* cf;  // [64] the staged context chunk: field ids
};
inline size_t rank_cross_lds_bytes(int nu, int C) {
  return (size_t)((nu + C) * kWave + 2 * kWave + kMaxCrosses) * 8 + kWave * 4;
}
__device__ __forceinline__ RankCrossLds rank_cross_lds(int nu, int C) {
  extern __shared__ __align__(16) u64 rank_cross_mem[];
  RankCrossLds s;
  s.cand = rank_cross_mem;
  s.xk = s.cand + nu * kWave;
  s.ck = s.xk + C * kWave;
  s.cop = s.ck + kWave;
  s.cxk = s.cop + kWave;
  s.cf = reinterpret_cast<int32_t*>(s.cxk + kMaxCrosses);
  return s;
}

// a lane's state across the request walk
struct RankCross {
  RankCrossLds s;
  u64 seen = 0;     // bit u: this lane's candidate row has distinct field u
  u64 found = 0;    // (wave-uniform) bit slot: the request's context has the slot's field
  u32 complete = 0; // (wave-uniform) bit c: cross c is context-complete
  int32_t myf = -1; // the field of this lane's slot (-1: the slot is unused)
  int nx = 0;       // keys in this lane's xk column

  // the candidate operands of row r, once per tile
  __device__ __forceinline__ void init(const RankArgs& a, const RankCrossMap& m, int64_t r) {
    const int lane = threadIdx.x;
    const CrossSpec& x = a.spec;
    s = rank_cross_lds(m.nu, x.n);
    const int c = lane >> 2, k = lane & 3;
    if (c < x.n && k < x.arity[c]) myf = x.field[c][k];
    if (r >= a.cands.rows) return;
    const BatchView& b = a.cands;
    const RowSpan rs = row_span(b, r);
    for (int j0 = 0; j0 < rs.len; j0 += kServeItems) {
      u64 key[kServeItems];
      int32_t g[kServeItems];
#pragma unroll
      for (int q = 0; q < kServeItems; ++q) {
        const bool on = j0 + q < rs.len;
        key[q] = on ? b.keys[rs.at(j0 + q)] : 0ull;
        g[q] = on ? b.fgid[rs.at(j0 + q)] : -1;  // (operand fields are >= 0)
      }
      for (int u = 0; u < m.nu; ++u) {
        const int32_t f = m.ufield[u];
#pragma unroll
        for (int q = 0; q < kServeItems; ++q)
          if (g[q] == f && !((seen >> u) & 1ull)) {
            seen |= 1ull << u;
            s.cand[u * kWave + lane] = key[q];
          }
      }
    }
  }

  // The context [c0, c1) of a visited request: its operands, which crosses it
  // completes, and the span of this lane's complete-cross key in s.cxk (one
  // key in the lanes below the number of complete crosses).  Wave-uniform.
  __device__ __forceinline__ RowSpan context(const RankArgs& a, int64_t c0, int64_t c1) {
    const int lane = threadIdx.x;
    const CrossSpec& x = a.spec;
    const u64 live = __ballot(myf >= 0);
    bool have = false;
    u64 op = kNoGroup;
    found = 0;
    for (int64_t j0 = c0; j0 < c1 && found != live; j0 += kWave) {
      const int cn = c1 - j0 < kWave ? (int)(c1 - j0) : kWave;
      __syncthreads();  // (the chunk before this one has been scanned)
      if (lane < cn) {
        s.ck[lane] = a.ctx_keys[j0 + lane];
        s.cf[lane] = a.ctx_fgid[j0 + lane];
      }
      __syncthreads();
      for (int i = 0; i < cn; ++i) {
        const int32_t g = s.cf[i];
        const u64 key = s.ck[i];
        if (!have && myf >= 0 && g == myf) {
          have = true;
          op = key;
        }
      }
      found = __ballot(have);
    }
    __syncthreads();  // (the request before this one has read its operands)
    s.cop[lane] = op;
    complete = 0u;
    int ncomp = 0, myc = -1;
    for (int c = 0; c < x.n; ++c) {
      const u64 need = ((1ull << x.arity[c]) - 1ull) << (4 * c);
      if ((found & need) == need) {
        if (lane == ncomp) myc = c;
        complete |= 1u << c;
        ++ncomp;
      }
    }
    __syncthreads();
    RowSpan xs;
    xs.base = lane;
    xs.len = 0;
    if (myc >= 0) {  // (myc < 16: lanes 0 .. ncomp - 1)
      u64 ops[kMaxCrossArity];
      int32_t fs[kMaxCrossArity];
#pragma unroll
      for (int k = 0; k < kMaxCrossArity; ++k) {
        ops[k] = s.cop[4 * myc + k];
        fs[k] = x.field[myc][k];
      }
      s.cxk[lane] = cross_key(fs, ops, x.arity[myc]);
      xs.len = 1;
    }
    return xs;
  }

  // a lane of the request just visited: its incomplete crosses, in spec order
  __device__ __forceinline__ void candidate(const RankArgs& a, const RankCrossMap& m) {
    const int lane = threadIdx.x;
    const CrossSpec& x = a.spec;
    int i = 0;
    for (int c = 0; c < x.n; ++c) {
      if ((complete >> c) & 1u) continue;
      u64 ops[kMaxCrossArity];
#pragma unroll
      for (int k = 0; k < kMaxCrossArity; ++k) {
        const int sl = 4 * c + k;
        u64 v = kNoGroup;
        if (k < x.arity[c]) {
          const int u = m.slot_u[sl];
          if ((found >> sl) & 1ull) v = s.cop[sl];
          else if ((seen >> u) & 1ull) v = s.cand[u * kWave + lane];
        }
        ops[k] = v;
      }
      s.xk[i * kWave + lane] = cross_key(x.field[c], ops, x.arity[c]);
      ++i;
    }
    nx = i;
  }

  __device__ __forceinline__ RowSpan keys() const {
    RowSpan xs;
    xs.base = threadIdx.x;
    xs.step = kWave;
    xs.len = nx;
    return xs;
  }
};

__global__ void __launch_bounds__(kServeBlock) k_rank_lr_x(RankArgs a, RankCrossMap m) {
  const BatchView& b = a.cands;
  const TableView& t = a.table;
  const int64_t t0 = (int64_t)blockIdx.x * kServeBlock, r = t0 + threadIdx.x;
  RankCross x;
  x.init(a, m, r);
  float wx = 0.0f;
  rank_request_walk(a, t0, [&](int64_t c0, int64_t c1, int64_t lo, int64_t hi) {
    float cw = 0.0f;
    serve_lr_sum(t, a.ctx_keys, rank_ctx_span(c0, c1), cw);
    const RowSpan xs = x.context(a, c0, c1);
    serve_lr_sum(t, x.s.cxk, xs, cw);
    cw = rank_allsum(cw);
    if (r >= lo && r < hi) {
      wx = cw;
      x.candidate(a, m);
    }
  });
  if (r < b.rows) {
    serve_lr_sum(t, b.keys, row_span(b, r), wx);
    serve_lr_sum(t, x.s.xk, x.keys(), wx);
    a.pctr[r] = sigmoid_ref(wx);
  }
}

template <int D>
__global__ void __launch_bounds__(kServeBlock) k_rank_fm_x(RankArgs a, RankCrossMap m) {
  const BatchView& b = a.cands;
  const TableView& t = a.table;
  const int64_t t0 = (int64_t)blockIdx.x * kServeBlock, r = t0 + threadIdx.x;
  RankCross x;
  x.init(a, m, r);
  float vs[D];
#pragma unroll
  for (int k = 0; k < D; ++k) vs[k] = 0.0f;
  float wx = 0.0f, vp = 0.0f;
  rank_request_walk(a, t0, [&](int64_t c0, int64_t c1, int64_t lo, int64_t hi) {
    float cv[D];
#pragma unroll
    for (int k = 0; k < D; ++k) cv[k] = 0.0f;
    float cw = 0.0f, cp = 0.0f;
    rank_fm_sum<D>(t, a.opt, a.ctx_keys, rank_ctx_span(c0, c1), cw, cv, cp);
    const RowSpan xs = x.context(a, c0, c1);
    rank_fm_sum<D>(t, a.opt, x.s.cxk, xs, cw, cv, cp);
    cw = rank_allsum(cw);
    cp = rank_allsum(cp);
#pragma unroll
    for (int k = 0; k < D; ++k) cv[k] = rank_allsum(cv[k]);
    if (r >= lo && r < hi) {
      wx = cw;
      vp = cp;
#pragma unroll
      for (int k = 0; k < D; ++k) vs[k] = cv[k];
      x.candidate(a, m);
    }
  });
  if (r < b.rows) {
    rank_fm_sum<D>(t, a.opt, b.keys, row_span(b, r), wx, vs, vp);
    rank_fm_sum<D>(t, a.opt, x.s.xk, x.keys(), wx, vs, vp);
    a.pctr[r] = sigmoid_ref(rank_fm_finish<D>(a.model.fm_math, wx, vs, vp));
  }
}

// (launch_rank has checked the table, the sizes and the arrays)
void launch_rank_cross(const RankArgs& a, hipStream_t st) {
  const CrossSpec& x = a.spec;
  const BatchView& b = a.cands;
  check_cross_spec(x, "rank");
  if ((a.ctx_nnz > 0 && !a.ctx_fgid) || (b.nnz > 0 && !b.fgid))
    throw std::invalid_argument("rank: crosses need the field ids of the contexts and the candidates");
  const RankCrossMap m = cross_map(x);
  const size_t lds = rank_cross_lds_bytes(m.nu, x.n);
  const dim3 g((unsigned)((b.rows + kServeBlock - 1) / kServeBlock)), blk(kServeBlock);
  if (a.model.kind == kLR) {
    hipLaunchKernelGGL(k_rank_lr_x, g, blk, lds, st, a, m);
  } else {
    switch (a.model.kernel_dim()) {
#define XF_RANK_CASE(DD) \
  case DD: hipLaunchKernelGGL(k_rank_fm_x<DD>, g, blk, lds, st, a, m); break;
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
