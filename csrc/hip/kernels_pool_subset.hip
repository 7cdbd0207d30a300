// xflow-amd: pool subsets (gfx950): every request scored against its own list
// of candidates of a resident pool.  docs/DESIGN.md §2.
//
//   k_pool_subset<KP, STAGE>   pctr[e] = sigmoid_ref(y(ctx q(e), pool index[e]))
//     The flat list index[0..M) holds all requests' lists one after another;
//     request q owns [req_ptr[q], req_ptr[q + 1]).  y is k_pool_score's chain,
//     acc = fma(A[k], B[k], acc) over k = 0 .. Dk + 1 from 0.0f with A = {g *
//     u_q, c_q, 1} and B = {u_i, 1, c_i} (pool_operand): an element depends on
//     its own two vectors alone, never on M, R, N, its place in the list or
//     what else the call holds.
//
//     VALU, not the matrix cores: the entries of a wave belong to arbitrary
//     (request, candidate) pairs -- usually one request and 64 unrelated
//     candidates -- so a 32 x 32 MFMA would compute 1024 products to keep 32.
//     The kernel is bound by the gather of the pool rows, Dk + 2 fmas per W
//     floats read, and is built around that gather.
//
//     A workgroup of 256 threads takes 256 consecutive entries, a wave 64 of
//     them, a lane one.  A wave finds the request of its first entry by binary
//     search over req_ptr and walks on from there (rank_request_walk's shape;
//     empty requests fall through): each lane keeps the request whose range
//     holds its entry.  No value of req_ptr or index is ever used as an
//     address unchecked: q comes from the walk's own counter, and an index
//     outside [0, N) -- or an entry no request owns -- reads nothing and
//     stores +0.0f (topk's last tie class).
//
//     W = 4 (LR, reference FM, FM-1/2): a row is one float4 the lane loads.
//     W >= 8 and STAGE: the wave gathers its 64 rows together.  float4 number
//     t = lane + 64 j of the wave's 64 * W / 4 belongs to row t / Q, part t % Q
//     (Q = W / 4): consecutive lanes read consecutive 16 bytes of one pool row,
//     so a load instruction covers 64 / Q whole rows instead of 64 different
//     lines.  The float4 goes to the wave's own LDS region, rows dense (stride
//     W), and after the barrier lane l reads row l back.  Q is odd for every
//     width but 8, so lanes l and l + 1 of the read are Q float4 banks apart
//     and 16 consecutive lanes cover all 16; at W = 8 part p of row r is kept
//     at p ^ (r / 8 & 1) for the same effect.  The write side is consecutive
//     float4s either way (DESIGN.md has the arithmetic).  The one barrier is
//     reached by every thread of the workgroup: lanes past M take part in the
//     gather with no row and only skip the store.
//     !STAGE: the lane loads its own Q float4s, the A/B of the staging; the
//     arithmetic is the same code on the same values, so the bits are too.
//     Staging measured behind at W = 8, even at 12 and ahead from 20 on, so the
//     engine stages from kPoolSubsetStageMin unless told otherwise.
//     The context vector is read from ctx + q * W by the lane itself: lanes of
//     one request share the address and the read is a broadcast.
// No atomics, no scratch memory; the pctr store is coalesced.
#include "pool_common.h"

namespace xflow {
namespace hip {

template <int KP, bool STAGE>
__global__ void __launch_bounds__(kBlock) k_pool_subset(PoolSubsetArgs a, int dk, float g) {
  constexpr int W = pool_subset_width(KP), Q = W / 4;
  constexpr bool kStaged = STAGE && Q > 1;
  static_assert(Q == 1 || Q % 2 == 1 || Q == 2, "the swizzle covers Q = 2 only");
  const int Dk = KP == 4 ? dk : KP - 2;  // (KP = 4: reference FM and FM-1 have 1, FM-2 has 2)
  const int lane = threadIdx.x % kWave;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int64_t w0 = (int64_t)blockIdx.x * kBlock + (int64_t)wave * kWave;  // the wave's first entry
  const int64_t e = w0 + lane;
  const int64_t wend = w0 + kWave < a.M ? w0 + kWave : a.M;

  // the request of this lane's entry (wave-uniform walk)
  int64_t q = -1;
  if (w0 < a.M) {
    int64_t l0 = 0, l1 = a.R;  // first request that ends past the wave's first entry
    while (l0 < l1) {
      const int64_t m = (l0 + l1) >> 1;
      if ((int64_t)a.req_ptr[m + 1] > w0) l1 = m;
      else l0 = m + 1;
    }
    for (int64_t r = l0; r < a.R; ++r) {
      const int64_t lo = a.req_ptr[r], hi = a.req_ptr[r + 1];
      if (lo >= wend) break;
      if (e >= lo && e < hi) q = r;
    }
  }
  int i = e < a.M ? a.index[e] : -1;  // -1: no row to read
  if (i < 0 || i >= a.N || q < 0) i = -1;

  const float4* pool4 = reinterpret_cast<const float4*>(a.pool);
  float bv[W];
  if constexpr (kStaged) {
    __shared__ float4 s_rows[kBlock * Q];
    pool_subset_gather<Q, true>(pool4, i, lane, s_rows + wave * (kWave * Q), bv);
  } else {
    pool_subset_gather<Q, false>(pool4, i, lane, nullptr, bv);
  }
  if (e >= a.M) return;
  float out = 0.0f;
  if (i >= 0)
    out = pool_subset_score<KP>(reinterpret_cast<const float4*>(a.ctx) + q * Q, bv, Dk, g);
  a.pctr[e] = out;
}

void launch_pool_subset(const PoolSubsetArgs& a, hipStream_t st) {
  if (!pool_check(a)) return;
  if (a.spec.n != 0) return launch_pool_subset_cross(a, st);  // kernels_pool_cross.hip
  const int Dk = pool_dk(a.model);
  const float g = pool_gain(a.model);
  const int KPr = (Dk + 2 + 1) & ~1;
  if (pool_subset_width(KPr) != pool_width(a.model))
    throw std::runtime_error("pool_subset: unsupported v_dim (1,2,4,8,10,16,32)");
  const dim3 grid((unsigned)((a.M + kBlock - 1) / kBlock)), blk(kBlock);
  switch (KPr) {
#define XF_POOL_CASE(KP)                                                                      \
  case KP:                                                                                    \
    if (a.stage) hipLaunchKernelGGL((k_pool_subset<KP, true>), grid, blk, 0, st, a, Dk, g);   \
    else hipLaunchKernelGGL((k_pool_subset<KP, false>), grid, blk, 0, st, a, Dk, g);          \
    break;
    XF_POOL_CASE(2) XF_POOL_CASE(4) XF_POOL_CASE(6) XF_POOL_CASE(10) XF_POOL_CASE(12)
    XF_POOL_CASE(18) XF_POOL_CASE(34)
#undef XF_POOL_CASE
    default:
      throw std::runtime_error("pool_subset: unsupported v_dim (1,2,4,8,10,16,32)");
  }
  XF_HIP_CHECK(hipGetLastError());
}

}  // namespace hip
}  // namespace xflow
