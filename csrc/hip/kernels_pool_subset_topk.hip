// xflow-amd: pool subsets, top-k (gfx950): every request's best k entries of its
// own list of pool candidates, scored and selected in one kernel -- the M
// scores are never stored (PoolSubsetTopkArgs, backend.h; docs/DESIGN.md §2).
//
//   k_pool_subset_topk<KP, STAGE>   one workgroup of 256 threads per tile of
//     4096 consecutive entries of the flat list index[0..M), whatever requests
//     the tile holds: k_topk_tile's tiling, with k_pool_subset's scores computed
//     straight into the words the network sorts.
//     score   16 rounds of 256 entries; in round j thread t takes entry t0 +
//             256 j + t, so the index loads and the walk of req_ptr are
//             coalesced.  A thread's 16 index loads are issued together before
//             the first round and wait in the slots of their words, so a round
//             has one memory latency, the gather's, not two.  A wave finds the request of its first entry by binary
//             search once and walks on from there through its rounds
//             (k_pool_subset's walk); a lane keeps the request whose range holds
//             its entry.  No value of req_ptr or index is used as an address
//             unchecked: q is the walk's own counter, and an index outside [0,
//             N) reads nothing and scores +0.0f.  The pool row arrives as in
//             k_pool_subset (pool_subset_gather: one float4 at W = 4; the
//             wave's 64 rows through its LDS region with STAGE; else the
//             lane's own Q loads) and the score is pool_subset_score, the same
//             device function on the same values: every score has the bits
//             k_pool_subset would have stored.  Rounds past the end of a short
//             last tile are skipped by the whole workgroup.
//     words   entry `rel` of the tile becomes k_topk_tile's word
//               (4095 - (lo - t0)) << 44 | eval_key_bits(score) << 12 | (4095 - rel)
//             (lo: the start of its request's entries inside the tile; an entry
//             past M or one no request owns is padding, 4095 - rel) and is
//             written to lds[rel], the 32 KB buffer topk_sort needs anyway.
//             After one barrier thread t reads words 16 t .. 16 t + 15 into
//             v[16], topk_sort's layout; a second barrier separates those reads
//             from the network's own use of the buffer.
//     sort    topk_sort over the next power of two of the tile's entries.
//     results k_topk_tile's: position p has the request of entry t0 + p and
//             rank p - lo; ranks below k are written.  A request wholly inside
//             the tile gets idx[q][rank] = index[row] -- the pool index, not
//             the position -- and score[q][rank] = the float whose bits are the
//             word's key: eval_key_bits is the identity on a positive float, so
//             the word holds the score itself, and a key of 0 (NaN, zero or
//             negative: the last tie class) comes back as +0.0f.  A request
//             that crosses a tile edge writes partial[pos] = key << 32 | ~ci.
//   k_pool_subset_topk_merge   one workgroup per tile edge: k_topk_merge's
//     ownership rule and rounds (topk_merge_edge, topk_common.h); the score is
//     the word's high half and idx is index[qa + ci].
//   k_pool_subset_map   the composed path's last step (Backend::pool_subset_map).
// Padding (-1 / +0.0f) is k_topk_fill's, launched first.  No atomics, no
// scratch besides partial ([M] words, only when M > 4096).
//
// LDS: the 32 KB of words and, staged, 64 * W * 4 bytes per wave of rows, kept
// apart (a word is written in the round that scores it, while the region is in
// use): 32 KB up to W = 4 and for every direct instance, 40 / 44 / 52 / 68 KB
// staged at W = 8 / 12 / 20 / 36.  Of a CU's 160 KB that is 5 workgroups (20
// waves) direct and 4 / 3 / 3 / 2 staged; the engine stages from 20 floats on,
// so 3 workgroups at FM-16 and 2 at FM-32 -- 8 waves, each with up to 9
// independent 1 KB loads in flight per round.
// Widest instance (KP = 34, staged), from the compiler's resource usage:
// 130 VGPRs, 0 AGPRs, 69632 bytes of LDS, no scratch, no spills (direct: 100
// VGPRs, 32768 bytes, none; the merge: 188 VGPRs, 32768 bytes, none).
#include "kernels.h"
#include "pool_common.h"
#include "topk_common.h"

namespace xflow {
namespace hip {

namespace {

template <int KP, bool STAGE>
__global__ void __launch_bounds__(kBlock) k_pool_subset_topk(PoolSubsetTopkArgs a, int dk, float g) {
  constexpr int W = pool_subset_width(KP), Q = W / 4;
  constexpr bool kStaged = STAGE && Q > 1;
  static_assert(Q == 1 || Q % 2 == 1 || Q == 2, "the swizzle covers Q = 2 only");
  __shared__ u64 lds[kTopkT];
  __shared__ float4 s_rows[kStaged ? kBlock * Q : 1];
  const int Dk = KP == 4 ? dk : KP - 2;  // (KP = 4: reference FM and FM-1 have 1, FM-2 has 2)
  const int tid = threadIdx.x, lane = tid % kWave;
  const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int64_t t0 = (int64_t)blockIdx.x * kTopkT;
  const int64_t tend = t0 + kTopkT < a.M ? t0 + kTopkT : a.M;
  const float4* pool4 = reinterpret_cast<const float4*>(a.pool);
  const float4* ctx4 = reinterpret_cast<const float4*>(a.ctx);
  float4* mine = s_rows + (kStaged ? wave * (kWave * Q) : 0);

  // the thread's 16 indices, all loads in flight at once; each waits in the
  // slot of its word, which no other thread touches before the barrier
  {
    int ii[kTopkPer];
#pragma unroll
    for (int j = 0; j < kTopkPer; ++j) {
      const int64_t e = t0 + j * kBlock + tid;
      ii[j] = e < tend ? a.index[e] : -1;  // -1: no row to read
    }
#pragma unroll
    for (int j = 0; j < kTopkPer; ++j) lds[j * kBlock + tid] = (u32)ii[j];
  }
  // first request that ends past the wave's first entry; the rounds walk on
  int64_t qc = topk_request(a.req_ptr, a.R, t0 + (int64_t)wave * kWave);
#pragma unroll 1
  for (int j = 0; j < kTopkPer; ++j) {
    const u32 rel = (u32)(j * kBlock + tid);
    const u64 pad = (u64)(kTopkT - 1) - rel;  // sorts behind every entry of the tile
    if (t0 + (int64_t)j * kBlock >= tend) {   // (the whole workgroup)
      lds[rel] = pad;
      continue;
    }
    const int64_t w0 = t0 + (int64_t)j * kBlock + (int64_t)wave * kWave;  // the wave's first entry
    const int64_t e = w0 + lane;
    const int64_t wend = w0 + kWave < tend ? w0 + kWave : tend;
    int64_t q = -1, qlo = 0;
    if (w0 < tend) {
      while (qc < a.R && (int64_t)a.req_ptr[qc + 1] <= w0) ++qc;
      for (int64_t r = qc; r < a.R; ++r) {
        const int64_t lo = a.req_ptr[r], hi = a.req_ptr[r + 1];
        if (lo >= wend) break;
        if (e >= lo && e < hi) q = r, qlo = lo;
      }
    }
    if (e >= tend) q = -1;
    int i = (int)(u32)lds[rel];
    if (i < 0 || i >= a.N || q < 0) i = -1;
    float bv[W];
    pool_subset_gather<Q, kStaged>(pool4, i, lane, mine, bv);
    const float p = i >= 0 ? pool_subset_score<KP>(ctx4 + q * Q, bv, Dk, g) : 0.0f;
    u64 word = pad;
    if (q >= 0) {
      const int64_t lo = qlo > t0 ? qlo : t0;  // (<= e)
      word |= (u64)(kTopkT - 1 - (u32)(lo - t0)) << 44 | (u64)eval_key_bits(p) << 12;
    }
    lds[rel] = word;
    if constexpr (kStaged) __syncthreads();  // the region is read before the next round fills it
  }
  __syncthreads();
  const u32 rel0 = (u32)tid * kTopkPer;
  u64 v[kTopkPer];
#pragma unroll
  for (int e = 0; e < kTopkPer; ++e) v[e] = lds[rel0 + e];
  __syncthreads();  // (the network writes the buffer)
  topk_sort(v, topk_pow2(tend - t0), lds);

  const int64_t r0 = t0 + rel0;  // this thread's first position
  int64_t q = topk_request(a.req_ptr, a.R, r0);
  bool live = true;
#pragma unroll
  for (int e = 0; e < kTopkPer; ++e) {
    const int64_t pos = r0 + e;
    live = live && pos < tend;
    if (live) {
      while (q < a.R && (int64_t)a.req_ptr[q + 1] <= pos) ++q;
      live = q < a.R;
    }
    if (!live) continue;
    const int64_t qa = a.req_ptr[q], qb = a.req_ptr[q + 1];
    if (pos < qa) continue;  // (no request owns it: padding sits here)
    const int64_t lo = qa > t0 ? qa : t0;
    const int64_t rank = pos - lo;
    const int64_t row = t0 + (kTopkT - 1 - (int64_t)(v[e] & (kTopkT - 1)));
    if (rank >= a.k || row >= tend || row < qa) continue;
    const u32 key = (u32)(v[e] >> 12);
    if (qa >= t0 && qb <= tend) {
      a.idx[q * a.k + rank] = a.index[row];
      a.score[q * a.k + rank] = __uint_as_float(key);
    } else if (a.partial) {
      a.partial[pos] = (u64)key << 32 | (u32)~(u32)(row - qa);
    }
  }
}

__global__ void __launch_bounds__(kBlock) k_pool_subset_topk_merge(PoolSubsetTopkArgs a) {
  __shared__ u64 lds[kTopkT];
  const u32 k = (u32)a.k, rel0 = threadIdx.x * kTopkPer;
  u64 v[kTopkPer];
  int64_t q, qa, qb;
  if (!topk_merge_edge(a.req_ptr, a.R, a.M, k, a.partial, v, lds, q, qa, qb)) return;
#pragma unroll
  for (int e = 0; e < kTopkPer; ++e) {
    const u32 p = rel0 + e, ci = ~(u32)v[e];
    if (p < k && v[e] != 0 && qa + (int64_t)ci < qb) {
      a.idx[q * k + p] = a.index[qa + ci];
      a.score[q * k + p] = __uint_as_float((u32)(v[e] >> 32));
    }
  }
}

__global__ void __launch_bounds__(kBlock)
k_pool_subset_map(int32_t* idx, const int32_t* req_ptr, const int32_t* index, int64_t R, int k,
                  int64_t M) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < R * k;
       i += (int64_t)gridDim.x * kBlock) {
    const int32_t x = idx[i];
    if (x < 0) continue;
    const int64_t q = i / k;
    int64_t lo = req_ptr[q], hi = req_ptr[q + 1];
    lo = lo < 0 ? 0 : (lo > M ? M : lo);
    hi = hi > M ? M : hi;
    idx[i] = lo + x < hi ? index[lo + x] : -1;
  }
}

}  // namespace

void launch_pool_subset_topk(const PoolSubsetTopkArgs& a, hipStream_t st) {
  if (!pool_check(a)) return;
  const int Dk = pool_dk(a.model);
  const float g = pool_gain(a.model);
  const int KPr = (Dk + 2 + 1) & ~1;
  if (pool_subset_width(KPr) != pool_width(a.model))
    throw std::runtime_error("pool_subset_topk: unsupported v_dim (1,2,4,8,10,16,32)");
  const int64_t tiles = (a.M + kTopkT - 1) / kTopkT;
  if (tiles > 1 && !a.partial)
    throw std::runtime_error("pool_subset_topk: more than one tile needs the scratch");
  // (one launch pads both arrays; the tiles then write the entries that exist)
  launch_topk_fill(a.idx, a.score, a.R * a.k, st);
  const dim3 grid((unsigned)tiles), blk(kBlock);
  if (tiles > 0) switch (KPr) {
#define XF_POOL_CASE(KP)                                                                        \
  case KP:                                                                                      \
    if (a.stage) hipLaunchKernelGGL((k_pool_subset_topk<KP, true>), grid, blk, 0, st, a, Dk, g); \
    else hipLaunchKernelGGL((k_pool_subset_topk<KP, false>), grid, blk, 0, st, a, Dk, g);        \
    break;
      XF_POOL_CASE(2) XF_POOL_CASE(4) XF_POOL_CASE(6) XF_POOL_CASE(10) XF_POOL_CASE(12)
      XF_POOL_CASE(18) XF_POOL_CASE(34)
#undef XF_POOL_CASE
      default:
        throw std::runtime_error("pool_subset_topk: unsupported v_dim (1,2,4,8,10,16,32)");
    }
  if (tiles > 1)
    hipLaunchKernelGGL(k_pool_subset_topk_merge, dim3((unsigned)(tiles - 1)), blk, 0, st, a);
  XF_HIP_CHECK(hipGetLastError());
}

void launch_pool_subset_map(int32_t* idx, const int32_t* req_ptr, const int32_t* index, int64_t R,
                            int k, int64_t M, hipStream_t st) {
  if (R <= 0 || k <= 0 || M <= 0) return;
  hipLaunchKernelGGL(k_pool_subset_map, dim3(grid_for(R * k)), dim3(kBlock), 0, st, idx, req_ptr,
                     index, R, k, M);
  XF_HIP_CHECK(hipGetLastError());
}

}  // namespace hip
}  // namespace xflow
