// xflow-amd: the 4096-word bitonic network shared by the top-k kernels
// (kernels_topk.hip: segmented top-k of a score array; kernels_pool_topk.hip:
// the merge of a pool's strip lists; kernels_pool_subset_topk.hip: a tile's
// scores computed into the network's registers), and the walk and the merge
// rounds of the two kernels that tile a flat list.  Included by .hip files only.
#pragma once
#include "hip_util.h"

namespace xflow {
namespace hip {

constexpr int kTopkT = (int)kTopkTile;
constexpr int kTopkPer = kTopkT / kBlock;  // words per thread
static_assert(kTopkPer == 16 && kTopkT == 4096, "the key packing and the network assume 256 x 16");

// a at the lower index: descending leaves the larger word there
__device__ __forceinline__ void topk_cx(u64& a, u64& b, bool desc) {
  const bool gt = a > b;
  const u64 hi = gt ? a : b, lo = gt ? b : a;
  a = desc ? hi : lo;
  b = desc ? lo : hi;
}

// the strides 8 .. 1 of one merge step, inside the thread
__device__ __forceinline__ void topk_local(u64 (&v)[kTopkPer], bool desc) {
#pragma unroll
  for (int j = kTopkPer / 2; j > 0; j >>= 1) {
#pragma unroll
    for (int r = 0; r < kTopkPer; ++r)
      if ((r & j) == 0) topk_cx(v[r], v[r | j], desc);
  }
}

// Sorts words 0 .. n - 1 of the workgroup's 4096 descending (n a power of two,
// 16 <= n <= 4096, the same in every thread; the other words stay among
// themselves).  Every thread of the workgroup calls it.
__device__ __forceinline__ void topk_sort(u64 (&v)[kTopkPer], u32 n, u64* lds) {
  const u32 tid = threadIdx.x, base = tid * kTopkPer;
  // sequences of 2, 4, 8: the direction alternates inside the thread
#pragma unroll
  for (int k = 2; k < kTopkPer; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
      for (int r = 0; r < kTopkPer; ++r)
        if ((r & j) == 0) topk_cx(v[r], v[r | j], (r & k) == 0);
    }
  }
  topk_local(v, (base & kTopkPer) == 0);
  for (u32 k = 2 * kTopkPer; k <= n; k <<= 1) {
    const bool desc = (base & k) == 0;
    for (u32 j = k >> 1; j >= (u32)kTopkPer; j >>= 1) {
      const bool keep_max = ((base & j) == 0) == desc;
      if (j >= (u32)(kTopkPer * kWave)) {  // the partner thread is in another wave
#pragma unroll
        for (int r = 0; r < kTopkPer; ++r) lds[r * kBlock + tid] = v[r];
        __syncthreads();
        const u32 pt = tid ^ (j / kTopkPer);
#pragma unroll
        for (int r = 0; r < kTopkPer; ++r) {
          const u64 o = lds[r * kBlock + pt];
          v[r] = (o > v[r]) == keep_max ? o : v[r];
        }
        __syncthreads();
      } else {
        const int m = (int)(j / kTopkPer);
#pragma unroll
        for (int r = 0; r < kTopkPer; ++r) {
          const u64 o = __shfl_xor(v[r], m);
          v[r] = (o > v[r]) == keep_max ? o : v[r];
        }
      }
    }
    topk_local(v, desc);
  }
}

__device__ __forceinline__ u32 topk_pow2(int64_t x) {
  u32 n = kTopkPer;
  while ((int64_t)n < x) n <<= 1;
  return n;
}

// first request that ends past `row` (R: none)
__device__ __forceinline__ int64_t topk_request(const int32_t* req_ptr, int64_t R, int64_t row) {
  int64_t l0 = 0, l1 = R;
  while (l0 < l1) {
    const int64_t m = (l0 + l1) >> 1;
    if ((int64_t)req_ptr[m + 1] > row) l1 = m;
    else l0 = m + 1;
  }
  return l0;
}

// The merge of one tile edge (k_topk_merge, k_pool_subset_topk_merge; one
// workgroup per edge, blockIdx.x + 1 the tile behind it).  At most one request
// crosses an edge, and the workgroup of the first edge a request crosses owns
// it.  false: nothing owned here (the same in every thread).  true: q, qa, qb
// are the request and its rows, and words [0, k) of the workgroup's 4096 (word
// i in v[i % 16] of thread i / 16) are its best partial words in order, 0 where
// it has fewer: the request's sorted partial lists (min(k, rows in the tile)
// words from the start of its rows in each tile) pass S - 1 per round next to
// the best k so far, S = 4096 / k >= 4, through topk_sort.
__device__ __forceinline__ bool topk_merge_edge(const int32_t* req_ptr, int64_t R, int64_t rows,
                                                u32 k, const u64* partial, u64 (&v)[kTopkPer],
                                                u64* lds, int64_t& q, int64_t& qa, int64_t& qb) {
  const int64_t edge = ((int64_t)blockIdx.x + 1) * kTopkT;  // (< rows)
  q = topk_request(req_ptr, R, edge);  // holds row `edge`
  if (q >= R) return false;
  qa = req_ptr[q];
  qb = (int64_t)req_ptr[q + 1] < rows ? (int64_t)req_ptr[q + 1] : rows;
  // owned here: starts inside the tile before this edge
  if (qa < edge - kTopkT || qa >= edge || qb <= edge) return false;
  const u32 S = (u32)kTopkT / k;
  const int64_t tlast = (qb - 1) / kTopkT;
  const u32 rel0 = threadIdx.x * kTopkPer;
#pragma unroll
  for (int e = 0; e < kTopkPer; ++e) v[e] = 0;  // (below every partial: an index is < 2^31)
  // words [0, k): the best so far; [s k, (s + 1) k), s >= 1: the list of tile tb + s - 1
  for (int64_t tb = blockIdx.x; tb <= tlast; tb += S - 1) {
    const int64_t lists = tlast - tb + 1 < (int64_t)(S - 1) ? tlast - tb + 1 : (int64_t)(S - 1);
#pragma unroll
    for (int e = 0; e < kTopkPer; ++e) {
      const u32 p = rel0 + e, s = p / k, off = p - s * k;
      if (s == 0) continue;
      u64 x = 0;
      if ((int64_t)s <= lists) {
        const int64_t t = tb + s - 1;
        const int64_t lo = qa > t * kTopkT ? qa : t * kTopkT;
        const int64_t hi = qb < (t + 1) * kTopkT ? qb : (t + 1) * kTopkT;
        if ((int64_t)off < hi - lo) x = partial[lo + off];
      }
      v[e] = x;
    }
    topk_sort(v, topk_pow2((lists + 1) * (int64_t)k), lds);
  }
  return true;
}

}  // namespace hip
}  // namespace xflow
