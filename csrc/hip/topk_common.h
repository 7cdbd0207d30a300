// xflow-amd: the 4096-word bitonic network shared by the top-k kernels
// (kernels_topk.hip: segmented top-k of a score array; kernels_pool_topk.hip:
// the merge of a pool's strip lists).  Included by .hip files only.
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

}  // namespace hip
}  // namespace xflow
