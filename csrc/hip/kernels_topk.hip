// xflow-amd: segmented top-k of a score array (gfx950): the best k candidates
// of every ranking request, in order, without a host round trip (TopkArgs,
// backend.h; docs/DESIGN.md §2).
//
// The grid of k_topk_tile runs over tiles of 4096 consecutive rows, whatever
// requests they belong to; 256 threads hold 16 words each.
//   keys      a thread finds the request of its first row by an upper-bound
//             search of req_ptr and walks on from there (empty requests fall
//             out of the walk).  Row `row` of request q becomes
//               (4095 - (lo - t0)) << 44 | skey << 12 | (4095 - (row - t0))
//             with t0 the tile's first row, lo = max(req_ptr[q], t0) the start
//             of the request's rows inside the tile and skey the 32-bit sort
//             key of the score (eval_key_bits).  Descending order of the word
//             is request ascending, score descending, row ascending.  A short
//             last tile is padded with 4095 - position, below every real key.
//   sort      one bitonic network over the tile (topk_sort): word i sits in
//             v[i % 16] of thread i / 16, so the strides 1 .. 8 are compare-
//             exchanges between a thread's registers, 16 .. 512 are wave
//             shuffles, and only 1024 and 2048 (three steps of the 78) pass
//             through the 32 KB of LDS.  A short tile runs the network of the
//             next power of two.
//   results   after the sort the rows of a request sit in the positions of its
//             own rows, so position p has the request of row t0 + p (the same
//             walk again) and rank p - lo.  Ranks below k are written: to
//             idx / score when the whole request lies in the tile, else to
//             partial[t0 + p] as skey << 32 | ~index.
// k_topk_merge has one workgroup per tile boundary.  At most one request
// crosses a boundary, and the workgroup of the first boundary a request
// crosses owns it: it reads the request's sorted partial lists (min(k, rows in
// the tile) words from the start of the request's rows in each tile), S - 1 of
// them per round next to the best k so far, S = 4096 / k >= 4, sorts the round
// with the same network, and writes the final k.
// No atomics and no float arithmetic: scores are compared as integers and
// copied as bits.  Values of req_ptr are only ever compared against rows and
// positions that were bounded first, so a malformed req_ptr gives wrong
// entries, never an access outside the arrays.
#include "kernels.h"
#include "topk_common.h"

namespace xflow {
namespace hip {

namespace {

__global__ void __launch_bounds__(kBlock) k_topk_fill(int32_t* idx, float* score, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kBlock) {
    idx[i] = -1;
    score[i] = 0.0f;
  }
}

__global__ void __launch_bounds__(kBlock) k_topk_tile(TopkArgs a) {
  __shared__ u64 lds[kTopkT];
  const int64_t t0 = (int64_t)blockIdx.x * kTopkT;
  const int64_t tend = t0 + kTopkT < a.rows ? t0 + kTopkT : a.rows;
  const u32 rel0 = threadIdx.x * kTopkPer;
  const int64_t r0 = t0 + rel0;  // this thread's first row and, after the sort, position
  const int64_t q0 = topk_request(a.req_ptr, a.R, r0);
  u64 v[kTopkPer];
  int64_t q = q0;
#pragma unroll
  for (int e = 0; e < kTopkPer; ++e) {
    const int64_t row = r0 + e;
    u64 key = kTopkT - 1 - (rel0 + e);  // sorts behind every row of the tile
    if (row < tend) {
      while (q < a.R && (int64_t)a.req_ptr[q + 1] <= row) ++q;
      if (q < a.R) {
        int64_t lo = a.req_ptr[q];
        lo = lo > t0 ? lo : t0;
        lo = lo < row ? lo : row;
        key |= (u64)(kTopkT - 1 - (u32)(lo - t0)) << 44 | (u64)eval_key_bits(a.pctr[row]) << 12;
      }
    }
    v[e] = key;
  }
  topk_sort(v, topk_pow2(tend - t0), lds);
  q = q0;
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
    int64_t lo = qa > t0 ? qa : t0;
    lo = lo < pos ? lo : pos;
    const int64_t rank = pos - lo;
    const int64_t row = t0 + (kTopkT - 1 - (int64_t)(v[e] & (kTopkT - 1)));
    if (rank >= a.k || row >= tend) continue;
    const u32 ci = (u32)(row - qa);
    if (qa >= t0 && qb <= tend) {
      a.idx[q * a.k + rank] = (int32_t)ci;
      a.score[q * a.k + rank] = a.pctr[row];
    } else if (a.partial) {
      a.partial[pos] = (v[e] >> 12) << 32 | (u32)~ci;
    }
  }
}

__global__ void __launch_bounds__(kBlock) k_topk_merge(TopkArgs a) {
  __shared__ u64 lds[kTopkT];
  const u32 k = (u32)a.k, rel0 = threadIdx.x * kTopkPer;
  u64 v[kTopkPer];
  int64_t q, qa, qb;
  if (!topk_merge_edge(a.req_ptr, a.R, a.rows, k, a.partial, v, lds, q, qa, qb)) return;
#pragma unroll
  for (int e = 0; e < kTopkPer; ++e) {
    const u32 p = rel0 + e, ci = ~(u32)v[e];
    if (p < k && v[e] != 0 && qa + (int64_t)ci < qb) {
      a.idx[q * k + p] = (int32_t)ci;
      a.score[q * k + p] = a.pctr[qa + ci];
    }
  }
}

}  // namespace

void launch_topk_fill(int32_t* idx, float* score, int64_t n, hipStream_t st) {
  hipLaunchKernelGGL(k_topk_fill, dim3(grid_for(n)), dim3(kBlock), 0, st, idx, score, n);
}

void launch_topk(const TopkArgs& a, hipStream_t st) {
  if (!topk_check(a)) return;
  const int64_t tiles = (a.rows + kTopkT - 1) / kTopkT;
  if (tiles > 1 && !a.partial) throw std::runtime_error("topk: more than one tile needs the scratch");
  // (one launch pads both arrays; the sort kernels then write the entries that exist)
  launch_topk_fill(a.idx, a.score, a.R * a.k, st);
  if (tiles > 0) hipLaunchKernelGGL(k_topk_tile, dim3((unsigned)tiles), dim3(kBlock), 0, st, a);
  if (tiles > 1) hipLaunchKernelGGL(k_topk_merge, dim3((unsigned)(tiles - 1)), dim3(kBlock), 0, st, a);
  XF_HIP_CHECK(hipGetLastError());
}

}  // namespace hip
}  // namespace xflow
