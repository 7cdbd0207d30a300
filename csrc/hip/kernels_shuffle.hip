// xflow-amd: per-epoch row shuffling on the device (Backend::shuffle_rows).
//
// Destination row i receives source row pi(i) = shuffle_index(i, rows, seed)
// (common.h): a keyed bijection every lane evaluates for itself, so there is
// no permutation array, no sort and no host in the loop.  The gathers read
// whole rows -- a row of a row-major or CSR batch is one contiguous run (312 B
// at the Criteo width) -- and write coalesced.
//
//   fixed width  k_shuffle_tile: k_field_major's LDS tile pass (kernels_layout
//                .hip) with the tile's 64 source rows taken from pi -- the
//                shuffle costs the transpose the step pays anyway; labels ride
//                in the same launch.  Row-major output: the same kernel
//                without the tile.
//   CSR          k_shuffle_len (the rows' new lengths and labels), the
//                exclusive scan (launch_scan_u32: the new row_ptr), then
//                k_shuffle_gather: a workgroup owns 256 consecutive
//                destination rows = one contiguous range of entries, keeps
//                their offsets and source bases in LDS, and every lane finds
//                its entry's row by binary search there.
#include <stdexcept>

#include "kernels.h"
#include "hip_util.h"

namespace xflow {
namespace hip {

constexpr int kShufTileRows = 64;
constexpr int kShufMaxFields = 64;  // LDS: 64 x 65 x 8 B = 33 KB per workgroup
constexpr int kShufGatherRows = kBlock;  // destination rows per gather workgroup

// TO != T: zero-extending copy (compact u32 keys -> u64), as k_field_major
template <typename T, typename TO, bool FM>
__global__ void __launch_bounds__(kBlock)
    k_shuffle_tile(const T* __restrict__ src, TO* __restrict__ dst,
                   const float* __restrict__ lab_in, float* __restrict__ lab_out, int64_t rows,
                   int F, ShufflePerm pi) {
  __shared__ int64_t srow[kShufTileRows];  // first element of the tile's source rows
  const int64_t r0 = (int64_t)blockIdx.x * kShufTileRows;
  const int nr = (int)(rows - r0 < kShufTileRows ? rows - r0 : kShufTileRows);
  if ((int)threadIdx.x < nr) {
    const int64_t p = (int64_t)pi.at((u64)(r0 + threadIdx.x));
    XF_DASSERT(p >= 0 && p < rows);
    srow[threadIdx.x] = p * F;
    if (lab_out) lab_out[r0 + threadIdx.x] = lab_in[p];
  }
  __syncthreads();
  const int n = nr * F;
  if constexpr (FM) {
    // (+1 column of padding: consecutive rows of one field land in different banks)
    __shared__ T tile[kShufTileRows * (kShufMaxFields + 1)];
    for (int i = threadIdx.x; i < n; i += kBlock) {
      const int r = i / F, f = i - r * F;
      tile[r * (kShufMaxFields + 1) + f] = src[srow[r] + f];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < F * kShufTileRows; i += kBlock) {
      const int f = i / kShufTileRows, r = i - f * kShufTileRows;
      if (r < nr) dst[(int64_t)f * rows + r0 + r] = (TO)tile[r * (kShufMaxFields + 1) + f];
    }
  } else {
    TO* d = dst + r0 * F;  // the tile's destination rows are one contiguous run
    for (int i = threadIdx.x; i < n; i += kBlock) {
      const int r = i / F, f = i - r * F;
      d[i] = (TO)src[srow[r] + f];
    }
  }
}

template <typename T, typename TO>
static void launch_tile(const void* src, void* dst, const float* lab_in, float* lab_out,
                        int64_t rows, int F, bool fm, const ShufflePerm& pi, hipStream_t st) {
  const dim3 g((unsigned)((rows + kShufTileRows - 1) / kShufTileRows));
  if (fm)
    hipLaunchKernelGGL((k_shuffle_tile<T, TO, true>), g, dim3(kBlock), 0, st,
                       static_cast<const T*>(src), static_cast<TO*>(dst), lab_in, lab_out, rows, F,
                       pi);
  else
    hipLaunchKernelGGL((k_shuffle_tile<T, TO, false>), g, dim3(kBlock), 0, st,
                       static_cast<const T*>(src), static_cast<TO*>(dst), lab_in, lab_out, rows, F,
                       pi);
  XF_HIP_CHECK(hipGetLastError());
}

void launch_shuffle_fixed(const ShuffleArgs& a, hipStream_t st) {
  const BatchView& s = a.src;
  if (s.rows <= 0) return;
  const int F = s.nnz_per_row;
  if (F > kShufMaxFields) throw std::invalid_argument("shuffle_rows: at most 64 fields");
  const ShufflePerm pi = shuffle_perm((u64)s.rows, a.seed);
  if (a.key_bytes == 4)
    launch_tile<u32, unsigned long long>(s.keys, a.keys, s.labels, a.labels, s.rows, F,
                                         a.field_major_out, pi, st);
  else
    launch_tile<unsigned long long, unsigned long long>(s.keys, a.keys, s.labels, a.labels, s.rows,
                                                        F, a.field_major_out, pi, st);
  if (s.fgid)
    launch_tile<u32, u32>(s.fgid, a.fgid, nullptr, nullptr, s.rows, F, a.field_major_out, pi, st);
}

// CSR 1: the destination rows' lengths and labels
__global__ void __launch_bounds__(kBlock)
    k_shuffle_len(const int32_t* __restrict__ row_ptr, const float* __restrict__ lab_in,
                  float* __restrict__ lab_out, u32* __restrict__ len, int64_t rows, ShufflePerm pi) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= rows) return;
  const int64_t p = (int64_t)pi.at((u64)i);
  XF_DASSERT(p >= 0 && p < rows);
  len[i] = (u32)(row_ptr[p + 1] - row_ptr[p]);
  lab_out[i] = lab_in[p];
}

void launch_shuffle_len(const ShuffleArgs& a, hipStream_t st) {
  const BatchView& s = a.src;
  if (s.rows <= 0) return;
  const ShufflePerm pi = shuffle_perm((u64)s.rows, a.seed);
  hipLaunchKernelGGL(k_shuffle_len, dim3((unsigned)((s.rows + kBlock - 1) / kBlock)), dim3(kBlock),
                     0, st, s.row_ptr, s.labels, a.labels, a.len, s.rows, pi);
  XF_HIP_CHECK(hipGetLastError());
}

// CSR 3: the entries.  dst_ptr is the scanned row_ptr of the destination.
__global__ void __launch_bounds__(kBlock)
    k_shuffle_gather(const int32_t* __restrict__ src_ptr, const int32_t* __restrict__ dst_ptr,
                     const u64* __restrict__ keys, const int32_t* __restrict__ fgid,
                     u64* __restrict__ keys_out, int32_t* __restrict__ fgid_out, int64_t rows,
                     int64_t nnz, ShufflePerm pi) {
  __shared__ int32_t off[kShufGatherRows + 1];  // first entry of each destination row
  __shared__ int32_t sbase[kShufGatherRows];    // first entry of its source row
  const int64_t r0 = (int64_t)blockIdx.x * kShufGatherRows;
  const int nr = (int)(rows - r0 < kShufGatherRows ? rows - r0 : kShufGatherRows);
  const int t = threadIdx.x;
  if (t < nr) {
    const int64_t p = (int64_t)pi.at((u64)(r0 + t));
    XF_DASSERT(p >= 0 && p < rows);
    off[t] = dst_ptr[r0 + t];
    sbase[t] = src_ptr[p];
  }
  if (t == 0) off[nr] = dst_ptr[r0 + nr];
  __syncthreads();
  const int64_t e1 = off[nr];
  for (int64_t e = (int64_t)off[0] + t; e < e1; e += kBlock) {
    // the row of entry e: off[lo] <= e < off[lo + 1] (empty rows: equal offsets)
    int lo = 0, hi = nr;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (off[mid] <= e) lo = mid;
      else hi = mid;
    }
    const int64_t from = (int64_t)sbase[lo] + (e - off[lo]);
    // (a row_ptr that does not describe the batch must not reach past the arrays)
    if ((u64)from < (u64)nnz && (u64)e < (u64)nnz) {
      keys_out[e] = keys[from];
      if (fgid) fgid_out[e] = fgid[from];
    }
  }
}

void launch_shuffle_gather(const ShuffleArgs& a, hipStream_t st) {
  const BatchView& s = a.src;
  if (s.rows <= 0 || s.nnz <= 0) return;
  static_assert(kShufGatherRows == kBlock, "one lane stages one row");
  const ShufflePerm pi = shuffle_perm((u64)s.rows, a.seed);
  const int64_t g = (s.rows + kShufGatherRows - 1) / kShufGatherRows;
  hipLaunchKernelGGL(k_shuffle_gather, dim3((unsigned)g), dim3(kBlock), 0, st, s.row_ptr, a.row_ptr,
                     s.keys, s.fgid, a.keys, a.fgid, s.rows, s.nnz, pi);
  XF_HIP_CHECK(hipGetLastError());
}

}  // namespace hip
}  // namespace xflow
