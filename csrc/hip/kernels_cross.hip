// xflow-amd: feature crosses on the device (Backend::cross_rows, CrossArgs).
//
// Every row gains C keys, cross_key (common.h) of the row's raw keys of the
// crossed fields, appended behind its own entries.  The layout pass has each
// row in LDS anyway, so a cross reads the batch no second time: it costs the
// C columns it writes.
//
//   fixed width, row-major   k_cross_tile: k_shuffle_tile's pass over 64-row
//                tiles (kernels_shuffle.hip) -- the source row is pi(i) with a
//                seed, i without; u32 keys widen; field-major or row-major
//                out; labels ride along.  Once the tile is staged each (row,
//                cross) pair computes its key from LDS into tile column F + c,
//                and the write pass covers F + C columns.  With field ids the
//                tile's fgid is staged too, the operand is found by one scan
//                of the row in LDS, and the transposed fgid plus the cross
//                ids leave from the same launch (the shuffle takes two).
//                LDS: 64 x 65 x 8 B = 33.3 KB of keys (4 workgroups per CU's
//                160 KB), + 64 x 65 x 4 B = 16.6 KB of field ids = 49.9 KB
//                (3 per CU); both row strides are odd in their element size,
//                so the column reads of a wave hit distinct banks.
//   field-major, no fgid     k_cross_cols: one lane per row reads the m
//                operand columns coalesced and writes the cross column (and
//                copies the input columns unless crossing in place).
//   CSR          k_cross_csr, one launch: a workgroup owns 256 consecutive
//                rows = one contiguous entry range of source and destination,
//                keeps their offsets in LDS, copies the entries as
//                k_shuffle_gather does (binary search in LDS, the same guard
//                against a row_ptr that lies), appends each row's C keys --
//                rows of up to 64 entries one lane per (row, cross), longer
//                ones a wave per row -- and writes the destination's row_ptr.
#include <stdexcept>

#include "kernels.h"
#include "hip_util.h"

namespace xflow {
namespace hip {

constexpr int kCrossTileRows = 64;
constexpr int kCrossLd = kCrossMaxFields + 1;  // padded tile row (elements)
constexpr int kCrossCsrRows = kBlock;          // rows per k_cross_csr workgroup
constexpr int kCrossLongRow = 64;              // CSR rows above this get a wave

template <typename T, bool FM, bool FG>
__global__ void __launch_bounds__(kBlock)
    k_cross_tile(const T* __restrict__ src, const int32_t* __restrict__ fg_in,
                 u64* __restrict__ dst, int32_t* __restrict__ fg_out,
                 const float* __restrict__ lab_in, float* __restrict__ lab_out, int64_t rows, int F,
                 int64_t stride, CrossSpec x, bool has_seed, ShufflePerm pi) {
  __shared__ int64_t srow[kCrossTileRows];  // first element of the tile's source rows
  __shared__ u64 tile[kCrossTileRows * kCrossLd];
  __shared__ int32_t ftile[FG ? kCrossTileRows * kCrossLd : 1];
  const int C = x.n, W = F + C;  // W <= kCrossMaxFields (launch_cross_fixed)
  const int64_t r0 = (int64_t)blockIdx.x * kCrossTileRows;
  const int nr = (int)(rows - r0 < kCrossTileRows ? rows - r0 : kCrossTileRows);
  if ((int)threadIdx.x < nr) {
    const int64_t i = r0 + threadIdx.x;
    const int64_t p = has_seed ? (int64_t)pi.at((u64)i) : i;
    XF_DASSERT(p >= 0 && p < rows);
    srow[threadIdx.x] = p * F;
    if (lab_out) lab_out[i] = lab_in[p];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nr * F; i += kBlock) {
    const int r = i / F, f = i - r * F;
    tile[r * kCrossLd + f] = (u64)src[srow[r] + f];
    if constexpr (FG) ftile[r * kCrossLd + f] = fg_in[srow[r] + f];
  }
  __syncthreads();
  // (consecutive lanes take consecutive rows of one cross)
  for (int i = threadIdx.x; i < C * kCrossTileRows; i += kBlock) {
    const int c = i / kCrossTileRows, r = i - c * kCrossTileRows;
    if (r >= nr) continue;
    const int m = x.arity[c];
    u64 ops[kMaxCrossArity];
    if constexpr (FG) {
      int at[kMaxCrossArity] = {-1, -1, -1, -1};  // first occurrence of each operand's field
      for (int j = 0; j < F; ++j) {
        const int32_t g = ftile[r * kCrossLd + j];
#pragma unroll
        for (int k = 0; k < kMaxCrossArity; ++k)
          if (k < m && at[k] < 0 && g == x.field[c][k]) at[k] = j;
      }
#pragma unroll
      for (int k = 0; k < kMaxCrossArity; ++k)
        ops[k] = (k < m && at[k] >= 0) ? tile[r * kCrossLd + at[k]] : kNoGroup;
    } else {
#pragma unroll
      for (int k = 0; k < kMaxCrossArity; ++k) {
        const int32_t f = k < m ? x.field[c][k] : -1;
        ops[k] = (f >= 0 && f < F) ? tile[r * kCrossLd + f] : kNoGroup;
      }
    }
    tile[r * kCrossLd + F + c] = cross_key(x.field[c], ops, m);
    if constexpr (FG) ftile[r * kCrossLd + F + c] = x.fgid_base + c;
  }
  __syncthreads();
  if constexpr (FM) {
    for (int i = threadIdx.x; i < W * kCrossTileRows; i += kBlock) {
      const int f = i / kCrossTileRows, r = i - f * kCrossTileRows;
      if (r < nr) {
        dst[(int64_t)f * stride + r0 + r] = tile[r * kCrossLd + f];
        if constexpr (FG)
          if (fg_out) fg_out[(int64_t)f * stride + r0 + r] = ftile[r * kCrossLd + f];
      }
    }
  } else {
    u64* d = dst + r0 * W;  // the tile's destination rows are one contiguous run
    for (int i = threadIdx.x; i < nr * W; i += kBlock) {
      const int r = i / W, f = i - r * W;
      d[i] = tile[r * kCrossLd + f];
      if constexpr (FG)
        if (fg_out) fg_out[r0 * W + i] = ftile[r * kCrossLd + f];
    }
  }
}

template <typename T, bool FM, bool FG>
static void launch_tile(const CrossArgs& a, hipStream_t st) {
  const BatchView& s = a.src;
  const dim3 g((unsigned)((s.rows + kCrossTileRows - 1) / kCrossTileRows));
  const ShufflePerm pi = shuffle_perm((u64)s.rows, a.seed);
  hipLaunchKernelGGL((k_cross_tile<T, FM, FG>), g, dim3(kBlock), 0, st,
                     reinterpret_cast<const T*>(s.keys), s.fgid, a.keys, a.fgid, s.labels,
                     a.labels == s.labels ? nullptr : a.labels, s.rows, s.nnz_per_row,
                     cross_out_stride(a), a.spec, a.has_seed, pi);
  XF_HIP_CHECK(hipGetLastError());
}

template <typename T>
static void launch_tile_t(const CrossArgs& a, hipStream_t st) {
  const bool fg = a.src.fgid != nullptr;
  if (a.field_major_out) {
    if (fg) launch_tile<T, true, true>(a, st);
    else launch_tile<T, true, false>(a, st);
  } else {
    if (fg) launch_tile<T, false, true>(a, st);
    else launch_tile<T, false, false>(a, st);
  }
}

void launch_cross_fixed(const CrossArgs& a, hipStream_t st) {
  const BatchView& s = a.src;
  if (s.rows <= 0) return;
  // (the tile holds F + C columns)
  if (s.nnz_per_row + a.spec.n > kCrossMaxFields)
    throw std::invalid_argument("cross_rows: fields + crosses exceed 64");
  if (a.key_bytes == 4) launch_tile_t<u32>(a, st);
  else launch_tile_t<unsigned long long>(a, st);
}

// field-major source: blockIdx.y = output column (an input column's copy, or
// cross y - F)
__global__ void __launch_bounds__(kBlock)
    k_cross_cols(const u64* __restrict__ src, u64* __restrict__ dst,
                 const float* __restrict__ lab_in, float* __restrict__ lab_out, int64_t rows, int F,
                 int64_t sstride, int64_t dstride, int col0, CrossSpec x) {
  const int col = col0 + (int)blockIdx.y;
  const int64_t step = (int64_t)gridDim.x * kBlock;
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < rows; r += step) {
    if (blockIdx.y == 0 && lab_out) lab_out[r] = lab_in[r];
    if (col < F) {
      dst[(int64_t)col * dstride + r] = src[(int64_t)col * sstride + r];
      continue;
    }
    const int c = col - F, m = x.arity[c];
    u64 ops[kMaxCrossArity];
#pragma unroll
    for (int k = 0; k < kMaxCrossArity; ++k) {
      const int32_t f = k < m ? x.field[c][k] : -1;
      ops[k] = (f >= 0 && f < F) ? src[(int64_t)f * sstride + r] : kNoGroup;
    }
    dst[(int64_t)col * dstride + r] = cross_key(x.field[c], ops, m);
  }
}

void launch_cross_cols(const CrossArgs& a, hipStream_t st) {
  const BatchView& s = a.src;
  if (s.rows <= 0) return;
  const int F = s.nnz_per_row, C = a.spec.n;
  const bool in_place = a.keys == s.keys;  // (same stride: check_cross_args)
  const int col0 = in_place ? F : 0;
  const int64_t gx = grid_for(s.rows, kBlock, 1024);
  hipLaunchKernelGGL(k_cross_cols, dim3((unsigned)gx, (unsigned)(F + C - col0)), dim3(kBlock), 0,
                     st, s.keys, a.keys, s.labels, a.labels == s.labels ? nullptr : a.labels, s.rows,
                     F, s.col_stride, cross_out_stride(a), col0, a.spec);
  XF_HIP_CHECK(hipGetLastError());
}

// the smallest value over the wave
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}

__global__ void __launch_bounds__(kBlock)
    k_cross_csr(const int32_t* __restrict__ src_ptr, const u64* __restrict__ keys,
                const int32_t* __restrict__ fgid, const float* __restrict__ lab_in,
                int32_t* __restrict__ dst_ptr, u64* __restrict__ keys_out,
                int32_t* __restrict__ fgid_out, float* __restrict__ lab_out, int64_t rows,
                int64_t nnz, CrossSpec x) {
  __shared__ int32_t off[kCrossCsrRows + 1];  // first source entry of each row
  __shared__ int nlong;
  __shared__ int longrow[kCrossCsrRows];      // the tile's rows of more than kCrossLongRow entries
  const int C = x.n;
  const int64_t nnz_out = nnz + (int64_t)C * rows;
  const int64_t r0 = (int64_t)blockIdx.x * kCrossCsrRows;
  const int nr = (int)(rows - r0 < kCrossCsrRows ? rows - r0 : kCrossCsrRows);  // (0: no rows)
  const int t = threadIdx.x;
  if (t < nr) {
    const int32_t o = src_ptr[r0 + t];
    off[t] = o;
    dst_ptr[r0 + t] = (int32_t)(o + (int64_t)C * (r0 + t));
    if (lab_out) lab_out[r0 + t] = lab_in[r0 + t];
  }
  if (t == 0) {
    nlong = 0;
    const int32_t o = src_ptr[r0 + nr];  // (r0 + nr <= rows: row_ptr holds rows + 1)
    off[nr] = o;
    // (the last workgroup writes row_ptr[rows])
    if (r0 + nr == rows) dst_ptr[rows] = (int32_t)(o + (int64_t)C * rows);
  }
  __syncthreads();
  if (nr <= 0) return;
  if (t < nr && (int64_t)off[t + 1] - off[t] > kCrossLongRow) longrow[atomicAdd(&nlong, 1)] = t;
  // the entries: source entry e of row lo goes to e + C * (r0 + lo)
  const int64_t e1 = off[nr];
  for (int64_t e = (int64_t)off[0] + t; e < e1; e += kBlock) {
    // the row of entry e: off[lo] <= e < off[lo + 1] (empty rows: equal offsets)
    int lo = 0, hi = nr;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (off[mid] <= e) lo = mid;
      else hi = mid;
    }
    const int64_t to = e + (int64_t)C * (r0 + lo);
    // (a row_ptr that does not describe the batch must not reach past the arrays)
    if ((u64)e < (u64)nnz && (u64)to < (u64)nnz_out) {
      keys_out[to] = keys[e];
      if (fgid_out) fgid_out[to] = fgid[e];
    }
  }
  __syncthreads();  // (nlong, longrow)
  // short rows: one lane per (row, cross), one scan of the row for its operands
  for (int i = t; i < nr * C; i += kBlock) {
    const int r = i / C, c = i - r * C;
    int64_t b = off[r], e = off[r + 1];
    if (e - b > kCrossLongRow) continue;
    b = b < 0 ? 0 : b;
    e = e > nnz ? nnz : e;
    const int m = x.arity[c];
    int64_t at[kMaxCrossArity] = {-1, -1, -1, -1};
    for (int64_t j = b; j < e; ++j) {
      const int32_t g = fgid[j];
#pragma unroll
      for (int k = 0; k < kMaxCrossArity; ++k)
        if (k < m && at[k] < 0 && g == x.field[c][k]) at[k] = j;
    }
    u64 ops[kMaxCrossArity];
#pragma unroll
    for (int k = 0; k < kMaxCrossArity; ++k) ops[k] = (k < m && at[k] >= 0) ? keys[at[k]] : kNoGroup;
    const int64_t to = (int64_t)off[r + 1] + (int64_t)C * (r0 + r) + c;
    if ((u64)to < (u64)nnz_out) {
      keys_out[to] = cross_key(x.field[c], ops, m);
      if (fgid_out) fgid_out[to] = x.fgid_base + c;
    }
  }
  // long rows: a wave per row, the lanes stride over its entries
  const int lane = t % kWave, nl = nlong;
  for (int q = t / kWave; q < nl; q += kBlock / kWave) {
    const int r = longrow[q];
    int64_t b = off[r], e = off[r + 1];
    b = b < 0 ? 0 : b;
    e = e > nnz ? nnz : e;
    for (int c = 0; c < C; ++c) {
      const int m = x.arity[c];
      int at[kMaxCrossArity];  // first matching entry, relative to b (INT_MAX: none)
#pragma unroll
      for (int k = 0; k < kMaxCrossArity; ++k) at[k] = 0x7fffffff;
      for (int64_t j = b + lane; j < e; j += kWave) {
        const int32_t g = fgid[j];
#pragma unroll
        for (int k = 0; k < kMaxCrossArity; ++k)
          if (k < m && at[k] == 0x7fffffff && g == x.field[c][k]) at[k] = (int)(j - b);
      }
      u64 ops[kMaxCrossArity];
#pragma unroll
      for (int k = 0; k < kMaxCrossArity; ++k) {
        const int first = wave_min(at[k]);
        ops[k] = (k < m && first != 0x7fffffff) ? keys[b + first] : kNoGroup;
      }
      const int64_t to = (int64_t)off[r + 1] + (int64_t)C * (r0 + r) + c;
      if (lane == 0 && (u64)to < (u64)nnz_out) {
        keys_out[to] = cross_key(x.field[c], ops, m);
        if (fgid_out) fgid_out[to] = x.fgid_base + c;
      }
    }
  }
}

void launch_cross_csr(const CrossArgs& a, hipStream_t st) {
  const BatchView& s = a.src;
  static_assert(kCrossCsrRows == kBlock, "one lane stages one row");
  // (no rows: one workgroup still writes row_ptr[0])
  const int64_t g = s.rows > 0 ? (s.rows + kCrossCsrRows - 1) / kCrossCsrRows : 1;
  hipLaunchKernelGGL(k_cross_csr, dim3((unsigned)g), dim3(kBlock), 0, st, s.row_ptr, s.keys, s.fgid,
                     s.labels, a.row_ptr, a.keys, a.fgid, a.labels == s.labels ? nullptr : a.labels,
                     s.rows, s.nnz, a.spec);
  XF_HIP_CHECK(hipGetLastError());
}

}  // namespace hip
}  // namespace xflow
