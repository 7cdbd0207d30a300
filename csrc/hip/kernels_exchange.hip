// xflow-amd: helpers of the multi-rank step around the exchange (gfx950): the
// u32 exclusive scan, the dense packing of CSR gradient entries in send order
// and their per-owner totals, the worker-side gradient gather and the row
// scatter of received values.
#include "table_common.h"

namespace xflow {
namespace hip {

// ---------------------------------------------------------------------------
// CSR exchange helpers (the multi-rank step of several slices): exclusive
// scan of per-key entry counts, dense packing of the entries in send order,
// per-owner entry totals.
// ---------------------------------------------------------------------------
constexpr int kScanItems = 16;                     // u32 per lane
constexpr int kScanTile = kBlock * kScanItems;     // 4096 per workgroup

// 1: per-tile sums
__global__ void __launch_bounds__(kBlock) k_scan_tiles(const u32* __restrict__ in,
                                                       const int64_t* __restrict__ n_dev,
                                                       int64_t n_host, u32* __restrict__ tiles) {
  const int64_t n = n_dev ? *n_dev : n_host;
  const int64_t t0 = (int64_t)blockIdx.x * kScanTile;
  if (t0 >= n) return;
  u32 v = 0;
#pragma unroll
  for (int q = 0; q < kScanItems; ++q) {
    const int64_t i = t0 + (int64_t)threadIdx.x * kScanItems + q;
    if (i < n) v += in[i];
  }
  u32 tot;
  (void)block_exclusive_scan<kBlock>(v, &tot);
  if (threadIdx.x == 0) tiles[blockIdx.x] = tot;
}

// 2: exclusive scan of the tile sums (one workgroup), total into tiles[nt]
__global__ void __launch_bounds__(kScanBlock) k_scan_top(u32* __restrict__ tiles,
                                                         const int64_t* __restrict__ n_dev,
                                                         int64_t n_host) {
  const int64_t n = n_dev ? *n_dev : n_host;
  const int nt = (int)((n + kScanTile - 1) / kScanTile);
  u32 carry = 0;
  for (int c0 = 0; c0 < nt; c0 += kScanBlock) {
    const int i = c0 + (int)threadIdx.x;
    const u32 v = i < nt ? tiles[i] : 0u;
    u32 t;
    const u32 ex = block_exclusive_scan<kScanBlock>(v, &t);
    if (i < nt) tiles[i] = carry + ex;
    carry += t;
  }
  if (threadIdx.x == 0) tiles[nt] = carry;
}

// 3: out[i] = exclusive prefix, out[n] = total
__global__ void __launch_bounds__(kBlock) k_scan_write(const u32* __restrict__ in,
                                                       const int64_t* __restrict__ n_dev,
                                                       int64_t n_host, const u32* __restrict__ tiles,
                                                       u32* __restrict__ out) {
  const int64_t n = n_dev ? *n_dev : n_host;
  const int64_t t0 = (int64_t)blockIdx.x * kScanTile;
  if (t0 > n) return;
  const int nt = (int)((n + kScanTile - 1) / kScanTile);
  if (t0 == n) {  // (n a multiple of the tile: the total has no tile of its own)
    if (threadIdx.x == 0) out[n] = tiles[nt];
    return;
  }
  u32 loc[kScanItems], v = 0;
#pragma unroll
  for (int q = 0; q < kScanItems; ++q) {
    const int64_t i = t0 + (int64_t)threadIdx.x * kScanItems + q;
    loc[q] = i < n ? in[i] : 0u;
    v += loc[q];
  }
  u32 tot;
  u32 ex = tiles[blockIdx.x] + block_exclusive_scan<kBlock>(v, &tot);
#pragma unroll
  for (int q = 0; q < kScanItems; ++q) {
    const int64_t i = t0 + (int64_t)threadIdx.x * kScanItems + q;
    if (i < n) out[i] = ex;
    ex += loc[q];
  }
  if (blockIdx.x == (unsigned)(nt - 1) && threadIdx.x == kBlock - 1) out[n] = ex;
}

// small arrays (<= kScanBlock x kScanItems, e.g. the CSR applies' per-wave
// deferral counts): the whole scan in one launch of one workgroup
constexpr int64_t kScanOneMax = (int64_t)kScanBlock * kScanItems;
__global__ void __launch_bounds__(kScanBlock) k_scan_one(const u32* __restrict__ in,
                                                         const int64_t* __restrict__ n_dev,
                                                         int64_t n_max, u32* __restrict__ out) {
  int64_t n = n_dev ? *n_dev : n_max;
  if (n > n_max) n = n_max;
  u32 loc[kScanItems], v = 0;
#pragma unroll
  for (int q = 0; q < kScanItems; ++q) {
    const int64_t i = (int64_t)threadIdx.x * kScanItems + q;
    loc[q] = i < n ? in[i] : 0u;
    v += loc[q];
  }
  u32 tot;
  u32 ex = block_exclusive_scan<kScanBlock>(v, &tot);
#pragma unroll
  for (int q = 0; q < kScanItems; ++q) {
    const int64_t i = (int64_t)threadIdx.x * kScanItems + q;
    if (i < n) out[i] = ex;
    ex += loc[q];
  }
  if (threadIdx.x == 0) out[n] = tot;
}

static bool scan_one_enabled() {
  static const bool on = [] {
    const char* e = std::getenv("XFLOW_SCAN_ONE");
    return !(e && e[0] == '0');
  }();
  return on;
}

void launch_scan_u32(const u32* in, u32* out, const int64_t* n_dev, int64_t n_max, u32* tiles,
                     hipStream_t st) {
  if (n_max <= kScanOneMax && scan_one_enabled()) {
    hipLaunchKernelGGL(k_scan_one, dim3(1), dim3(kScanBlock), 0, st, in, n_dev, n_max, out);
    XF_HIP_CHECK(hipGetLastError());
    return;
  }
  const int g = (int)((n_max + kScanTile - 1) / kScanTile) + 1;
  hipLaunchKernelGGL(k_scan_tiles, dim3(g), dim3(kBlock), 0, st, in, n_dev, n_max, tiles);
  hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(kScanBlock), 0, st, tiles, n_dev, n_max);
  hipLaunchKernelGGL(k_scan_write, dim3(g), dim3(kBlock), 0, st, in, n_dev, n_max, tiles, out);
  XF_HIP_CHECK(hipGetLastError());
}

// entries of key i from the producer layout (off, cnt) to doff[i] (dense)
template <typename E>
__global__ void __launch_bounds__(kBlock) k_csr_pack(const u32* __restrict__ off,
                                                     const u32* __restrict__ cnt,
                                                     const E* __restrict__ src,
                                                     const u32* __restrict__ doff,
                                                     const int64_t* __restrict__ n_dev,
                                                     int64_t n_host, E* __restrict__ dst) {
  const int64_t n = n_dev ? *n_dev : n_host;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const u32 c = cnt[i], o = off[i], d = doff[i];
    for (u32 j = 0; j < c; ++j) dst[d + j] = src[o + j];
  }
}

// full-row entries (standard FM: m 16-byte words each)
__global__ void __launch_bounds__(kBlock) k_csr_pack_u4(const u32* __restrict__ off,
                                                        const u32* __restrict__ cnt,
                                                        const uint4* __restrict__ src,
                                                        const u32* __restrict__ doff,
                                                        const int64_t* __restrict__ n_dev,
                                                        int64_t n_host, int m,
                                                        uint4* __restrict__ dst) {
  const int64_t n = n_dev ? *n_dev : n_host;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const u32 c = cnt[i], o = off[i], d = doff[i];
    for (u32 j = 0; j < c * (u32)m; ++j) dst[(u64)d * m + j] = src[(u64)o * m + j];
  }
}

// per-owner entry totals: owner r's keys are the send-order range of the
// (decoded) key counts before it
__global__ void k_csr_totals(const int64_t* __restrict__ counts, int world, int encoded,
                             const u32* __restrict__ doff, int64_t* __restrict__ totals) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int64_t o = 0;
  for (int r = 0; r < world; ++r) {
    int64_t c = counts[r];
    if (encoded) c = (c & ((1ll << kCountBits) - 1)) - 1;
    c = c > 0 ? c : 0;
    totals[r] = (int64_t)doff[o + c] - (int64_t)doff[o];
    o += c;
  }
}

void launch_csr_pack(const u32* off, const u32* cnt, const void* src, const u32* doff,
                     const int64_t* n_dev, int64_t n_max, void* dst, int entry_bytes,
                     hipStream_t st) {
  const int g = grid_for(n_max);
  if (entry_bytes == 8)
    hipLaunchKernelGGL(k_csr_pack<u64>, dim3(g), dim3(kBlock), 0, st, off, cnt,
                       static_cast<const u64*>(src), doff, n_dev, n_max, static_cast<u64*>(dst));
  else if (entry_bytes == 12)
    hipLaunchKernelGGL(k_csr_pack<uint3>, dim3(g), dim3(kBlock), 0, st, off, cnt,
                       static_cast<const uint3*>(src), doff, n_dev, n_max, static_cast<uint3*>(dst));
  else if (entry_bytes > 0 && entry_bytes % 16 == 0)
    hipLaunchKernelGGL(k_csr_pack_u4, dim3(g), dim3(kBlock), 0, st, off, cnt,
                       static_cast<const uint4*>(src), doff, n_dev, n_max, entry_bytes / 16,
                       static_cast<uint4*>(dst));
  else throw std::runtime_error("csr_pack: entries of 8, 12 or 16k bytes");
  XF_HIP_CHECK(hipGetLastError());
}

void launch_csr_totals(const int64_t* counts, int world, bool encoded, const u32* doff,
                       int64_t* totals, hipStream_t st) {
  hipLaunchKernelGGL(k_csr_totals, dim3(1), dim3(kWave), 0, st, counts, world, encoded ? 1 : 0,
                     doff, totals);
  XF_HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// worker-side gradient gather (multi-rank path): pos-indexed raw sums ->
// owner-grouped send buffer, normalised per slice, source rows cleared.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) k_gather_grads(GatherGradArgs a) {
  int64_t n = dev_count(a.n_dev, a.n_max, a.n_max);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int S = a.S, ps = a.pstride, W = S * ps, wd = a.width ? a.width : ps;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    u32 row = a.map[i];
    float* __restrict__ src = a.grad_rw + (size_t)row * W;
    float* __restrict__ dst = a.out + (size_t)i * S * wd;
    for (int s = 0; s < S; ++s)
      for (int p = 0; p < wd; ++p) {
        dst[s * wd + p] = norm_grad(src[s * ps + p], a.slice_rows, s);
        src[s * ps + p] = 0.0f;
      }
    if (a.tmask_rw) {
      a.out_mask[i] = a.tmask_rw[row];
      a.tmask_rw[row] = 0u;
    }
  }
}

// The same with one thread per 16-byte unit (width and pstride multiples of
// 4): every unit's load is independent -- the row-per-thread loop above
// serialises a load -> store round trip per float (the stores may alias the
// next loads for the compiler), 225 us per MVM-10 rank-step in the emulated
// 8-GPU step.
__global__ void __launch_bounds__(kBlock) k_gather_grads4(GatherGradArgs a) {
  const int64_t n = dev_count(a.n_dev, a.n_max, a.n_max);
  const u32 S = (u32)a.S, ps4 = (u32)a.pstride / 4, wd4 = (u32)(a.width ? a.width : a.pstride) / 4;
  const u32 per = S * wd4;  // units per entry
  const u32 units = (u32)n * per;  // (< 2^32: checked by the launcher)
  const u32 stride = gridDim.x * blockDim.x;
  float4* __restrict__ g4 = reinterpret_cast<float4*>(a.grad_rw);
  float4* __restrict__ o4 = reinterpret_cast<float4*>(a.out);
  for (u32 u = blockIdx.x * blockDim.x + threadIdx.x; u < units; u += stride) {
    const u32 i = u / per;
    const u32 r = u - i * per, s = r / wd4, q = r - s * wd4;
    const u32 row = a.map[i];
    float4* sp = g4 + (u64)row * S * ps4 + (u64)s * ps4 + q;
    const float4 v = *sp;
    o4[u] = make_float4(norm_grad(v.x, a.slice_rows, (int)s), norm_grad(v.y, a.slice_rows, (int)s),
                        norm_grad(v.z, a.slice_rows, (int)s), norm_grad(v.w, a.slice_rows, (int)s));
    *sp = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (r == 0 && a.tmask_rw) {
      a.out_mask[i] = a.tmask_rw[row];
      a.tmask_rw[row] = 0u;
    }
  }
}

void launch_gather_grads(const GatherGradArgs& a, hipStream_t st) {
  if (a.n_max <= 0) return;
  const int wd = a.width ? a.width : a.pstride;
  const bool vec = a.pstride % 4 == 0 && wd % 4 == 0 &&
                   (double)a.n_max * a.S * (wd / 4) < 4294967295.0 &&
                   (reinterpret_cast<uintptr_t>(a.grad_rw) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(a.out) & 15) == 0;
  if (vec) {
    const int64_t units = a.n_max * (int64_t)a.S * (wd / 4);
    hipLaunchKernelGGL(k_gather_grads4, dim3(grid_for(units)), dim3(kBlock), 0, st, a);
  } else {
    hipLaunchKernelGGL(k_gather_grads, dim3(grid_for(a.n_max)), dim3(kBlock), 0, st, a);
  }
  XF_HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// row gather / scatter helpers
// ---------------------------------------------------------------------------
// width a multiple of 4: one thread per 16-byte unit, 32-bit index math (the
// element loop's 64-bit division per float dominated at MVM widths)
__global__ void k_scatter_rows4(const float4* __restrict__ src, float4* __restrict__ dst,
                                const u32* __restrict__ map, const int64_t* n_dev, int64_t n_max,
                                u32 w4, float* __restrict__ zero_out, int zero_width) {
  const int64_t rows = dev_count(n_dev, n_max, n_max);
  const u32 n = (u32)rows * w4;  // (< 2^32: checked by the launcher)
  const u32 stride = gridDim.x * blockDim.x;
  for (u32 e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
    const u32 i = e / w4;
    const u32 c = e - i * w4;
    const u64 r = map ? (u64)map[i] : (u64)i;
    dst[r * w4 + c] = src[e];
  }
  if (zero_out)
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows * zero_width;
         i += (int64_t)stride)
      zero_out[i] = 0.0f;
}

__global__ void k_scatter_rows(const float* __restrict__ src, float* __restrict__ dst,
                               const u32* __restrict__ map, const int64_t* n_dev, int64_t n_max,
                               int width, float* __restrict__ zero_out, int zero_width) {
  const int64_t rows = dev_count(n_dev, n_max, n_max), n = rows * width;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
    int64_t i = e / width;
    int c = (int)(e - i * width);
    int64_t r = map ? (int64_t)map[i] : i;
    dst[r * width + c] = src[e];
  }
  if (zero_out)  // the send buffer the reduction fills next (saves a memset launch)
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows * zero_width;
         i += stride)
      zero_out[i] = 0.0f;
}

void launch_scatter_rows(const float* src, float* dst, const u32* map, const int64_t* n_dev,
                         int64_t n_max, int width, float* zero_out, int zero_width,
                         hipStream_t st) {
  if (n_max <= 0) return;
  if (width % 4 == 0 && (double)n_max * width < 4294967295.0 &&
      (reinterpret_cast<uintptr_t>(src) & 15) == 0 &&
      (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
    hipLaunchKernelGGL(k_scatter_rows4, dim3(grid_for(n_max * width / 4)), dim3(kBlock), 0, st,
                       reinterpret_cast<const float4*>(src), reinterpret_cast<float4*>(dst), map,
                       n_dev, n_max, (u32)(width / 4), zero_out, zero_width);
    XF_HIP_CHECK(hipGetLastError());
    return;
  }
  hipLaunchKernelGGL(k_scatter_rows, dim3(grid_for(n_max * width)), dim3(kBlock), 0, st, src, dst,
                     map, n_dev, n_max, width, zero_out, zero_width);
  XF_HIP_CHECK(hipGetLastError());
}

}  // namespace hip
}  // namespace xflow
