// xflow-amd: device-side evaluation metrics (gfx950).
//
// Reference: Base::calculate_auc (/root/reference/src/base/base.h:84-110) --
// rank 0 sorts every test prediction by pctr (descending) with std::sort and
// walks them once: area += (#positives ranked above) for each negative,
// logloss += y*log2(p) + (1-y)*log2(1-p).  Here the test shard's predictions
// stay in HBM:
//
//   1. stable LSD radix sort of (key = ~bits(pctr), label) pairs, 4 passes of
//      8 bits (the key is eval_key_bits, backend.h: pctr > 0 keeps its float
//      bits, which order like the values, everything else is +0; ~ makes it
//      descending; ties keep prediction order), each pass
//        k_rs_hist     per-tile digit histograms (LDS)
//        k_rs_scan     per-digit exclusive scan over tiles (one workgroup per digit)
//        k_rs_scatter  stable scatter: per-wave digit match (8 ballots), wave
//                      counts combined in wave order through LDS
//   2. k_auc_pos / k_auc_area  positives per tile, then for every negative the
//      positives before it -- an exact int64 area (the reference accumulates it
//      in float, exact below 2^24)
//   3. k_logloss  log2 / ln likelihood terms in prediction order, fixed-order
//      double reductions (deterministic), no sort needed.
//
// Only the final scalars travel to the host (EvalMetrics).
#include <algorithm>
#include <cstring>

#include "kernels.h"
#include "hip_util.h"

namespace xflow {
namespace hip {

constexpr int kRsBlock = 1024;
constexpr int kRsItems = 4;
constexpr int kRsTile = kRsBlock * kRsItems;  // elements per tile (workgroup)
constexpr int kRsWaves = kRsBlock / kWave;
constexpr int kRsDigits = 256;

__global__ void __launch_bounds__(kRsBlock) k_rs_hist(const u32* __restrict__ keys, int64_t n,
                                                      int shift, u32* __restrict__ ghist,
                                                      int tiles) {
  __shared__ u32 h[kRsDigits];
  for (int d = threadIdx.x; d < kRsDigits; d += kRsBlock) h[d] = 0u;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * kRsTile;
#pragma unroll
  for (int t = 0; t < kRsItems; ++t) {
    const int64_t e = base + (int64_t)t * kRsBlock + threadIdx.x;
    if (e < n) atomicAdd(&h[(keys[e] >> shift) & 0xFFu], 1u);
  }
  __syncthreads();
  for (int d = threadIdx.x; d < kRsDigits; d += kRsBlock)
    ghist[(size_t)d * tiles + blockIdx.x] = h[d];
}

// one workgroup per digit: exclusive scan of the tiles' counts (in place), total
__global__ void __launch_bounds__(kBlock) k_rs_scan(u32* __restrict__ ghist, int tiles,
                                                    u32* __restrict__ tot) {
  const size_t row = (size_t)blockIdx.x * tiles;
  u32 carry = 0;
  for (int c0 = 0; c0 < tiles; c0 += kBlock) {
    const int i = c0 + (int)threadIdx.x;
    const u32 v = i < tiles ? ghist[row + i] : 0u;
    u32 t;
    const u32 ex = block_exclusive_scan<kBlock>(v, &t);
    if (i < tiles) ghist[row + i] = carry + ex;
    carry += t;
  }
  if (threadIdx.x == 0) tot[blockIdx.x] = carry;
}

__global__ void __launch_bounds__(kRsBlock) k_rs_scatter(const u32* __restrict__ keys,
                                                         const u32* __restrict__ vals, int64_t n,
                                                         int shift, const u32* __restrict__ ghist,
                                                         const u32* __restrict__ tot, int tiles,
                                                         u32* __restrict__ okeys,
                                                         u32* __restrict__ ovals) {
  __shared__ u32 base[kRsDigits];     // digit start + this tile's offset in the digit
  __shared__ u32 run[kRsDigits];      // elements of the digit placed by earlier rounds
  __shared__ u32 wcnt[kRsWaves][kRsDigits];
  const int lane = lane_id(), w = threadIdx.x / kWave;
  if (threadIdx.x < kRsDigits) {
    // exclusive scan of the 256 digit totals (sequential: 256 adds)
    u32 s = 0;
    for (int d = 0; d < (int)threadIdx.x; ++d) s += tot[d];
    base[threadIdx.x] = s + ghist[(size_t)threadIdx.x * tiles + blockIdx.x];
    run[threadIdx.x] = 0u;
  }
  const int64_t tb = (int64_t)blockIdx.x * kRsTile;
  for (int t = 0; t < kRsItems; ++t) {
    for (int i = threadIdx.x; i < kRsWaves * kRsDigits; i += kRsBlock) (&wcnt[0][0])[i] = 0u;
    __syncthreads();
    const int64_t e = tb + (int64_t)t * kRsBlock + threadIdx.x;
    const bool valid = e < n;
    const u32 k = valid ? keys[e] : 0u;
    const u32 dg = (k >> shift) & 0xFFu;
    // lanes of this wave with the same digit (match over the 8 digit bits)
    unsigned long long m = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const unsigned long long b = __ballot(valid && ((dg >> bit) & 1u));
      m &= ((dg >> bit) & 1u) ? b : ~b;
    }
    const u32 rank = (u32)__popcll(m & ((1ull << lane) - 1ull));
    if (valid && rank == 0) wcnt[w][dg] = (u32)__popcll(m);
    __syncthreads();
    if (threadIdx.x < kRsDigits) {  // wave-order prefix per digit
      u32 r = run[threadIdx.x];
      for (int ww = 0; ww < kRsWaves; ++ww) {
        const u32 c = wcnt[ww][threadIdx.x];
        wcnt[ww][threadIdx.x] = r;
        r += c;
      }
      run[threadIdx.x] = r;
    }
    __syncthreads();
    if (valid) {
      const u32 pos = base[dg] + wcnt[w][dg] + rank;
      okeys[pos] = k;
      ovals[pos] = vals[e];
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kBlock) k_auc_keys(const float* __restrict__ pctr,
                                                     const float* __restrict__ labels, int64_t n,
                                                     u32* __restrict__ keys, u32* __restrict__ vals) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    keys[i] = ~eval_key_bits(pctr[i]);  // descending pctr
    vals[i] = labels[i] > 0.5f ? 1u : 0u;
  }
}

// positives per tile of the sorted labels
__global__ void __launch_bounds__(kBlock) k_auc_pos(const u32* __restrict__ lab, int64_t n,
                                                    u32* __restrict__ bpos) {
  const int64_t base = (int64_t)blockIdx.x * kRsTile;
  u32 c = 0;
  for (int i = threadIdx.x; i < kRsTile; i += kBlock) {
    const int64_t e = base + i;
    if (e < n) c += lab[e];
  }
  u32 t;
  block_exclusive_scan<kBlock>(c, &t);
  if (threadIdx.x == 0) bpos[blockIdx.x] = t;
}

// exclusive scan of the tiles' positives (one workgroup), total in *tp
__global__ void __launch_bounds__(kBlock) k_auc_scan(u32* __restrict__ bpos, int tiles,
                                                     unsigned long long* __restrict__ tp) {
  unsigned long long carry = 0;
  for (int c0 = 0; c0 < tiles; c0 += kBlock) {
    const int i = c0 + (int)threadIdx.x;
    const u32 v = i < tiles ? bpos[i] : 0u;
    u32 t;
    const u32 ex = block_exclusive_scan<kBlock>(v, &t);
    if (i < tiles) bpos[i] = (u32)(carry + ex);
    carry += t;
  }
  if (threadIdx.x == 0) *tp = carry;
}

// per tile: sum over its negatives of the positives ranked above them (the
// tile's items in order: thread-contiguous runs of kRsItems)
__global__ void __launch_bounds__(kBlock) k_auc_area(const u32* __restrict__ lab, int64_t n,
                                                     const u32* __restrict__ bpos,
                                                     unsigned long long* __restrict__ part) {
  constexpr int kPer = kRsTile / kBlock;
  const int64_t base = (int64_t)blockIdx.x * kRsTile + (int64_t)threadIdx.x * kPer;
  u32 l[kPer];
  u32 c = 0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    l[j] = base + j < n ? lab[base + j] : 2u;  // 2: past the end
    c += l[j] == 1u;
  }
  u32 t;
  u32 before = bpos[blockIdx.x] + block_exclusive_scan<kBlock>(c, &t);
  unsigned long long area = 0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    if (l[j] == 1u) ++before;
    else if (l[j] == 0u) area += before;
  }
  __shared__ unsigned long long s[kBlock / kWave];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) area += __shfl_xor(area, o);
  if (threadIdx.x % kWave == 0) s[threadIdx.x / kWave] = area;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long a = 0;
    for (int i = 0; i < kBlock / kWave; ++i) a += s[i];
    part[blockIdx.x] = a;
  }
}

// log-likelihood terms in prediction order; per-workgroup double partials in a
// fixed order (deterministic)
constexpr int kLlGrid = 1024;

__global__ void __launch_bounds__(kBlock) k_logloss(const float* __restrict__ pctr,
                                                    const float* __restrict__ labels, int64_t n,
                                                    double* __restrict__ part) {
  double l2 = 0.0, ln = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float p = pctr[i];
    const int y = labels[i] > 0.5f ? 1 : 0;
    // base.h:98-99: y * log2(float p) + (1.0 - y) * log2(double 1 - p)
    l2 += (double)((float)y * log2f(p)) + (1.0 - y) * log2(1.0 - (double)p);
    const float pc = fminf(fmaxf(p, 1e-7f), 1.0f - 1e-7f);
    ln += y ? -log((double)pc) : -log(1.0 - (double)pc);
  }
  __shared__ double s2[kBlock / kWave], sl[kBlock / kWave];
  l2 = wave_sum(l2);
  ln = wave_sum(ln);
  if (threadIdx.x % kWave == 0) {
    s2[threadIdx.x / kWave] = l2;
    sl[threadIdx.x / kWave] = ln;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0, b = 0.0;
    for (int i = 0; i < kBlock / kWave; ++i) {
      a += s2[i];
      b += sl[i];
    }
    part[2 * blockIdx.x] = a;
    part[2 * blockIdx.x + 1] = b;
  }
}

// fixed-order final sums: out = {area (u64), log2 sum, ln sum}
__global__ void k_eval_final(const unsigned long long* __restrict__ apart, int tiles,
                             const double* __restrict__ lpart, int lblocks,
                             unsigned long long* __restrict__ area, double* __restrict__ sums) {
  if (threadIdx.x == 0) {
    unsigned long long a = 0;
    for (int i = 0; i < tiles; ++i) a += apart[i];
    *area = a;
  } else if (threadIdx.x == 1) {
    double l2 = 0.0, ln = 0.0;
    for (int i = 0; i < lblocks; ++i) {
      l2 += lpart[2 * i];
      ln += lpart[2 * i + 1];
    }
    sums[0] = l2;
    sums[1] = ln;
  }
}

void launch_eval_metrics(const float* pctr, const float* labels, int64_t n, EvalMetrics* out,
                         hipStream_t st) {
  *out = EvalMetrics();
  out->n = n;
  if (n <= 0) return;
  if (n >= (1ll << 31)) throw std::runtime_error("eval_metrics: at most 2^31-1 predictions");
  const int tiles = (int)((n + kRsTile - 1) / kRsTile);
  const int lblocks = (int)std::min<int64_t>(kLlGrid, (n + kBlock - 1) / kBlock);
  // workspace: 2 x (keys, vals) ping-pong, digit histograms, tile partials, results
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t o = off;
    off += (bytes + 255) & ~(size_t)255;
    return o;
  };
  const size_t o_k0 = take(4 * (size_t)n), o_v0 = take(4 * (size_t)n), o_k1 = take(4 * (size_t)n),
               o_v1 = take(4 * (size_t)n), o_h = take(4 * (size_t)kRsDigits * tiles),
               o_tot = take(4 * kRsDigits), o_bp = take(4 * (size_t)tiles),
               o_ap = take(8 * (size_t)tiles), o_lp = take(16 * (size_t)lblocks),
               o_res = take(8 * 4);
  char* ws = nullptr;
  XF_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&ws), off, st));
  u32* k0 = reinterpret_cast<u32*>(ws + o_k0);
  u32* v0 = reinterpret_cast<u32*>(ws + o_v0);
  u32* k1 = reinterpret_cast<u32*>(ws + o_k1);
  u32* v1 = reinterpret_cast<u32*>(ws + o_v1);
  u32* gh = reinterpret_cast<u32*>(ws + o_h);
  u32* tot = reinterpret_cast<u32*>(ws + o_tot);
  u32* bp = reinterpret_cast<u32*>(ws + o_bp);
  auto* ap = reinterpret_cast<unsigned long long*>(ws + o_ap);
  auto* lp = reinterpret_cast<double*>(ws + o_lp);
  auto* res = reinterpret_cast<unsigned long long*>(ws + o_res);  // area, tp, sums x2
  hipLaunchKernelGGL(k_auc_keys, dim3(grid_for(n)), dim3(kBlock), 0, st, pctr, labels, n, k0, v0);
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 8 * pass;
    hipLaunchKernelGGL(k_rs_hist, dim3(tiles), dim3(kRsBlock), 0, st, k0, n, shift, gh, tiles);
    hipLaunchKernelGGL(k_rs_scan, dim3(kRsDigits), dim3(kBlock), 0, st, gh, tiles, tot);
    hipLaunchKernelGGL(k_rs_scatter, dim3(tiles), dim3(kRsBlock), 0, st, k0, v0, n, shift, gh, tot,
                       tiles, k1, v1);
    std::swap(k0, k1);
    std::swap(v0, v1);
  }
  hipLaunchKernelGGL(k_auc_pos, dim3(tiles), dim3(kBlock), 0, st, v0, n, bp);
  hipLaunchKernelGGL(k_auc_scan, dim3(1), dim3(kBlock), 0, st, bp, tiles, res + 1);
  hipLaunchKernelGGL(k_auc_area, dim3(tiles), dim3(kBlock), 0, st, v0, n, bp, ap);
  hipLaunchKernelGGL(k_logloss, dim3(lblocks), dim3(kBlock), 0, st, pctr, labels, n, lp);
  hipLaunchKernelGGL(k_eval_final, dim3(1), dim3(64), 0, st, ap, tiles, lp, lblocks, res,
                     reinterpret_cast<double*>(res + 2));
  XF_HIP_CHECK(hipGetLastError());
  unsigned long long h[4];
  XF_HIP_CHECK(hipMemcpyAsync(h, res, sizeof(h), hipMemcpyDeviceToHost, st));
  XF_HIP_CHECK(hipFreeAsync(ws, st));
  XF_HIP_CHECK(hipStreamSynchronize(st));
  out->area = h[0];
  out->tp = (int64_t)h[1];
  double d[2];
  std::memcpy(d, h + 2, sizeof(d));
  out->log2_sum = d[0];
  out->ln_sum = d[1];
}

// ---- grouped evaluation (GroupedEval, backend.h) ---------------------------
//
//   1. k_grp_init      gk = group key, pv = eval_key_bits(pctr) << 1 | label per
//                      row; OR / AND of all group keys (which key bytes vary)
//   2. stable LSD radix sort of the (gk, pv) pairs, 8 bits a pass: 4 passes on
//      ~bits(pctr) (descending pctr), then one per byte of the group key that
//      is not the same in every row (k_gs_hist / k_rs_scan / k_gs_scatter).
//      After it the rows of a group are contiguous in ascending key order
//      (kNoGroup last), in descending pctr inside the group.
//   3. device-wide scans over the sorted rows (k_gr_tot / k_gr_carry /
//      k_gr_heads): positives, group heads, tie-run heads (group or pctr bits
//      differ from the predecessor) and the fixed-point pctr sum.  Every
//      tie-run head writes (row, positives before, pctr sum before, group)
//      at its run's rank, every group head its first run at its group's rank.
//   4. k_gr_runs / k_gr_carry64 / k_gr_runscan: a run of `neg` negatives and
//      `pos` positives adds neg * (2 * positives of its group in earlier runs
//      + pos) to the group's area2; exclusive u64 scan of these over the runs.
//   5. k_gr_groups: one lane per group; its sums are differences of the scans
//      at its first run and at the next group's (a group of any size, over
//      any number of tiles, is no special case).  Per-workgroup partials of
//      the two double sums in ascending group order, summed in tile order by
//      k_gr_final: a fixed order.  Integer atomics only (step 1).
constexpr int kGrPer = kRsTile / kBlock;  // sorted rows (runs) per thread, contiguous
constexpr u32 kGrMask = (1u << 21) - 1;   // three per-workgroup counts packed in a u64

enum : int { kGrPos = 0, kGrGroups, kGrRuns, kGrFx, kGrArea, kGrNoGroup, kGrUsed, kGrRows,
             kGrGauc, kGrCal, kGrOr, kGrNand, kGrWords };

// digit of pass d: 0..3 the bytes of ~bits(pctr), 4..11 the bytes of the group key
__device__ __forceinline__ u32 gs_digit(u64 g, u32 v, int d) {
  return d < 4 ? ((~(v >> 1)) >> (8 * d)) & 0xFFu : (u32)(g >> (8 * (d - 4))) & 0xFFu;
}

__device__ __forceinline__ long long gr_fx(u32 v) {
  return (long long)__builtin_rint((double)__uint_as_float(v >> 1) * 4294967296.0);
}

template <int BLOCK>
__device__ __forceinline__ unsigned long long block_exclusive_scan64(unsigned long long v,
                                                                     unsigned long long* total) {
  __shared__ unsigned long long wsum[BLOCK / kWave];
  const int lane = threadIdx.x % kWave, w = threadIdx.x / kWave;
  unsigned long long incl = v;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const unsigned long long t = __shfl_up(incl, o);
    if (lane >= o) incl += t;
  }
  if (lane == kWave - 1) wsum[w] = incl;
  __syncthreads();
  unsigned long long off = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < BLOCK / kWave; ++i) {
    off += (i < w) ? wsum[i] : 0ull;
    tot += wsum[i];
  }
  __syncthreads();
  *total = tot;
  return off + incl - v;
}

__global__ void __launch_bounds__(kBlock) k_grp_init(const float* __restrict__ pctr,
                                                     const float* __restrict__ labels,
                                                     const u64* __restrict__ groups, int64_t n,
                                                     u64* __restrict__ gk, u32* __restrict__ pv,
                                                     unsigned long long* __restrict__ res) {
  unsigned long long o = 0ull, na = 0ull;  // bits set in some key / clear in some key
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const u64 g = groups[i];
    gk[i] = g;
    pv[i] = (eval_key_bits(pctr[i]) << 1) | (labels[i] > 0.5f ? 1u : 0u);
    o |= g;
    na |= ~g;
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    o |= __shfl_xor(o, s);
    na |= __shfl_xor(na, s);
  }
  if (threadIdx.x % kWave == 0) {
    atomicOr(&res[kGrOr], o);
    atomicOr(&res[kGrNand], na);
  }
}

__global__ void __launch_bounds__(kRsBlock) k_gs_hist(const u64* __restrict__ gk,
                                                      const u32* __restrict__ pv, int64_t n, int d,
                                                      u32* __restrict__ ghist, int tiles) {
  __shared__ u32 h[kRsDigits];
  for (int i = threadIdx.x; i < kRsDigits; i += kRsBlock) h[i] = 0u;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * kRsTile;
#pragma unroll
  for (int t = 0; t < kRsItems; ++t) {
    const int64_t e = base + (int64_t)t * kRsBlock + threadIdx.x;
    if (e < n) atomicAdd(&h[d < 4 ? gs_digit(0ull, pv[e], d) : gs_digit(gk[e], 0u, d)], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kRsDigits; i += kRsBlock)
    ghist[(size_t)i * tiles + blockIdx.x] = h[i];
}

// k_rs_scatter for (u64 group key, u32 pctr bits | label) pairs and digit d
__global__ void __launch_bounds__(kRsBlock) k_gs_scatter(const u64* __restrict__ gk,
                                                         const u32* __restrict__ pv, int64_t n,
                                                         int d, const u32* __restrict__ ghist,
                                                         const u32* __restrict__ tot, int tiles,
                                                         u64* __restrict__ ogk,
                                                         u32* __restrict__ opv) {
  __shared__ u32 base[kRsDigits];
  __shared__ u32 run[kRsDigits];
  __shared__ u32 wcnt[kRsWaves][kRsDigits];
  const int lane = lane_id(), w = threadIdx.x / kWave;
  if (threadIdx.x < kRsDigits) {
    u32 s = 0;
    for (int i = 0; i < (int)threadIdx.x; ++i) s += tot[i];
    base[threadIdx.x] = s + ghist[(size_t)threadIdx.x * tiles + blockIdx.x];
    run[threadIdx.x] = 0u;
  }
  const int64_t tb = (int64_t)blockIdx.x * kRsTile;
  for (int t = 0; t < kRsItems; ++t) {
    for (int i = threadIdx.x; i < kRsWaves * kRsDigits; i += kRsBlock) (&wcnt[0][0])[i] = 0u;
    __syncthreads();
    const int64_t e = tb + (int64_t)t * kRsBlock + threadIdx.x;
    const bool valid = e < n;
    const u64 g = valid ? gk[e] : 0ull;
    const u32 v = valid ? pv[e] : 0u;
    const u32 dg = gs_digit(g, v, d);
    unsigned long long m = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const unsigned long long b = __ballot(valid && ((dg >> bit) & 1u));
      m &= ((dg >> bit) & 1u) ? b : ~b;
    }
    const u32 rank = (u32)__popcll(m & ((1ull << lane) - 1ull));
    if (valid && rank == 0) wcnt[w][dg] = (u32)__popcll(m);
    __syncthreads();
    if (threadIdx.x < kRsDigits) {  // wave-order prefix per digit
      u32 r = run[threadIdx.x];
      for (int ww = 0; ww < kRsWaves; ++ww) {
        const u32 c = wcnt[ww][threadIdx.x];
        wcnt[ww][threadIdx.x] = r;
        r += c;
      }
      run[threadIdx.x] = r;
    }
    __syncthreads();
    if (valid) {
      const u32 pos = base[dg] + wcnt[w][dg] + rank;
      XF_DASSERT((int64_t)pos < n);
      ogk[pos] = g;
      opv[pos] = v;
    }
    __syncthreads();
  }
}

// a thread's kGrPer contiguous sorted rows from `base`: their pv words, bit j
// of gh / rh set when row j is a group / tie-run head; returns the rows < n
__device__ __forceinline__ int gr_load(const u64* __restrict__ gk, const u32* __restrict__ pv,
                                       int64_t n, int64_t base, u32 (&v)[kGrPer], u32& gh,
                                       u32& rh) {
  gh = rh = 0u;
  int cnt = 0;
  u64 pk = 0ull;
  u32 pb = 0u;
  if (base > 0 && base - 1 < n) {
    pk = gk[base - 1];
    pb = pv[base - 1] >> 1;
  }
#pragma unroll
  for (int j = 0; j < kGrPer; ++j) {
    const int64_t e = base + j;
    v[j] = 0u;
    if (e < n) {
      const u64 k = gk[e];
      v[j] = pv[e];
      const bool g = e == 0 || k != pk;
      const bool r = g || (v[j] >> 1) != pb;
      gh |= (g ? 1u : 0u) << j;
      rh |= (r ? 1u : 0u) << j;
      pk = k;
      pb = v[j] >> 1;
      cnt = j + 1;
    }
  }
  return cnt;
}

// per tile of the sorted rows: positives, group heads, run heads, pctr sum
__global__ void __launch_bounds__(kBlock) k_gr_tot(const u64* __restrict__ gk,
                                                   const u32* __restrict__ pv, int64_t n,
                                                   u32* __restrict__ tp, u32* __restrict__ tg,
                                                   u32* __restrict__ tr,
                                                   unsigned long long* __restrict__ ts) {
  const int64_t base = (int64_t)blockIdx.x * kRsTile + (int64_t)threadIdx.x * kGrPer;
  u32 v[kGrPer], gh, rh;
  const int cnt = gr_load(gk, pv, n, base, v, gh, rh);
  unsigned long long pos = 0, fx = 0;
#pragma unroll
  for (int j = 0; j < kGrPer; ++j) {
    if (j < cnt) {
      pos += v[j] & 1u;
      fx += (unsigned long long)gr_fx(v[j]);
    }
  }
  unsigned long long tc, tf;
  block_exclusive_scan64<kBlock>(
      pos | ((unsigned long long)__popc(gh) << 21) | ((unsigned long long)__popc(rh) << 42), &tc);
  block_exclusive_scan64<kBlock>(fx, &tf);
  if (threadIdx.x == 0) {
    tp[blockIdx.x] = (u32)tc & kGrMask;
    tg[blockIdx.x] = (u32)(tc >> 21) & kGrMask;
    tr[blockIdx.x] = (u32)(tc >> 42);
    ts[blockIdx.x] = tf;
  }
}

// exclusive scans of the tiles' four totals (one workgroup), totals in res
__global__ void __launch_bounds__(kBlock) k_gr_carry(u32* __restrict__ tp, u32* __restrict__ tg,
                                                     u32* __restrict__ tr,
                                                     unsigned long long* __restrict__ ts, int tiles,
                                                     unsigned long long* __restrict__ res) {
  unsigned long long cp = 0, cg = 0, cr = 0, cs = 0;
  for (int c0 = 0; c0 < tiles; c0 += kBlock) {
    const int i = c0 + (int)threadIdx.x;
    const bool in = i < tiles;
    unsigned long long t;
    unsigned long long ex = block_exclusive_scan64<kBlock>(in ? tp[i] : 0u, &t);
    if (in) tp[i] = (u32)(cp + ex);
    cp += t;
    ex = block_exclusive_scan64<kBlock>(in ? tg[i] : 0u, &t);
    if (in) tg[i] = (u32)(cg + ex);
    cg += t;
    ex = block_exclusive_scan64<kBlock>(in ? tr[i] : 0u, &t);
    if (in) tr[i] = (u32)(cr + ex);
    cr += t;
    ex = block_exclusive_scan64<kBlock>(in ? ts[i] : 0ull, &t);
    if (in) ts[i] = cs + ex;
    cs += t;
  }
  if (threadIdx.x == 0) {
    res[kGrPos] = cp;
    res[kGrGroups] = cg;
    res[kGrRuns] = cr;
    res[kGrFx] = cs;
  }
}

// run heads write their run's record at its rank, group heads their first run
// at the group's rank; the last row closes both lists (entries [runs], [groups])
__global__ void __launch_bounds__(kBlock) k_gr_heads(
    const u64* __restrict__ gk, const u32* __restrict__ pv, int64_t n, const u32* __restrict__ tp,
    const u32* __restrict__ tg, const u32* __restrict__ tr,
    const unsigned long long* __restrict__ ts, u32* __restrict__ runpos, u32* __restrict__ runP,
    u32* __restrict__ runG, unsigned long long* __restrict__ runS, u32* __restrict__ grpRun) {
  const int64_t base = (int64_t)blockIdx.x * kRsTile + (int64_t)threadIdx.x * kGrPer;
  u32 v[kGrPer], gh, rh;
  const int cnt = gr_load(gk, pv, n, base, v, gh, rh);
  unsigned long long pos = 0, fx = 0;
#pragma unroll
  for (int j = 0; j < kGrPer; ++j) {
    if (j < cnt) {
      pos += v[j] & 1u;
      fx += (unsigned long long)gr_fx(v[j]);
    }
  }
  unsigned long long tc, tf;
  const unsigned long long ex = block_exclusive_scan64<kBlock>(
      pos | ((unsigned long long)__popc(gh) << 21) | ((unsigned long long)__popc(rh) << 42), &tc);
  const unsigned long long exs = block_exclusive_scan64<kBlock>(fx, &tf);
  u32 P = tp[blockIdx.x] + ((u32)ex & kGrMask);
  u32 G = tg[blockIdx.x] + ((u32)(ex >> 21) & kGrMask);
  u32 R = tr[blockIdx.x] + (u32)(ex >> 42);
  unsigned long long S = ts[blockIdx.x] + exs;
#pragma unroll
  for (int j = 0; j < kGrPer; ++j) {
    if (j < cnt) {
      if ((rh >> j) & 1u) {
        const bool g = (gh >> j) & 1u;
        XF_DASSERT((int64_t)R < n && (int64_t)G <= n);
        runpos[R] = (u32)(base + j);
        runP[R] = P;
        runS[R] = S;
        runG[R] = g ? G : G - 1u;
        if (g) grpRun[G++] = R;
        ++R;
      }
      P += v[j] & 1u;
      S += (unsigned long long)gr_fx(v[j]);
    }
  }
  if (cnt > 0 && base + cnt == n) {
    runpos[R] = (u32)n;
    runP[R] = P;
    runS[R] = S;
    grpRun[G] = R;
  }
}

// c[j] of run j: negatives * (2 * positives of the group in earlier runs +
// the run's positives); tile totals
__global__ void __launch_bounds__(kBlock) k_gr_runs(const u32* __restrict__ runpos,
                                                    const u32* __restrict__ runP,
                                                    const u32* __restrict__ runG,
                                                    const u32* __restrict__ grpRun,
                                                    const unsigned long long* __restrict__ res,
                                                    unsigned long long* __restrict__ runA,
                                                    unsigned long long* __restrict__ ta) {
  const int64_t runs = (int64_t)res[kGrRuns];
  const int64_t base = (int64_t)blockIdx.x * kRsTile + (int64_t)threadIdx.x * kGrPer;
  unsigned long long sum = 0;
  for (int j = 0; j < kGrPer; ++j) {
    const int64_t r = base + j;
    if (r < runs) {
      const u32 p0 = runP[r];
      const unsigned long long pos = runP[r + 1] - p0;
      const unsigned long long neg = (runpos[r + 1] - runpos[r]) - pos;
      const unsigned long long before = p0 - runP[grpRun[runG[r]]];
      const unsigned long long c = neg * (2ull * before + pos);
      runA[r] = c;
      sum += c;
    }
  }
  unsigned long long t;
  block_exclusive_scan64<kBlock>(sum, &t);
  if (threadIdx.x == 0) ta[blockIdx.x] = t;
}

__global__ void __launch_bounds__(kBlock) k_gr_carry64(unsigned long long* __restrict__ ta,
                                                       int tiles,
                                                       unsigned long long* __restrict__ total) {
  unsigned long long carry = 0;
  for (int c0 = 0; c0 < tiles; c0 += kBlock) {
    const int i = c0 + (int)threadIdx.x;
    unsigned long long t;
    const unsigned long long ex = block_exclusive_scan64<kBlock>(i < tiles ? ta[i] : 0ull, &t);
    if (i < tiles) ta[i] = carry + ex;
    carry += t;
  }
  if (threadIdx.x == 0) *total = carry;
}

// runA: c[j] -> the exclusive prefix of c over the runs (in place), runA[runs] = total
__global__ void __launch_bounds__(kBlock) k_gr_runscan(unsigned long long* __restrict__ runA,
                                                       const unsigned long long* __restrict__ ta,
                                                       const unsigned long long* __restrict__ res) {
  const int64_t runs = (int64_t)res[kGrRuns];
  const int64_t base = (int64_t)blockIdx.x * kRsTile + (int64_t)threadIdx.x * kGrPer;
  unsigned long long c[kGrPer], sum = 0;
#pragma unroll
  for (int j = 0; j < kGrPer; ++j) {
    c[j] = base + j < runs ? runA[base + j] : 0ull;
    sum += c[j];
  }
  unsigned long long t;
  unsigned long long a = ta[blockIdx.x] + block_exclusive_scan64<kBlock>(sum, &t);
#pragma unroll
  for (int j = 0; j < kGrPer; ++j) {
    if (base + j < runs) {
      runA[base + j] = a;
      a += c[j];
      if (base + j == runs - 1) runA[runs] = a;
    }
  }
}

// one lane per group, groups of a workgroup in ascending order per lane and
// over the lanes; per-workgroup partials {gauc_num, cal_abs}, {used, rows_used}
__global__ void __launch_bounds__(kBlock) k_gr_groups(
    const u64* __restrict__ gk, const u32* __restrict__ runpos, const u32* __restrict__ runP,
    const unsigned long long* __restrict__ runS, const unsigned long long* __restrict__ runA,
    const u32* __restrict__ grpRun, unsigned long long* __restrict__ res, u64* __restrict__ tkey,
    long long* __restrict__ tn, long long* __restrict__ tpos,
    unsigned long long* __restrict__ tarea, long long* __restrict__ tsump,
    double* __restrict__ pd, unsigned long long* __restrict__ pu) {
  const int64_t ngroups = (int64_t)res[kGrGroups];
  double gauc = 0.0, cal = 0.0;
  unsigned long long used = 0, rows = 0;
  for (int j = 0; j < kGrPer; ++j) {
    const int64_t k = (int64_t)blockIdx.x * kRsTile + (int64_t)j * kBlock + threadIdx.x;
    if (k >= ngroups) break;
    const u32 r0 = grpRun[k], r1 = grpRun[k + 1];
    const u64 key = gk[runpos[r0]];
    const long long ng = (long long)(runpos[r1] - runpos[r0]);
    const long long pos = (long long)(runP[r1] - runP[r0]);
    const unsigned long long area2 = runA[r1] - runA[r0];
    const long long sump = (long long)(runS[r1] - runS[r0]);
    if (key == kNoGroup) {  // (the last group)
      res[kGrNoGroup] = (unsigned long long)ng;
      continue;
    }
    if (tkey) {
      tkey[k] = key;
      tn[k] = ng;
      tpos[k] = pos;
      tarea[k] = area2;
      tsump[k] = sump;
    }
    if (pos > 0 && pos < ng) {
      ++used;
      rows += (unsigned long long)ng;
      gauc += group_auc_term(ng, pos, area2);
    }
    cal += group_cal_term(sump, pos);
  }
  __shared__ double sd[2][kBlock / kWave];
  __shared__ unsigned long long su[2][kBlock / kWave];
  gauc = wave_sum(gauc);
  cal = wave_sum(cal);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    used += __shfl_xor(used, o);
    rows += __shfl_xor(rows, o);
  }
  if (threadIdx.x % kWave == 0) {
    sd[0][threadIdx.x / kWave] = gauc;
    sd[1][threadIdx.x / kWave] = cal;
    su[0][threadIdx.x / kWave] = used;
    su[1][threadIdx.x / kWave] = rows;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    double a = 0.0;
    unsigned long long b = 0;
    for (int i = 0; i < kBlock / kWave; ++i) {
      a += sd[threadIdx.x][i];
      b += su[threadIdx.x][i];
    }
    pd[2 * blockIdx.x + threadIdx.x] = a;
    pu[2 * blockIdx.x + threadIdx.x] = b;
  }
}

// fixed-order sums of the workgroups' partials
__global__ void k_gr_final(const double* __restrict__ pd, const unsigned long long* __restrict__ pu,
                           int tiles, unsigned long long* __restrict__ res) {
  if (threadIdx.x < 2) {
    double a = 0.0;
    for (int i = 0; i < tiles; ++i) a += pd[2 * i + threadIdx.x];
    reinterpret_cast<double*>(res)[kGrGauc + threadIdx.x] = a;
  } else if (threadIdx.x < 4) {
    unsigned long long b = 0;
    for (int i = 0; i < tiles; ++i) b += pu[2 * i + (threadIdx.x - 2)];
    res[kGrUsed + (threadIdx.x - 2)] = b;
  }
}

void launch_eval_grouped(const float* pctr, const float* labels, const u64* groups, int64_t n,
                         GroupedEval* out, GroupTable* table, hipStream_t st) {
  *out = GroupedEval();
  if (table) *table = GroupTable();
  out->n = n;
  if (n <= 0) return;
  if (n >= (1ll << 31)) throw std::runtime_error("eval_grouped: at most 2^31-1 predictions");
  const int tiles = (int)((n + kRsTile - 1) / kRsTile);
  const size_t N = (size_t)n, N1 = N + 1;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t o = off;
    off += (bytes + 255) & ~(size_t)255;
    return o;
  };
  // workspace: 2 x (gk, pv) ping-pong, digit histograms, run / group lists,
  // tile totals and partials, results, the table when asked for
  const size_t o_k0 = take(8 * N), o_k1 = take(8 * N), o_v0 = take(4 * N), o_v1 = take(4 * N),
               o_h = take(4 * (size_t)kRsDigits * tiles), o_tot = take(4 * kRsDigits),
               o_rpos = take(4 * N1), o_rp = take(4 * N1), o_rg = take(4 * N1),
               o_rs = take(8 * N1), o_ra = take(8 * N1), o_gr = take(4 * N1),
               o_tp = take(4 * (size_t)tiles), o_tg = take(4 * (size_t)tiles),
               o_tr = take(4 * (size_t)tiles), o_ts = take(8 * (size_t)tiles),
               o_ta = take(8 * (size_t)tiles), o_pd = take(16 * (size_t)tiles),
               o_pu = take(16 * (size_t)tiles), o_res = take(8 * kGrWords),
               o_tab = take(table ? 5 * 8 * N : 0);
  char* ws = nullptr;
  XF_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&ws), off, st));
  using ull = unsigned long long;
  u64* k0 = reinterpret_cast<u64*>(ws + o_k0);
  u64* k1 = reinterpret_cast<u64*>(ws + o_k1);
  u32* v0 = reinterpret_cast<u32*>(ws + o_v0);
  u32* v1 = reinterpret_cast<u32*>(ws + o_v1);
  u32* gh = reinterpret_cast<u32*>(ws + o_h);
  u32* tot = reinterpret_cast<u32*>(ws + o_tot);
  u32* rpos = reinterpret_cast<u32*>(ws + o_rpos);
  u32* rp = reinterpret_cast<u32*>(ws + o_rp);
  u32* rg = reinterpret_cast<u32*>(ws + o_rg);
  ull* rs = reinterpret_cast<ull*>(ws + o_rs);
  ull* ra = reinterpret_cast<ull*>(ws + o_ra);
  u32* gr = reinterpret_cast<u32*>(ws + o_gr);
  u32* tp = reinterpret_cast<u32*>(ws + o_tp);
  u32* tg = reinterpret_cast<u32*>(ws + o_tg);
  u32* tr = reinterpret_cast<u32*>(ws + o_tr);
  ull* ts = reinterpret_cast<ull*>(ws + o_ts);
  ull* ta = reinterpret_cast<ull*>(ws + o_ta);
  double* pd = reinterpret_cast<double*>(ws + o_pd);
  ull* pu = reinterpret_cast<ull*>(ws + o_pu);
  ull* res = reinterpret_cast<ull*>(ws + o_res);
  u64* tkey = table ? reinterpret_cast<u64*>(ws + o_tab) : nullptr;
  long long* tn = reinterpret_cast<long long*>(tkey ? tkey + N : nullptr);
  long long* tpos = tkey ? tn + N : nullptr;
  ull* tarea = reinterpret_cast<ull*>(tkey ? tpos + N : nullptr);
  long long* tsump = reinterpret_cast<long long*>(tkey ? tarea + N : nullptr);
  XF_HIP_CHECK(hipMemsetAsync(res, 0, 8 * kGrWords, st));
  hipLaunchKernelGGL(k_grp_init, dim3(grid_for(n)), dim3(kBlock), 0, st, pctr, labels, groups, n,
                     k0, v0, res);
  // the group-key bytes that differ between rows: the others need no pass
  ull bits[2];
  XF_HIP_CHECK(hipMemcpyAsync(bits, res + kGrOr, sizeof(bits), hipMemcpyDeviceToHost, st));
  XF_HIP_CHECK(hipStreamSynchronize(st));
  const ull varies = bits[0] & bits[1];
  for (int d = 0; d < 12; ++d) {
    if (d >= 4 && ((varies >> (8 * (d - 4))) & 0xFFull) == 0) continue;
    hipLaunchKernelGGL(k_gs_hist, dim3(tiles), dim3(kRsBlock), 0, st, k0, v0, n, d, gh, tiles);
    hipLaunchKernelGGL(k_rs_scan, dim3(kRsDigits), dim3(kBlock), 0, st, gh, tiles, tot);
    hipLaunchKernelGGL(k_gs_scatter, dim3(tiles), dim3(kRsBlock), 0, st, k0, v0, n, d, gh, tot,
                       tiles, k1, v1);
    std::swap(k0, k1);
    std::swap(v0, v1);
  }
  hipLaunchKernelGGL(k_gr_tot, dim3(tiles), dim3(kBlock), 0, st, k0, v0, n, tp, tg, tr, ts);
  hipLaunchKernelGGL(k_gr_carry, dim3(1), dim3(kBlock), 0, st, tp, tg, tr, ts, tiles, res);
  hipLaunchKernelGGL(k_gr_heads, dim3(tiles), dim3(kBlock), 0, st, k0, v0, n, tp, tg, tr, ts, rpos,
                     rp, rg, rs, gr);
  hipLaunchKernelGGL(k_gr_runs, dim3(tiles), dim3(kBlock), 0, st, rpos, rp, rg, gr, res, ra, ta);
  hipLaunchKernelGGL(k_gr_carry64, dim3(1), dim3(kBlock), 0, st, ta, tiles, res + kGrArea);
  hipLaunchKernelGGL(k_gr_runscan, dim3(tiles), dim3(kBlock), 0, st, ra, ta, res);
  hipLaunchKernelGGL(k_gr_groups, dim3(tiles), dim3(kBlock), 0, st, k0, rpos, rp, rs, ra, gr, res,
                     tkey, tn, tpos, tarea, tsump, pd, pu);
  hipLaunchKernelGGL(k_gr_final, dim3(1), dim3(64), 0, st, pd, pu, tiles, res);
  XF_HIP_CHECK(hipGetLastError());
  ull h[kGrWords];
  XF_HIP_CHECK(hipMemcpyAsync(h, res, sizeof(h), hipMemcpyDeviceToHost, st));
  XF_HIP_CHECK(hipStreamSynchronize(st));
  out->n_nogroup = (int64_t)h[kGrNoGroup];
  out->groups = (int64_t)h[kGrGroups] - (out->n_nogroup > 0 ? 1 : 0);
  out->groups_used = (int64_t)h[kGrUsed];
  out->rows_used = (int64_t)h[kGrRows];
  std::memcpy(&out->gauc_num, &h[kGrGauc], sizeof(double));
  std::memcpy(&out->cal_abs, &h[kGrCal], sizeof(double));
  if (table && out->groups > 0) {
    const size_t G = (size_t)out->groups;
    table->key.resize(G);
    table->n.resize(G);
    table->pos.resize(G);
    table->area2.resize(G);
    table->sump.resize(G);
    XF_HIP_CHECK(hipMemcpyAsync(table->key.data(), tkey, 8 * G, hipMemcpyDeviceToHost, st));
    XF_HIP_CHECK(hipMemcpyAsync(table->n.data(), tn, 8 * G, hipMemcpyDeviceToHost, st));
    XF_HIP_CHECK(hipMemcpyAsync(table->pos.data(), tpos, 8 * G, hipMemcpyDeviceToHost, st));
    XF_HIP_CHECK(hipMemcpyAsync(table->area2.data(), tarea, 8 * G, hipMemcpyDeviceToHost, st));
    XF_HIP_CHECK(hipMemcpyAsync(table->sump.data(), tsump, 8 * G, hipMemcpyDeviceToHost, st));
  }
  XF_HIP_CHECK(hipFreeAsync(ws, st));
  XF_HIP_CHECK(hipStreamSynchronize(st));
}

__global__ void __launch_bounds__(kBlock) k_row_group_key(BatchView b, int field,
                                                          u64* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < b.rows; r += stride)
    out[r] = row_group_key(b, r, field);
}

void launch_row_group_keys(const BatchView& b, int field, u64* out, hipStream_t st) {
  if (b.rows <= 0) return;
  hipLaunchKernelGGL(k_row_group_key, dim3(grid_for(b.rows)), dim3(kBlock), 0, st, b, field, out);
  XF_HIP_CHECK(hipGetLastError());
}

}  // namespace hip
}  // namespace xflow
