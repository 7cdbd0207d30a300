// xflow-amd: gfx950 kernels for the HBM-resident sparse parameter store.
//
// Replaces the ps-lite KVServer + unordered_map store of the reference
// (ftrl.h:38-152, server.h:20-35) and the worker-side sort/unique key
// preparation (lr_worker.cc:146-166).  The store's kernels by concern:
//
//   kernels_dedup.hip     key preparation: dedup scratch, compaction
//   kernels_pull.hip      probe / insert, pull values, feature admission
//   kernels_apply.hip     the optimiser push, owner grouping
//   kernels_exchange.hip  scan, CSR wire packing, gradient gather, row scatter
//   this file             fill / small copies / snapshot / clear, checkpoint
//                         export and import, growth by segment splits, pruning,
//                         prefill, the sparsity count, the delta-checkpoint filter
//
// All of them are memory-latency bound (random 16-64 B accesses): they keep
// several independent probes in flight per lane, count bookkeeping with one
// atomic per workgroup (single-address atomics serialise), and read
// device-side element counts so a whole step runs without host syncs.
#include "table_common.h"

namespace xflow {
namespace hip {

__global__ void k_fill_u64(u64* p, u64 v, size_t n) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = v;
}

struct SmallBytes {
  unsigned char b[256];
};

__global__ void k_upload_small(unsigned char* __restrict__ dst, SmallBytes v, int n) {
  for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = v.b[i];
}

void launch_upload_small(void* dst, const void* src, size_t bytes, hipStream_t st) {
  if (bytes == 0) return;
  if (bytes > sizeof(SmallBytes)) throw std::runtime_error("upload_small: at most 256 bytes");
  SmallBytes v;
  std::memcpy(v.b, src, bytes);
  hipLaunchKernelGGL(k_upload_small, dim3(1), dim3(64), 0, st, static_cast<unsigned char*>(dst),
                     v, (int)bytes);
  XF_HIP_CHECK(hipGetLastError());
}

// (e.g. the sharded step's split sizes into pinned memory: a copy-engine D2H
// left ~6 us of idle GPU behind it per step)
__global__ void k_download_small(unsigned char* __restrict__ dst,
                                 const unsigned char* __restrict__ src, int n) {
  for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
}

void launch_download_small(void* host_dst, const void* src, size_t bytes, hipStream_t st) {
  if (bytes == 0) return;
  if (bytes > (1u << 16)) throw std::runtime_error("download_small: at most 64 KB");
  hipLaunchKernelGGL(k_download_small, dim3(1), dim3(256), 0, st,
                     static_cast<unsigned char*>(host_dst), static_cast<const unsigned char*>(src),
                     (int)bytes);
  XF_HIP_CHECK(hipGetLastError());
}

__global__ void k_snapshot(HostSnap* dst, const u32* mon, unsigned long long seq) {
  store_snapshot(dst, mon, seq);
}

void launch_snapshot(HostSnap* dst, const u32* mon, unsigned long long seq, hipStream_t st) {
  hipLaunchKernelGGL(k_snapshot, dim3(1), dim3(64), 0, st, dst, mon, seq);
  XF_HIP_CHECK(hipGetLastError());
}

void launch_fill_u64(u64* p, u64 v, size_t n, hipStream_t st) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_fill_u64, dim3(grid_for((int64_t)n)), dim3(kBlock), 0, st, p, v, n);
  XF_HIP_CHECK(hipGetLastError());
}

__global__ void k_table_clear(TableView t) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  const int W = t.L.stride;
  for (u64 s = (u64)blockIdx.x * blockDim.x + threadIdx.x; s < t.cap; s += stride) {
    u32* sp = t.words + s * (u64)W;
    sp[0] = 0xFFFFFFFFu;
    sp[1] = 0xFFFFFFFFu;
    for (int w = 2; w < W; ++w) sp[w] = 0u;
  }
}

void launch_table_clear(const TableView& t, hipStream_t st) {
  hipLaunchKernelGGL(k_table_clear, dim3(grid_for((int64_t)t.cap)), dim3(kBlock), 0, st, t);
  XF_HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// checkpoint export / import
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) k_table_export(TableView t, u64* __restrict__ keys_out,
                                                         u32* __restrict__ words_out,
                                                         int64_t max_rows,
                                                         unsigned long long* counter) {
  const int W = t.L.stride - 2;
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 s = (u64)blockIdx.x * blockDim.x + threadIdx.x; s < t.cap; s += stride) {
    const u32* sp = t.words + s * (u64)t.L.stride;
    u64 key = *reinterpret_cast<const u64*>(sp);
    bool live = key != kEmptyKey;
    unsigned long long idx = wave_append(counter, live);
    if (live && (int64_t)idx < max_rows) {
      keys_out[idx] = key;
      for (int w = 0; w < W; ++w) words_out[idx * W + w] = sp[2 + w];
    }
  }
}

void launch_table_export(const TableView& t, u64* keys_out, u32* words_out, int64_t max_rows,
                         unsigned long long* counter, hipStream_t st) {
  XF_HIP_CHECK(hipMemsetAsync(counter, 0, sizeof(unsigned long long), st));
  hipLaunchKernelGGL(k_table_export, dim3(grid_for((int64_t)t.cap)), dim3(kBlock), 0, st, t,
                     keys_out, words_out, max_rows, counter);
  XF_HIP_CHECK(hipGetLastError());
}

__global__ void __launch_bounds__(kBlock) k_table_import(TableView t, const u64* __restrict__ keys,
                                                         const u32* __restrict__ words,
                                                         int64_t n) {
  const int W = t.L.stride - 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  unsigned int claims = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    bool claimed = false;
    u32 slot = probe(t, sanitize_key(keys[i]), true, claimed);
    claims += claimed;
    if (slot == kNoSlot) continue;
    u32* sp = t.words + (u64)slot * t.L.stride;
    for (int w = 0; w < W; ++w) sp[2 + w] = words[i * W + w];
  }
  block_count_add<kBlock>(t.size, claims);
}

// Growth by segment splits (TableView geometry, Backend::table_split).  t is
// the geometry after the split: segments [s0, s0 + k) of t.level split into
// their buddies s + 2^level, which are mapped and cleared.  A key moves when
// bit (seg_log2 + level) of its hash is set.
//
// Phase 1 marks the cluster starts of the source segments (an occupied slot
// whose predecessor in the segment is free) in a bitmap, before any slot
// changes: phase 2 rewrites clusters, and a start test racing with those
// writes could see a half-rewritten cluster.  Phase 2: one lane per cluster
// walks it in order (linear probing's backward-shift deletion, for every
// moving key at once).  At walk position d every slot before d is final:
// a moving key is CAS-inserted into the buddy segment (an empty table that
// only other moving keys compete for) with its state words, and slot d is
// freed; a staying key goes to the first free slot from its home on -- a
// slot freed earlier in the walk, or d itself -- and slot d is freed if it
// left.  Slots before d are never freed again, so every chain from a home to
// its key stays occupied.  Clusters are separated by free slots, so lanes
// never touch each other's slots.
__global__ void __launch_bounds__(kBlock) k_table_split_marks(TableView t, u64 s0, u64 k,
                                                              u64* __restrict__ marks) {
  const int g = t.seg_log2;
  const u64 m = (1ull << g) - 1;
  const u64 n = k << g;
  const int W = t.L.stride;
  const u64 stride = (u64)gridDim.x * blockDim.x;
  // (n is a multiple of 64 when g >= 6; the ballot of a partial wave is padded)
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < ((n + 63) & ~63ull); i += stride) {
    bool start = false;
    if (i < n) {
      const u64 base = (s0 << g) + (i & ~m), c = i & m;
      const u64 kc = *reinterpret_cast<const u64*>(t.words + (base + c) * (u64)W);
      const u64 kp = *reinterpret_cast<const u64*>(t.words + (base + ((c - 1) & m)) * (u64)W);
      start = kc != kEmptyKey && kp == kEmptyKey;
    }
    const unsigned long long b = __ballot(start);
    if ((threadIdx.x & 63) == 0) marks[i >> 6] = b;
  }
}

__global__ void __launch_bounds__(kBlock) k_table_split(TableView t, u64 s0, u64 k,
                                                        const u64* __restrict__ marks) {
  const int g = t.seg_log2;
  const u64 G = 1ull << g, m = G - 1;
  const u64 n = k << g;
  const int W = t.L.stride;
  const u64 move_bit = 1ull << (g + t.level);
  const u64 buddy = (1ull << t.level) << g;  // slot offset of a segment's buddy
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    if (!((marks[i >> 6] >> (i & 63)) & 1ull)) continue;
    const u64 base = (s0 << g) + (i & ~m), c = i & m;
    auto slot_at = [&](u64 off) { return t.words + (base + ((c + off) & m)) * (u64)W; };
    auto free_slot = [&](u32* sp) {
      sp[0] = 0xFFFFFFFFu;
      sp[1] = 0xFFFFFFFFu;
      for (int w = 2; w < W; ++w) sp[w] = 0u;
    };
    for (u64 d = 0; d < G; ++d) {  // d: walk offset from the cluster start c
      u32* sp = slot_at(d);
      const u64 key = *reinterpret_cast<const u64*>(sp);
      if (key == kEmptyKey) break;
      const u64 h = fmix64(key);
      if (h & move_bit) {
        u64 q = base + buddy + (h & m);
        bool placed = false;
        for (u64 r = 0; r < t.probe_limit; ++r) {
          u32* qp = t.words + q * (u64)W;
          const u64 prev = atomicCAS(reinterpret_cast<unsigned long long*>(qp),
                                     (unsigned long long)kEmptyKey, (unsigned long long)key);
          if (prev == kEmptyKey) {
            for (int w = 2; w < W; ++w) qp[w] = sp[w];
            placed = true;
            break;
          }
          q = table_next(t, q);
        }
        if (!placed) *t.overflow = 1u;
        free_slot(sp);
      } else {
        u64 off = ((h & m) - c) & m;  // home, in [0, d]: the chain from it is unbroken
        while (off < d && *reinterpret_cast<const u64*>(slot_at(off)) != kEmptyKey) ++off;
        if (off != d) {
          u32* dp = slot_at(off);
          for (int w = 0; w < W; ++w) dp[w] = sp[w];
          free_slot(sp);
        }
      }
    }
  }
}

void launch_table_split(const TableView& t, u64 s0, u64 k, u64* marks, hipStream_t st) {
  const int64_t n = (int64_t)(k << t.seg_log2);
  if (n <= 0) return;
  hipLaunchKernelGGL(k_table_split_marks, dim3(grid_for(n, kBlock, 16384)), dim3(kBlock), 0, st,
                     t, s0, k, marks);
  XF_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_table_split, dim3(grid_for(n, kBlock, 16384)), dim3(kBlock), 0, st, t, s0,
                     k, (const u64*)marks);
  XF_HIP_CHECK(hipGetLastError());
}

// Pruning (Backend::table_prune): drop the keys of segments [s0, s0 + k) that
// meet slot_prunable.  The split's walk with another "this key leaves" rule
// and no buddy segment: k_table_split_marks marks the cluster starts before
// any slot changes, then one lane per cluster walks it in order.  At walk
// position d every slot before d is final: a leaving key's slot is freed; a
// staying key goes to the first free slot from its home on -- a slot freed
// earlier in the walk, or d itself.  Staying keys only move backwards inside
// their own cluster, so lanes never meet and no insert can overflow.  A
// segment with no free slot has no cluster start and is left alone; that
// cannot happen below load 1 (inserts stop at probe_limit <= segment slots,
// and the engine grows the table long before).
// LR16: LR-FTRL 16-byte slots (key, n, z), each read and written as one
// 16-byte access.
template <bool LR16>
__global__ void __launch_bounds__(kBlock) k_table_prune(TableView t, OptSpec o, float max_n,
                                                        u64 s0, u64 k,
                                                        const u64* __restrict__ marks,
                                                        unsigned long long* dropped) {
  const int g = t.seg_log2;
  const u64 G = 1ull << g, m = G - 1;
  const u64 n = k << g;
  const int W = t.L.stride;
  const u64 stride = (u64)gridDim.x * blockDim.x;
  unsigned int drops = 0;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    if (!((marks[i >> 6] >> (i & 63)) & 1ull)) continue;
    const u64 base = (s0 << g) + (i & ~m), c = i & m;
    auto slot_at = [&](u64 off) { return t.words + (base + ((c + off) & m)) * (u64)W; };
    if constexpr (LR16) {
      const uint4 kFree = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u);
      for (u64 d = 0; d < G; ++d) {
        uint4* sp = reinterpret_cast<uint4*>(slot_at(d));
        const uint4 v = *sp;
        const u64 key = (u64)v.x | ((u64)v.y << 32);
        if (key == kEmptyKey) break;
        const float fn = __uint_as_float(v.z), fz = __uint_as_float(v.w);
        if (param_prunable(ftrl_weight(fz, fn, o.ftrl), fn, kFTRL, max_n)) {
          *sp = kFree;
          ++drops;
        } else {
          u64 off = ((fmix64(key) & m) - c) & m;  // home, in [0, d]
          while (off < d && *reinterpret_cast<const u64*>(slot_at(off)) != kEmptyKey) ++off;
          if (off != d) {
            *reinterpret_cast<uint4*>(slot_at(off)) = v;
            *sp = kFree;
          }
        }
      }
    } else {
      auto free_slot = [&](u32* sp) {
        sp[0] = 0xFFFFFFFFu;
        sp[1] = 0xFFFFFFFFu;
        for (int w = 2; w < W; ++w) sp[w] = 0u;
      };
      for (u64 d = 0; d < G; ++d) {
        u32* sp = slot_at(d);
        const u64 key = *reinterpret_cast<const u64*>(sp);
        if (key == kEmptyKey) break;
        if (slot_prunable(sp, key, t.L, o, max_n)) {
          free_slot(sp);
          ++drops;
        } else {
          u64 off = ((fmix64(key) & m) - c) & m;  // home, in [0, d]
          while (off < d && *reinterpret_cast<const u64*>(slot_at(off)) != kEmptyKey) ++off;
          if (off != d) {
            u32* dp = slot_at(off);
            for (int w = 0; w < W; ++w) dp[w] = sp[w];
            free_slot(sp);
          }
        }
      }
    }
  }
  block_count_add<kBlock>(dropped, drops);
}

// *size -= *count, *total += *count (the prune's launches counted into *count)
__global__ void k_table_prune_finish(unsigned long long* size, unsigned long long* total,
                                     const unsigned long long* count) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const unsigned long long c = *count;
    *size -= c;
    *total += c;
  }
}

void launch_table_prune(const TableView& t, const OptSpec& o, float max_n, u64 s0, u64 k,
                        u64* marks, unsigned long long* count, hipStream_t st) {
  const int64_t n = (int64_t)(k << t.seg_log2);
  if (n <= 0) return;
  hipLaunchKernelGGL(k_table_split_marks, dim3(grid_for(n, kBlock, 16384)), dim3(kBlock), 0, st,
                     t, s0, k, marks);
  XF_HIP_CHECK(hipGetLastError());
  if (t.L.lr16())
    hipLaunchKernelGGL(k_table_prune<true>, dim3(grid_for(n, kBlock, 16384)), dim3(kBlock), 0, st,
                       t, o, max_n, s0, k, (const u64*)marks, count);
  else
    hipLaunchKernelGGL(k_table_prune<false>, dim3(grid_for(n, kBlock, 16384)), dim3(kBlock), 0,
                       st, t, o, max_n, s0, k, (const u64*)marks, count);
  XF_HIP_CHECK(hipGetLastError());
}

void launch_table_prune_finish(unsigned long long* size, unsigned long long* total,
                               const unsigned long long* count, hipStream_t st) {
  hipLaunchKernelGGL(k_table_prune_finish, dim3(1), dim3(64), 0, st, size, total, count);
  XF_HIP_CHECK(hipGetLastError());
}

__global__ void __launch_bounds__(kBlock) k_table_prefill(TableView t, int64_t n, u64 seed) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  unsigned int claims = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const u64 key = prefill_key(seed, (u64)i);
    bool claimed = false;
    const u32 slot = probe(t, key, true, claimed);
    claims += claimed;
    if (slot != kNoSlot && t.L.has_flag) t.words[(u64)slot * t.L.stride + t.L.flag_word] = 1u;
  }
  block_count_add<kBlock>(t.size, claims);
}

void launch_table_prefill(const TableView& t, int64_t n, u64 seed, hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_table_prefill, dim3(grid_for(n, kBlock, 16384)), dim3(kBlock), 0, st, t, n,
                     seed);
  XF_HIP_CHECK(hipGetLastError());
}

void launch_table_import(const TableView& t, const u64* keys, const u32* words, int64_t n,
                         hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_table_import, dim3(grid_for(n)), dim3(kBlock), 0, st, t, keys, words, n);
  XF_HIP_CHECK(hipGetLastError());
}

// L1 sparsity report: count (key, param) weights that are exactly non-zero.
// A full-table sweep (dwordx4-friendly for 16-B LR slots), one atomic per
// workgroup.
__global__ void __launch_bounds__(kBlock) k_table_nonzero(TableView t, OptSpec o,
                                                          unsigned long long* counter) {
  const TableLayout& L = t.L;
  const u64 stride = (u64)gridDim.x * blockDim.x;
  unsigned int cnt = 0;
  for (u64 s = (u64)blockIdx.x * blockDim.x + threadIdx.x; s < t.cap; s += stride) {
    const u32* sp = t.words + s * (u64)L.stride;
    const u64 key = *reinterpret_cast<const u64*>(sp);
    if (key == kEmptyKey) continue;
    for (int p = 0; p < L.P; ++p) cnt += slot_weight(sp, key, p, L, o) != 0.0f;
  }
  block_count_add<kBlock>(counter, cnt);
}

void launch_table_nonzero(const TableView& t, const OptSpec& o, unsigned long long* counter,
                          hipStream_t st) {
  XF_HIP_CHECK(hipMemsetAsync(counter, 0, sizeof(unsigned long long), st));
  hipLaunchKernelGGL(k_table_nonzero, dim3(grid_for((int64_t)t.cap)), dim3(kBlock), 0, st, t, o,
                     counter);
  XF_HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// delta checkpoints (EngineConfig::delta_track, docs/DESIGN.md §2): the
// touched-key filter, one bit per key at delta_bit(key, L) of 2^L bits
// ---------------------------------------------------------------------------
// Shaped like k_admit_count: each lane owns kDeltaItems entries one block
// apart and issues their key loads, then their filter-word loads, before it
// resolves any.  The word is read first and the atomicOr issued only when the
// bit is clear: bits only ever go from 0 to 1 between two clears, so a stale
// read can only cost a redundant OR, and after an epoch's first steps the hot
// head of the key distribution is marked and the kernel mostly reads.  A pure
// OR: the filter depends on the set of keys alone, never on lane order.
constexpr int kDeltaItems = 4;
constexpr int kDeltaChunk = kBlock * kDeltaItems;

__global__ void __launch_bounds__(kBlock) k_delta_mark(u32* __restrict__ bits, int L,
                                                       const u64* __restrict__ keys,
                                                       const int64_t* n_dev, int64_t n_host,
                                                       int64_t n_max) {
  const int64_t n = dev_count(n_dev, n_host, n_max);
  if ((int64_t)blockIdx.x * kDeltaChunk >= n) return;  // (grid sized by capacity)
  const int64_t base = (int64_t)blockIdx.x * kDeltaChunk + threadIdx.x;
  bool on[kDeltaItems];
  u64 bit[kDeltaItems];
  u32 w[kDeltaItems];
#pragma unroll
  for (int j = 0; j < kDeltaItems; ++j) {
    const int64_t i = base + (int64_t)j * kBlock;
    on[j] = i < n;
    bit[j] = delta_bit(on[j] ? sanitize_key(keys[i]) : 0ull, L);
  }
#pragma unroll
  for (int j = 0; j < kDeltaItems; ++j) {
    if (!on[j]) continue;
    XF_DASSERT((bit[j] >> 5) < (1ull << (L - 5)));
    w[j] = bits[bit[j] >> 5];
  }
#pragma unroll
  for (int j = 0; j < kDeltaItems; ++j) {
    if (!on[j]) continue;
    const u32 m = 1u << (u32)(bit[j] & 31u);
    if (!(w[j] & m)) atomicOr(bits + (bit[j] >> 5), m);
  }
}

void launch_delta_mark(u32* bits, int L, const u64* keys, const int64_t* n_dev, int64_t n_host,
                       int64_t n_max, hipStream_t st) {
  if (L < kDeltaMinLog2 || L > kDeltaMaxLog2) throw std::runtime_error("delta_mark: log2");
  const int64_t nm = n_dev ? n_max : n_host;
  if (nm <= 0) return;
  const int64_t g = (nm + kDeltaChunk - 1) / kDeltaChunk;
  hipLaunchKernelGGL(k_delta_mark, dim3((unsigned)g), dim3(kBlock), 0, st, bits, L, keys, n_dev,
                     n_host, n_dev ? n_max : n_host);
  XF_HIP_CHECK(hipGetLastError());
}

// k_table_export with one more predicate: the key's filter bit is set.
// max_rows = 0 only counts (the outputs are not touched).
__global__ void __launch_bounds__(kBlock) k_table_export_marked(
    TableView t, const u32* __restrict__ bits, int L, u64* __restrict__ keys_out,
    u32* __restrict__ words_out, int64_t max_rows, unsigned long long* counter) {
  const int W = t.L.stride - 2;
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 s = (u64)blockIdx.x * blockDim.x + threadIdx.x; s < t.cap; s += stride) {
    const u32* sp = t.words + s * (u64)t.L.stride;
    const u64 key = *reinterpret_cast<const u64*>(sp);
    bool live = key != kEmptyKey;
    if (live) {
      const u64 b = delta_bit(key, L);
      live = (bits[b >> 5] >> (u32)(b & 31u)) & 1u;
    }
    unsigned long long idx = wave_append(counter, live);
    if (live && (int64_t)idx < max_rows) {
      keys_out[idx] = key;
      for (int w = 0; w < W; ++w) words_out[idx * W + w] = sp[2 + w];
    }
  }
}

void launch_table_export_marked(const TableView& t, const u32* bits, int L, u64* keys_out,
                                u32* words_out, int64_t max_rows, unsigned long long* counter,
                                hipStream_t st) {
  if (L < kDeltaMinLog2 || L > kDeltaMaxLog2) throw std::runtime_error("table_export_marked: log2");
  XF_HIP_CHECK(hipMemsetAsync(counter, 0, sizeof(unsigned long long), st));
  hipLaunchKernelGGL(k_table_export_marked, dim3(grid_for((int64_t)t.cap)), dim3(kBlock), 0, st,
                     t, bits, L, keys_out, words_out, max_rows, counter);
  XF_HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// serving snapshots (docs/DESIGN.md §2): the keys that meet slot_exported
// (types.h) with their P resolved weights.  Shaped like k_table_export_marked;
// max_rows = 0 only counts (the outputs are not touched).
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) k_table_export_weights(
    TableView t, OptSpec o, u64* __restrict__ keys_out, float* __restrict__ weights_out,
    int64_t max_rows, unsigned long long* counter) {
  const TableLayout& L = t.L;
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 s = (u64)blockIdx.x * blockDim.x + threadIdx.x; s < t.cap; s += stride) {
    const u32* sp = t.words + s * (u64)L.stride;
    const u64 key = *reinterpret_cast<const u64*>(sp);
    const bool live = key != kEmptyKey && slot_exported(sp, key, L, o);
    const unsigned long long idx = wave_append(counter, live);
    if (live && (int64_t)idx < max_rows) {
      keys_out[idx] = key;
      for (int p = 0; p < L.P; ++p) weights_out[idx * L.P + p] = slot_weight(sp, key, p, L, o);
    }
  }
}

void launch_table_export_weights(const TableView& t, const OptSpec& o, u64* keys_out,
                                 float* weights_out, int64_t max_rows,
                                 unsigned long long* counter, hipStream_t st) {
  XF_HIP_CHECK(hipMemsetAsync(counter, 0, sizeof(unsigned long long), st));
  hipLaunchKernelGGL(k_table_export_weights, dim3(grid_for((int64_t)t.cap)), dim3(kBlock), 0, st,
                     t, o, keys_out, weights_out, max_rows, counter);
  XF_HIP_CHECK(hipGetLastError());
}

// Serving deltas (docs/DESIGN.md §2): k_table_export_marked's walk and
// compaction, k_table_export_weights' output.  The predicate is the filter bit
// alone, not slot_exported: a marked key whose weights read as an absent key's
// is the delta's way to say "this key left".  max_rows = 0 only counts.
__global__ void __launch_bounds__(kBlock) k_table_export_weights_marked(
    TableView t, OptSpec o, const u32* __restrict__ bits, int Lb, u64* __restrict__ keys_out,
    float* __restrict__ weights_out, int64_t max_rows, unsigned long long* counter) {
  const TableLayout& L = t.L;
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 s = (u64)blockIdx.x * blockDim.x + threadIdx.x; s < t.cap; s += stride) {
    const u32* sp = t.words + s * (u64)L.stride;
    const u64 key = *reinterpret_cast<const u64*>(sp);
    bool live = key != kEmptyKey;
    if (live) {
      const u64 b = delta_bit(key, Lb);
      live = (bits[b >> 5] >> (u32)(b & 31u)) & 1u;
    }
    const unsigned long long idx = wave_append(counter, live);
    if (live && (int64_t)idx < max_rows) {
      keys_out[idx] = key;
      for (int p = 0; p < L.P; ++p) weights_out[idx * L.P + p] = slot_weight(sp, key, p, L, o);
    }
  }
}

void launch_table_export_weights_marked(const TableView& t, const OptSpec& o, const u32* bits,
                                        int L, u64* keys_out, float* weights_out,
                                        int64_t max_rows, unsigned long long* counter,
                                        hipStream_t st) {
  if (L < kDeltaMinLog2 || L > kDeltaMaxLog2)
    throw std::runtime_error("table_export_weights_marked: log2");
  XF_HIP_CHECK(hipMemsetAsync(counter, 0, sizeof(unsigned long long), st));
  hipLaunchKernelGGL(k_table_export_weights_marked, dim3(grid_for((int64_t)t.cap)), dim3(kBlock),
                     0, st, t, o, bits, L, keys_out, weights_out, max_rows, counter);
  XF_HIP_CHECK(hipGetLastError());
}

// set bits of the filter's 2^(L - 5) words, one atomic per workgroup
__global__ void __launch_bounds__(kBlock) k_delta_popcount(const u32* __restrict__ bits,
                                                           u64 words,
                                                           unsigned long long* counter) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  unsigned int cnt = 0;  // (<= 2^29 words over 2048 x 256 lanes: 2^15 bits a lane)
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += stride)
    cnt += __popc(bits[i]);
  block_count_add<kBlock>(counter, cnt);
}

void launch_delta_popcount(const u32* bits, int L, unsigned long long* counter, hipStream_t st) {
  if (L < kDeltaMinLog2 || L > kDeltaMaxLog2) throw std::runtime_error("delta_popcount: log2");
  const u64 words = 1ull << (L - 5);
  XF_HIP_CHECK(hipMemsetAsync(counter, 0, sizeof(unsigned long long), st));
  hipLaunchKernelGGL(k_delta_popcount, dim3(grid_for((int64_t)words)), dim3(kBlock), 0, st, bits,
                     words, counter);
  XF_HIP_CHECK(hipGetLastError());
}

}  // namespace hip
}  // namespace xflow
