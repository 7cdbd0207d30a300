// xflow-amd: refreshing a live frozen table from a serving delta (gfx950;
// docs/DESIGN.md §2 "Serving deltas", Backend::frozen_upsert / frozen_sweep).
//
// A serving delta lists (key, P resolved weights) for every touched key of the
// training table -- the keys whose weights went back to what an absent key
// reads included: those are the deletions, and no flag marks them.  Applying
// it to a frozen table is two launches on the engine's stream:
//
//   k_frozen_upsert  one lane per entry: probe with insert, write the weights,
//                    and flag the slot's segment in dirty[] when the weights
//                    written are exactly the absent ones
//   k_frozen_sweep   over the flagged segments only: k_table_prune's cluster
//                    walk (kernels_table.hip) with the rule "this key leaves"
//                    = !slot_exported -- the slot cannot be told from absence
//                    by any pull -- and backward-shift re-packing of the keys
//                    that stay; no tombstones
//
// Both are bound by their random 16-64 B slot accesses, like the rest of the
// store's kernels (kernels_table.hip): one atomic per workgroup for the
// counts, several independent loads in flight per lane.
#include "table_common.h"

namespace xflow {
namespace hip {

namespace {

// a frozen LR table: 16-byte slots {key, w, pad}, the absent weight +0.0
__host__ __device__ inline bool frozen_lr16(const TableLayout& L) {
  return L.opt == kFrozen && L.P == 1 && L.stride == 4;
}

// the entries a lane of k_frozen_upsert<true> owns, one block apart (as
// k_delta_mark's kDeltaItems)
constexpr int kUpsertItems = 4;
constexpr int kUpsertChunk = kBlock * kUpsertItems;

}  // namespace

// Keys are unique within a launch (after sanitize_key), so a slot has one
// writer.  dirty[s] = 1 is a plain store: any writer wins.
// LR16: each lane issues the key, weight and home-slot loads of its
// kUpsertItems entries before it resolves any of them; a slot is written as
// one 16-byte store.
template <bool LR16>
__global__ void __launch_bounds__(kBlock) k_frozen_upsert(TableView t, OptSpec o,
                                                          const u64* __restrict__ keys,
                                                          const u32* __restrict__ wbits,
                                                          int64_t n, u32* __restrict__ dirty) {
  const int g = t.seg_log2;
  unsigned int claims = 0;
  if constexpr (LR16) {
    const int64_t base = (int64_t)blockIdx.x * kUpsertChunk + threadIdx.x;
    bool on[kUpsertItems];
    u64 key[kUpsertItems], home[kUpsertItems], cur[kUpsertItems];
    u32 w[kUpsertItems];
#pragma unroll
    for (int j = 0; j < kUpsertItems; ++j) {
      const int64_t i = base + (int64_t)j * kBlock;
      on[j] = i < n;
      key[j] = sanitize_key(on[j] ? keys[i] : 0ull);
      w[j] = on[j] ? wbits[i] : 0u;
    }
#pragma unroll
    for (int j = 0; j < kUpsertItems; ++j) {
      home[j] = table_home(t, fmix64(key[j]));
      XF_DASSERT(home[j] < t.cap);
      cur[j] = on[j] ? *reinterpret_cast<const u64*>(t.words + home[j] * 4ull) : 0ull;
    }
#pragma unroll
    for (int j = 0; j < kUpsertItems; ++j) {
      if (!on[j]) continue;
      u32 slot = (u32)home[j];
      if (cur[j] != key[j]) {  // (not at its home: the chain walk, claiming when absent)
        bool claimed = false;
        slot = probe(t, key[j], true, claimed);
        claims += claimed;
        if (slot == kNoSlot) continue;
      }
      XF_DASSERT((u64)slot < t.cap);
      *reinterpret_cast<uint4*>(t.words + (u64)slot * 4ull) =
          make_uint4((u32)key[j], (u32)(key[j] >> 32), w[j], 0u);
      if (w[j] == 0u) dirty[slot >> g] = 1u;
    }
  } else {
    const TableLayout& L = t.L;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
      const u64 key = sanitize_key(keys[i]);
      bool claimed = false;
      const u32 slot = probe(t, key, true, claimed);
      claims += claimed;
      if (slot == kNoSlot) continue;
      XF_DASSERT((u64)slot < t.cap);
      u32* sp = t.words + (u64)slot * L.stride;
      bool absent = true;
      for (int p = 0; p < L.P; ++p) {
        const u32 b = wbits[i * L.P + p];
        sp[2 + p] = b;
        absent = absent && b == weight_bits(absent_weight(key, p, L, o));
      }
      if (absent) dirty[slot >> g] = 1u;
    }
  }
  block_count_add<kBlock>(t.size, claims);
}

void launch_frozen_upsert(const TableView& t, const OptSpec& o, const u64* keys,
                          const float* weights, int64_t n, u32* dirty, hipStream_t st) {
  if (t.L.opt != kFrozen || t.L.has_flag || t.L.sp != 1)
    throw std::runtime_error("frozen_upsert: needs a frozen table");
  if (n <= 0) return;
  const u32* wbits = reinterpret_cast<const u32*>(weights);
  if (frozen_lr16(t.L)) {
    const int64_t g = (n + kUpsertChunk - 1) / kUpsertChunk;
    if (g > 0x7fffffffll) throw std::runtime_error("frozen_upsert: too many entries");
    hipLaunchKernelGGL(k_frozen_upsert<true>, dim3((unsigned)g), dim3(kBlock), 0, st, t, o, keys,
                       wbits, n, dirty);
  } else {
    hipLaunchKernelGGL(k_frozen_upsert<false>, dim3(grid_for(n)), dim3(kBlock), 0, st, t, o, keys,
                       wbits, n, dirty);
  }
  XF_HIP_CHECK(hipGetLastError());
}

// k_table_split_marks over the flagged segments of [s0, s0 + k): the cluster
// starts (an occupied slot whose predecessor in the segment is free) as a
// bitmap, before any slot changes.  A segment whose dirty flag is unset gets
// zero marks and none of its slots is read.  The flagged segments are counted
// into *swept.
__global__ void __launch_bounds__(kBlock) k_frozen_sweep_marks(TableView t, u64 s0, u64 k,
                                                               const u32* __restrict__ dirty,
                                                               u64* __restrict__ marks,
                                                               unsigned long long* swept) {
  const int g = t.seg_log2;
  const u64 m = (1ull << g) - 1;
  const u64 n = k << g;
  const int W = t.L.stride;
  const u64 stride = (u64)gridDim.x * blockDim.x;
  unsigned int segs = 0;
  // (n is a multiple of 64 when g >= 6; the ballot of a partial wave is padded)
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < ((n + 63) & ~63ull); i += stride) {
    bool start = false;
    if (i < n && dirty[s0 + (i >> g)]) {
      const u64 base = (s0 << g) + (i & ~m), c = i & m;
      segs += c == 0;
      const u64 kc = *reinterpret_cast<const u64*>(t.words + (base + c) * (u64)W);
      const u64 kp = *reinterpret_cast<const u64*>(t.words + (base + ((c - 1) & m)) * (u64)W);
      start = kc != kEmptyKey && kp == kEmptyKey;
    }
    const unsigned long long b = __ballot(start);
    if ((threadIdx.x & 63) == 0) marks[i >> 6] = b;
  }
  block_count_add<kBlock>(swept, segs);
}

// k_table_prune's walk with the rule !slot_exported: one lane per marked
// cluster start walks the cluster in order; at walk position d every slot
// before d is final.  A slot that reads as absent is freed; a staying key goes
// to the first free slot from its home on -- a slot freed earlier in the walk,
// or d itself.  Staying keys only move backwards inside their own cluster, so
// lanes never meet.  LR16: frozen LR's 16-byte slots, one access each.
template <bool LR16>
__global__ void __launch_bounds__(kBlock) k_frozen_sweep(TableView t, OptSpec o, u64 s0, u64 k,
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
        if (v.z == 0u) {  // (+0.0: what an absent LR key reads)
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
        if (!slot_exported(sp, key, t.L, o)) {
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

void launch_frozen_sweep(const TableView& t, const OptSpec& o, u64 s0, u64 k, const u32* dirty,
                         u64* marks, unsigned long long* dropped, unsigned long long* swept,
                         hipStream_t st) {
  if (t.L.opt != kFrozen || t.L.has_flag || t.L.sp != 1)
    throw std::runtime_error("frozen_sweep: needs a frozen table");
  const int64_t n = (int64_t)(k << t.seg_log2);
  if (n <= 0) return;
  hipLaunchKernelGGL(k_frozen_sweep_marks, dim3(grid_for(n, kBlock, 16384)), dim3(kBlock), 0, st,
                     t, s0, k, dirty, marks, swept);
  XF_HIP_CHECK(hipGetLastError());
  if (frozen_lr16(t.L))
    hipLaunchKernelGGL(k_frozen_sweep<true>, dim3(grid_for(n, kBlock, 16384)), dim3(kBlock), 0, st,
                       t, o, s0, k, (const u64*)marks, dropped);
  else
    hipLaunchKernelGGL(k_frozen_sweep<false>, dim3(grid_for(n, kBlock, 16384)), dim3(kBlock), 0,
                       st, t, o, s0, k, (const u64*)marks, dropped);
  XF_HIP_CHECK(hipGetLastError());
}

}  // namespace hip
}  // namespace xflow
