// xflow-amd: device code shared by the parameter-store kernels (kernels_dedup /
// kernels_pull / kernels_apply / kernels_exchange / kernels_table .hip): only
// what two or more of them need.  Included by .hip files only; as in
// model_common.h, every __device__ function a kernel calls is defined here or
// in the kernel's own file.
#pragma once
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "kernels.h"
#include "hip_util.h"

namespace xflow {
namespace hip {

// grid cap of the lane-group pull/apply kernels (8 K workgroups of 256: four
// resident rounds; their grid-stride loops pipeline the random row accesses,
// see RowPipe -- 16 K measured 2 % slower on FM-8, 64 K 6 %)
constexpr int kGroupGridCap = 8192;

// workgroup of the one-workgroup scans (k_compact_scan, k_scan_top, k_scan_one)
constexpr int kScanBlock = 1024;

// ---------------------------------------------------------------------------
// persistent table probe
// ---------------------------------------------------------------------------
__device__ __forceinline__ u32 probe(const TableView& t, u64 key, bool insert, bool& claimed) {
  u64 s = table_home(t, fmix64(key));
  const int stride = t.L.stride;
  for (u64 n = 0; n < t.probe_limit; ++n) {
    u64* kp = reinterpret_cast<u64*>(t.words + s * (u64)stride);
    u64 cur = *kp;
    if (cur == key) return (u32)s;
    if (cur == kEmptyKey) {
      if (!insert) return kNoSlot;
      u64 prev = atomicCAS((unsigned long long*)kp, (unsigned long long)kEmptyKey,
                           (unsigned long long)key);
      if (prev == kEmptyKey) { claimed = true; return (u32)s; }
      if (prev == key) return (u32)s;
    }
    s = table_next(t, s);
  }
  // bounded chain (TableView::probe_limit): a key is never stored further out
  if (insert) *t.overflow = 1u;
  return kNoSlot;
}

// Packed lane groups for the multi-parameter pull/apply: P lanes per key
// (lane p owns parameter p), floor(64/P) keys per wave, never straddling a
// wave.  In pow2 groups of 16 lanes these kernels were VALU-issue bound (FTRL
// closed form with IEEE division/sqrt, lazy N(0,1) init; PMC of the FM-8
// apply: 1626 VALU instructions per wave for 16 keys, 50 % of wave cycles
// waiting): packing 7 FM-8 keys (P = 9) into a wave is 1.75x fewer
// instructions per key.  Packed, they are bound by the dependent random row
// accesses instead (an apply fed the pull's weights, skipping the closed
// form, was slower), which RowPipe overlaps with the previous key's math.
struct PackedLane {
  int P, K, g, p;        // lanes per key, keys per wave, key in wave, param
  bool on;               // lane belongs to a key group (64 % P lanes idle)
  int64_t first, stride;  // key index of this lane's group, grid stride in keys
};

__device__ __forceinline__ PackedLane packed_lane(int P) {
  PackedLane r;
  r.P = P;
  r.K = kWave / P;
  const int lane = threadIdx.x % kWave;
  r.g = lane / P;
  r.p = lane - r.g * P;
  r.on = r.g < r.K;
  const int64_t waves = (int64_t)(blockDim.x / kWave);
  r.first = ((int64_t)blockIdx.x * waves + threadIdx.x / kWave) * r.K + r.g;
  r.stride = (int64_t)gridDim.x * waves * r.K;
  return r;
}

// One key's slot words a lane of its packed group needs (key, pushed flag,
// the lane's param state), loaded one grid-stride iteration ahead of use by
// the multi-parameter pull/apply: with the slot index loaded two ahead, the
// random row access of iteration t+1 is in flight while iteration t computes.
struct RowPre {
  u64 key = 0;
  u32 flag = 1;
  float s0 = 0.0f, s1 = 0.0f;  // FTRL (n, z); SGD w
};

__device__ __forceinline__ RowPre row_pre(const u32* __restrict__ words, u32 slot, int p,
                                          const TableLayout& L) {
  RowPre r;
  if (slot == kNoSlot) return r;
  const u32* sp = words + (u64)slot * L.stride;
  r.key = *reinterpret_cast<const u64*>(sp);
  if (L.has_flag) r.flag = sp[L.flag_word];
  if (L.opt == kFTRL) {
    const float2 nz = *reinterpret_cast<const float2*>(sp + 2 + 2 * p);
    r.s0 = nz.x;
    r.s1 = nz.y;
  } else {
    r.s0 = __uint_as_float(sp[2 + p]);
  }
  return r;
}

// The same words from the pull's stash (PullArgs::out_nz, FTRL): entry i's
// (n, z) of param p at [i * P + p], n < 0 marking a key never pushed; the
// key from the unique list.  Coalesced, unlike the slot's row.
__device__ __forceinline__ RowPre row_stash(const float2* __restrict__ stash,
                                            const u64* __restrict__ keys, int64_t i, int p,
                                            int P) {
  RowPre r;
  const float2 nz = stash[(size_t)i * P + p];
  r.key = keys[i];
  r.flag = nz.x >= 0.0f ? 1u : 0u;
  r.s0 = nz.x >= 0.0f ? nz.x : 0.0f;
  r.s1 = nz.y;
  return r;
}

// Grid-stride pipeline over a packed group's keys: slots two iterations
// ahead, row words one ahead (RowPre) -- from the slot's row, or from the
// pull's stash when the caller sets `stash` (and `keys`).
struct RowPipe {
  int64_t stride, n;
  u32 s_cur, s_nx;
  RowPre r_nx;
  const float2* stash = nullptr;
  const u64* keys = nullptr;
  __device__ __forceinline__ RowPre row(const u32* words, u32 slot, int64_t i, int p,
                                        const TableLayout& L) const {
    return stash ? row_stash(stash, keys, i, p, L.P) : row_pre(words, slot, p, L);
  }
  __device__ __forceinline__ void start(const u32* __restrict__ slots, const u32* words,
                                        int64_t i, int p, const TableLayout& L) {
    s_cur = i < n ? slots[i] : kNoSlot;
    s_nx = i + stride < n ? slots[i + stride] : kNoSlot;
    if (i < n) r_nx = row(words, s_cur, i, p, L);
  }
  // at the top of iteration i: returns (slot, row) of i, issues i + stride's
  // row loads and i + 2 * stride's slot load
  __device__ __forceinline__ u32 next(const u32* __restrict__ slots, const u32* words, int64_t i,
                                      int p, const TableLayout& L, RowPre& r) {
    const u32 slot = s_cur;
    r = r_nx;
    s_cur = s_nx;
    if (i + stride < n) r_nx = row(words, s_cur, i + stride, p, L);
    if (i + 2 * stride < n) s_nx = slots[i + 2 * stride];
    return slot;
  }
};

// grid for packed groups: one key per group up to the cap
static int packed_grid(int64_t n, int P) {
  const int64_t keys_per_block = (int64_t)(kBlock / kWave) * (kWave / P);
  const int64_t g = (n + keys_per_block - 1) / keys_per_block;
  return (int)(g < 1 ? 1 : (g < kGroupGridCap ? g : kGroupGridCap));
}

// The reference divides a float sum by the row count in double and rounds to
// float (lr_worker.cc:116-118).  For a float x and an integer n < 2^24 (exact
// in float) that equals the correctly rounded float quotient x / n: double
// rounding is innocuous for division when the wide format has >= 2p+2 bits
// (53 >= 2*24+2), so the f64 division sequence is replaced by the f32 one.
__device__ __forceinline__ float norm_grad(float raw, const int32_t* slice_rows, int s) {
  if (!slice_rows) return raw;
  const int32_t r = slice_rows[s];
  return r < (1 << 24) ? raw / (float)r : (float)((double)raw / (double)r);
}

}  // namespace hip
}  // namespace xflow
