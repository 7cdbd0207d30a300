// xflow-amd: the frozen-table probes shared by the one-launch scoring kernels
// (kernels_serve.hip: a lane per row; kernels_rank.hip: a context per tile of
// candidate rows).  Included by .hip files only.
#pragma once
#include "model_common.h"

namespace xflow {
namespace hip {

// Occurrences a lane keeps in flight: their key loads are issued together,
// then their home-slot loads (one dwordx4 each), before any is resolved --
// as in k_pull_lr16, memory-level parallelism is what matters.  A chain that
// continues past the home slot (rare at the snapshot's load <= 0.5) is
// walked slot by slot.
constexpr int kServeItems = 8;
// one wave per workgroup: a lane's work is a chain of dependent round trips,
// so small batches should spread over as many CUs as they have waves
constexpr int kServeBlock = kWave;

// LR, 16-byte slots {key, w, pad}: adds the weights of the occurrences of rs
// in `keys` to wx in occurrence order; an absent key adds 0.0f.
__device__ __forceinline__ void serve_lr_sum(const TableView& t, const u64* keys,
                                             const RowSpan& rs, float& wx) {
  const uint4* slots = reinterpret_cast<const uint4*>(t.words);
  for (int j0 = 0; j0 < rs.len; j0 += kServeItems) {
    u64 key[kServeItems], s[kServeItems];
    uint4 v[kServeItems];
#pragma unroll
    for (int q = 0; q < kServeItems; ++q) {
      const bool on = j0 + q < rs.len;
      key[q] = on ? sanitize_key(keys[rs.at(j0 + q)]) : 0ull;
      s[q] = table_home(t, fmix64(key[q]));
    }
#pragma unroll
    for (int q = 0; q < kServeItems; ++q)
      if (j0 + q < rs.len) v[q] = slots[s[q]];
#pragma unroll
    for (int q = 0; q < kServeItems; ++q) {
      if (j0 + q >= rs.len) continue;
      float w = 0.0f;  // an absent key adds 0.0f
      uint4 cur = v[q];
      u64 sq = s[q];
      // slots at distance >= probe_limit are never examined (bounded chains)
      for (u64 c = 0; c < t.probe_limit; ++c) {
        const u64 k = (u64)cur.x | ((u64)cur.y << 32);
        if (k == key[q]) {
          w = __uint_as_float(cur.z);
          break;
        }
        if (k == kEmptyKey) break;
        sq = table_next(t, sq);
        cur = slots[sq];
      }
      wx += w;
    }
  }
}

// FM and MVM slots of 2 + P words {key, w_0 .. w_{P-1}, pad}:
// words of the widest slot that holds nw weights, and the occurrences in
// flight per lane: the resolved slots stay in registers (N * SW words)
constexpr int serve_sw(int nw) { return (2 + nw + 3) & ~3; }
constexpr int serve_items(int nw) { return serve_sw(nw) <= 16 ? 8 : 4; }

template <int NW>  // weights per key at the kernel width (FM 1 + D, MVM D)
struct ServeProbe {
  static constexpr int SW = serve_sw(NW), Q = SW / 4, N = serve_items(NW);
  u64 key[N];
  uint4 w4[N][Q];  // the key's slot, or what was loaded on the way (absent)
  u32 hit = 0;     // bit q: key[q] is in the table

  // occurrences j0 .. j0 + C - 1 of the row (those past its end: off) into
  // items 0 .. C - 1; C = 1: one probe (MVM's untuned product orders)
  template <int C = N>
  __device__ __forceinline__ void load(const TableView& t, const BatchView& b, const RowSpan& rs,
                                       int j0) {
    const uint4* slots = reinterpret_cast<const uint4*>(t.words);
    const u64 q4 = (u64)(t.L.stride / 4);
    u64 s[C];
#pragma unroll
    for (int q = 0; q < C; ++q) {
      const bool on = j0 + q < rs.len;
      key[q] = on ? sanitize_key(b.keys[rs.at(j0 + q)]) : 0ull;
      s[q] = table_home(t, fmix64(key[q]));
    }
#pragma unroll
    for (int q = 0; q < C; ++q) {
      w4[q][0] = make_uint4(0u, 0u, 0u, 0u);
      if (j0 + q < rs.len) w4[q][0] = slots[s[q] * q4];
    }
    hit = 0u;
#pragma unroll
    for (int q = 0; q < C; ++q) {
      if (!(j0 + q < rs.len)) continue;
      uint4 cur = w4[q][0];
      u64 sq = s[q];
      // slots at distance >= probe_limit are never examined (bounded chains)
      for (u64 c = 0; c < t.probe_limit; ++c) {
        const u64 k = (u64)cur.x | ((u64)cur.y << 32);
        if (k == key[q]) {
          hit |= 1u << q;
          w4[q][0] = cur;
          s[q] = sq;
          break;
        }
        if (k == kEmptyKey) break;
        sq = table_next(t, sq);
        cur = slots[sq * q4];
      }
    }
#pragma unroll
    for (int q = 0; q < C; ++q)
#pragma unroll
      for (int i = 1; i < Q; ++i) {
        w4[q][i] = make_uint4(0u, 0u, 0u, 0u);
        if (((hit >> q) & 1u) && (u64)i < q4) w4[q][i] = slots[s[q] * q4 + (u64)i];
      }
  }

  // the NW weights of item q (the same q in every lane): the slot's P, or an
  // absent key's, then the padding
  __device__ __forceinline__ void weights(int q, const TableLayout& L, const OptSpec& o,
                                          float (&w)[NW]) const {
    u64 k = 0ull;
    bool found = false;
    u32 sw[SW];
#pragma unroll
    for (int i = 0; i < SW; ++i) sw[i] = 0u;
#pragma unroll
    for (int i = 0; i < N; ++i)
      if (q == i) {
        k = key[i];
        found = ((hit >> i) & 1u) != 0u;
#pragma unroll
        for (int j = 0; j < Q; ++j) {
          sw[4 * j] = w4[i][j].x;
          sw[4 * j + 1] = w4[i][j].y;
          sw[4 * j + 2] = w4[i][j].z;
          sw[4 * j + 3] = w4[i][j].w;
        }
      }
#pragma unroll
    for (int i = 0; i < NW; ++i) w[i] = (found && i < L.P) ? __uint_as_float(sw[2 + i]) : 0.0f;
    if (!found) {
      // (one copy of the lazy init's code: a loop over the real params)
#pragma unroll 1
      for (int p = 0; p < L.P; ++p) {
        const float v = absent_weight(k, p, L, o);
#pragma unroll
        for (int i = 0; i < NW; ++i)
          if (i == p) w[i] = v;
      }
    }
  }
};

}  // namespace hip
}  // namespace xflow
