// xflow-amd: pull of the HBM-resident sparse parameter store (gfx950).
// Replaces the Pull of the ps-lite KVServer + unordered_map store of the
// reference (ftrl.h:38-152, server.h:20-35):
//
//   table_pull   probe/insert of unique keys into the persistent table and
//                evaluation of the reference pull value (FTRL weight closed form
//                from (n,z), lazy N(0,1)*1e-2 latent init).
//
// and feature admission: an inserting pull that claims a slot only for a key
// seen often enough (AdmitView, backend.h).
#include "table_common.h"

namespace xflow {
namespace hip {

// LR-FTRL fast path: 16-byte slots {key, n, z}; one dwordx4 load yields the
// key and the optimizer state together.  Each lane owns kPullItems keys spaced
// one block apart and issues all first-probe loads before resolving any (the
// table is tens of GB: every probe is an HBM miss, so memory-level parallelism
// is what matters).
//
// Line-at-a-time probing: the first round loads only the key's home slot (at
// low load it answers almost every probe); a chain that continues loads the
// REST of the aligned 64-byte line (up to 3 slots, independent dwordx4
// loads) in one round trip and resolves those probe positions from
// registers, then whole lines.  Same table layout and probe order as
// one-slot linear probing, but at a realistic load (0.47: a 1e9-key model in
// 2^31 slots) a chain costs one extra round trip per line, not per slot.
constexpr int kPullItems = 2;
constexpr int kPullChunk = kBlock * kPullItems;
constexpr int kLineSlots = 4;  // 16-byte slots per 64-byte line

__global__ void __launch_bounds__(kBlock) k_pull_lr16(TableView t, FtrlParams fp,
                                                      const u64* __restrict__ keys,
                                                      const int64_t* n_dev, int64_t n_host,
                                                      int64_t n_max, bool insert,
                                                      u32* __restrict__ out_slot,
                                                      float* __restrict__ out_vals,
                                                      const u32* __restrict__ out_map,
                                                      float2* __restrict__ out_nz,
                                                      float* __restrict__ zero_out) {
  const int64_t n = dev_count(n_dev, n_host, n_max);
  if ((int64_t)blockIdx.x * kPullChunk >= n) return;  // (grid sized by capacity)
  const u64 segm = (1ull << t.seg_log2) - 1;  // (chains wrap inside a segment)
  uint4* slots = reinterpret_cast<uint4*>(t.words);
  const int64_t base = (int64_t)blockIdx.x * kPullChunk + threadIdx.x;
  u64 key[kPullItems], s[kPullItems];
  uint4 v[kPullItems];
#pragma unroll
  for (int j = 0; j < kPullItems; ++j) {
    int64_t i = base + (int64_t)j * kBlock;
    key[j] = i < n ? sanitize_key(keys[i]) : 0ull;
    s[j] = table_home(t, fmix64(key[j]));
  }
#pragma unroll
  for (int j = 0; j < kPullItems; ++j) {
    int64_t i = base + (int64_t)j * kBlock;
    if (i < n) v[j] = slots[s[j]];
  }
  // output rows loaded up front too: after the first key's stores the
  // compiler could not hoist them (possible aliasing), one round trip each
  u32 orow[kPullItems];
#pragma unroll
  for (int j = 0; j < kPullItems; ++j) {
    int64_t i = base + (int64_t)j * kBlock;
    orow[j] = (out_map && i < n) ? out_map[i] : (u32)i;
  }
  unsigned int claims = 0;
#pragma unroll
  for (int j = 0; j < kPullItems; ++j) {
    int64_t i = base + (int64_t)j * kBlock;
    if (i >= n) continue;
    u32 slot = kNoSlot;
    float w = 0.0f;
    float2 nz = make_float2(0.0f, 0.0f);  // fresh slot: zero state
    u64 sj = s[j];
    int q0 = (int)(sj & (kLineSlots - 1)), q1 = q0 + 1;  // registers hold [q0, q1) of the line
    uint4 ln[kLineSlots];
#pragma unroll
    for (int q = 0; q < kLineSlots; ++q) ln[q] = v[j];  // (only ln[q0] is read in round one)
    bool done = false;
    // c = slots examined so far = probe distance of the round's first slot;
    // slots at distance >= probe_limit are never examined (bounded chains)
    for (u64 c = 0; c < t.probe_limit && !done;) {
#pragma unroll
      for (int q = 0; q < kLineSlots; ++q) {
        if (q < q0 || q >= q1 || done || c + (u64)(q - q0) >= t.probe_limit) continue;
        const u64 cur = (u64)ln[q].x | ((u64)ln[q].y << 32);
        const u64 sq = (sj & ~(u64)(kLineSlots - 1)) + (u64)q;
        if (cur == key[j]) {
          slot = (u32)sq;
          nz = make_float2(__uint_as_float(ln[q].z), __uint_as_float(ln[q].w));
          w = ftrl_weight(nz.y, nz.x, fp);
          done = true;
        } else if (cur == kEmptyKey) {
          if (!insert) {
            done = true;
          } else {
            const u64 prev = atomicCAS(reinterpret_cast<unsigned long long*>(&slots[sq]),
                                       (unsigned long long)kEmptyKey, (unsigned long long)key[j]);
            if (prev == kEmptyKey) {  // fresh slot: state is zero -> w = 0
              ++claims;
              slot = (u32)sq;
              done = true;
            } else if (prev == key[j]) {  // claimed by another lane this launch
              slot = (u32)sq;
              done = true;
            }
            // else: taken by another key meanwhile -- keep probing
          }
        }
      }
      if (done) break;
      c += (u64)(q1 - q0);
      // next: the rest of this line after the home slot, then whole lines --
      // every slot of a round is loaded at once (one dependent round trip)
      if (q1 < kLineSlots) {
        q0 = q1;
      } else {
        sj = (sj & ~segm) | (((sj | (u64)(kLineSlots - 1)) + 1) & segm);
        q0 = 0;
      }
      q1 = kLineSlots;
      const uint4* line = slots + (sj & ~(u64)(kLineSlots - 1));
#pragma unroll
      for (int q = 0; q < kLineSlots; ++q)
        if (q >= q0) ln[q] = line[q];
    }
    if (insert && slot == kNoSlot) *t.overflow = 1u;
    if (out_slot) out_slot[i] = slot;
    if (out_vals) out_vals[out_map ? (int64_t)orow[j] : i] = w;
    if (out_nz) out_nz[i] = nz;
    if (zero_out) zero_out[i] = 0.0f;  // (width 1: LR)
  }
  block_count_add<kBlock>(t.size, claims);
}

__global__ void __launch_bounds__(kBlock) k_pull_generic(PullArgs a) {
  int64_t n = dev_count(a.n_dev, a.n_host, a.n_max);
  const TableView& t = a.table;
  const TableLayout& L = t.L;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  unsigned int claims = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    u64 key = sanitize_key(a.keys[i]);
    bool claimed = false;
    u32 slot = probe(t, key, a.insert, claimed);
    claims += claimed;
    if (a.out_slot) a.out_slot[i] = slot;
    if (a.out_vals) {
      float* dst = a.out_vals + (size_t)(a.out_map ? a.out_map[i] : i) * a.pstride;
      if (slot == kNoSlot) {
        for (int p = 0; p < L.P; ++p) dst[p] = absent_weight(key, p, L, a.opt);
      } else {
        const u32* sp = t.words + (u64)slot * L.stride;
        for (int p = 0; p < L.P; ++p) dst[p] = slot_weight(sp, key, p, L, a.opt);
      }
    }
  }
  block_count_add<kBlock>(t.size, claims);
}

// Multi-parameter layouts (FM / MVM / SGD): phase 1 probes one key per lane
// (kPullItems keys in flight) and records the slot; phase 2 evaluates the
// pull values with a group of G lanes per key (G = pow2 >= pstride), so the
// slot's state words and the output row are read/written contiguously.
// Keys per lane (sequential chains): 2 measured +0.6 % over 4 and 1 on FM-8
// at table load 0.47; probing slot pairs per round trip -1.2 %
// (profiles/r2_s3_fm_pull_apply_pipeline.txt).  The grid is sized by the
// capacity, so blocks past the device count return at once.
constexpr int kProbeItems = 2;
__global__ void __launch_bounds__(kBlock) k_pull_probe(TableView t, const u64* __restrict__ keys,
                                                       const int64_t* n_dev, int64_t n_host,
                                                       int64_t n_max, bool insert,
                                                       u32* __restrict__ out_slot) {
  const int64_t n = dev_count(n_dev, n_host, n_max);
  const int64_t base = (int64_t)blockIdx.x * (kBlock * kProbeItems) + threadIdx.x;
  if ((int64_t)blockIdx.x * (kBlock * kProbeItems) >= n) return;  // (grid sized by capacity)
  unsigned int claims = 0;
#pragma unroll
  for (int j = 0; j < kProbeItems; ++j) {
    int64_t i = base + (int64_t)j * kBlock;
    if (i >= n) continue;
    bool claimed = false;
    out_slot[i] = probe(t, sanitize_key(keys[i]), insert, claimed);
    claims += claimed;
  }
  block_count_add<kBlock>(t.size, claims);
}

__global__ void __launch_bounds__(kBlock) k_pull_values(PullArgs a) {
  const int64_t n = dev_count(a.n_dev, a.n_host, a.n_max);
  const TableLayout& L = a.table.L;
  const PackedLane pl = packed_lane(L.P);
  const int p = pl.p;
  const int gbase = (threadIdx.x % kWave) - p;  // lane of the group's param 0
  // (a key group's lanes share i: the group-uniform loop keeps them together
  // through the shuffles; idle lanes run no iteration)
  int64_t i = pl.on ? pl.first : n;
  RowPipe pipe;
  pipe.stride = pl.stride;
  pipe.n = n;
  pipe.start(a.out_slot, a.table.words, i, p, L);
  // the output row index one iteration ahead as well: loaded after this
  // iteration's stores it would wait for them (gfx9 vmcnt counts stores)
  u32 om_nx = (a.out_map && i < n) ? a.out_map[i] : 0u;
  for (; i < n; i += pl.stride) {
    RowPre rp;
    const u32 slot = pipe.next(a.out_slot, a.table.words, i, p, L, rp);
    const u32 om = om_nx;
    if (a.out_map && i + pl.stride < n) om_nx = a.out_map[i + pl.stride];
    float v;
    if (slot == kNoSlot) {
      v = absent_weight(sanitize_key(a.keys[i]), p, L, a.opt);
    } else {
      v = state_weight(rp.key, rp.flag != 0u, rp.s0, rp.s1, p, L, a.opt);
    }
    if (a.out_nz)  // the apply's stash (FTRL): (n, z), n = -1 for a key never pushed
      reinterpret_cast<float2*>(a.out_nz)[(size_t)i * L.P + p] =
          make_float2(slot != kNoSlot && rp.flag ? rp.s0 : -1.0f, slot != kNoSlot ? rp.s1 : 0.0f);
    if (a.out_w) {
      a.out_w[(size_t)i * a.pstride + p] = v;
      for (int c = L.P + p; c < a.pstride; c += L.P) a.out_w[(size_t)i * a.pstride + c] = 0.0f;
    }
    if (a.zero_out)
      for (int c = p; c < a.zero_width; c += L.P) a.zero_out[(size_t)i * a.zero_width + c] = 0.0f;
    if (!a.out_vals) continue;
    const size_t row = a.out_map ? (size_t)om : (size_t)i;
    if (a.fm_vals) {
      // (w, Σ_k v_k, Σ_k v_k^2) of the key, summed in param order by lane 0
      float sv = 0.0f, qv = 0.0f;
      for (int j = L.p_w; j < L.P; ++j) {
        const float x = __shfl(v, gbase + j);
        sv += x;
        qv += x * x;
      }
      if (p == 0) reinterpret_cast<float4*>(a.out_vals)[row] = make_float4(v, sv, qv, 0.0f);
    } else {
      a.out_vals[row * a.pstride + p] = v;
      for (int c = L.P + p; c < a.pstride; c += L.P) a.out_vals[row * a.pstride + c] = 0.0f;
    }
  }
}

// ---------------------------------------------------------------------------
// feature admission (AdmitView, backend.h): phases 2 and 3 of an inserting
// pull, over the entries the probe-only pull before them left without a slot
// ---------------------------------------------------------------------------
// Each lane owns kAdmitItems entries one block apart and issues their
// independent loads (slot, key, then the filter words) before it resolves
// any: an absent key's filter block is one random 64-byte line, so as in
// k_pull_lr16 memory-level parallelism is what matters.
constexpr int kAdmitItems = 2;
constexpr int kAdmitChunk = kBlock * kAdmitItems;

// counter += 1, saturating at 255, by a CAS loop on its aligned 32-bit word
// (`seen`: a value of the word loaded earlier).  Every adder that finds the
// counter below 255 adds exactly 1 and one at 255 adds nothing, so the final
// state is min(255, start + adders) whatever the order.
__device__ __forceinline__ void admit_bump(u32* __restrict__ word, int shift, u32 seen) {
  while (((seen >> shift) & 0xFFu) != 0xFFu) {
    const u32 prev = atomicCAS(word, seen, seen + (1u << shift));
    if (prev == seen) break;
    seen = prev;
  }
}

__global__ void __launch_bounds__(kBlock) k_admit_count(AdmitView av,
                                                        const u64* __restrict__ keys,
                                                        const int64_t* n_dev, int64_t n_host,
                                                        int64_t n_max,
                                                        const u32* __restrict__ slots) {
  const int64_t n = dev_count(n_dev, n_host, n_max);
  if ((int64_t)blockIdx.x * kAdmitChunk >= n) return;  // (grid sized by capacity)
  u32* words = reinterpret_cast<u32*>(av.counters);
  const int64_t base = (int64_t)blockIdx.x * kAdmitChunk + threadIdx.x;
  bool on[kAdmitItems];
  AdmitPos pos[kAdmitItems];
  u32 w0[kAdmitItems], w1[kAdmitItems];
#pragma unroll
  for (int j = 0; j < kAdmitItems; ++j) {
    const int64_t i = base + (int64_t)j * kBlock;
    on[j] = i < n && slots[i] == kNoSlot;
    pos[j] = admit_pos(on[j] ? sanitize_key(keys[i]) : 0ull, av.log2);
  }
#pragma unroll
  for (int j = 0; j < kAdmitItems; ++j) {
    if (!on[j]) continue;
    w0[j] = words[pos[j].c0 >> 2];
    w1[j] = words[pos[j].c1 >> 2];
  }
#pragma unroll
  for (int j = 0; j < kAdmitItems; ++j) {
    if (!on[j]) continue;
    admit_bump(words + (pos[j].c0 >> 2), (int)(pos[j].c0 & 3u) * 8, w0[j]);
    // (the two counters may share a word: the second loop's first compare
    // then fails once and continues from the word it finds)
    admit_bump(words + (pos[j].c1 >> 2), (int)(pos[j].c1 & 3u) * 8, w1[j]);
  }
}

// Phase 3.  Runs after every increment of the call (a launch of its own):
// all entries of one key read the same two counters and decide alike.  An
// admitted key is inserted by the table's CAS probe; entries of one key get
// one slot.  The overflow flag is set only by an admitted key that finds no
// slot within probe_limit (probe); an unadmitted entry keeps kNoSlot.
__global__ void __launch_bounds__(kBlock) k_admit_insert(TableView t, AdmitView av,
                                                         const u64* __restrict__ keys,
                                                         const int64_t* n_dev, int64_t n_host,
                                                         int64_t n_max, u32* __restrict__ slots) {
  const int64_t n = dev_count(n_dev, n_host, n_max);
  if ((int64_t)blockIdx.x * kAdmitChunk >= n) return;  // (grid sized by capacity)
  const int64_t base = (int64_t)blockIdx.x * kAdmitChunk + threadIdx.x;
  bool on[kAdmitItems];
  u64 key[kAdmitItems];
  AdmitPos pos[kAdmitItems];
  unsigned int c0[kAdmitItems], c1[kAdmitItems];
#pragma unroll
  for (int j = 0; j < kAdmitItems; ++j) {
    const int64_t i = base + (int64_t)j * kBlock;
    on[j] = i < n && slots[i] == kNoSlot;
    key[j] = on[j] ? sanitize_key(keys[i]) : 0ull;
    pos[j] = admit_pos(key[j], av.log2);
  }
#pragma unroll
  for (int j = 0; j < kAdmitItems; ++j) {
    if (!on[j]) continue;
    c0[j] = av.counters[pos[j].c0];
    c1[j] = av.counters[pos[j].c1];
  }
  unsigned int claims = 0;
#pragma unroll
  for (int j = 0; j < kAdmitItems; ++j) {
    if (!on[j]) continue;
    if ((int)(c0[j] < c1[j] ? c0[j] : c1[j]) < av.min_count) continue;
    bool claimed = false;
    slots[base + (int64_t)j * kBlock] = probe(t, key[j], true, claimed);
    claims += claimed;
  }
  block_count_add<kBlock>(t.size, claims);
}

static void launch_admit(const PullArgs& a, hipStream_t st) {
  if (a.admit.log2 < kAdmitBlockLog2 || a.admit.log2 > kAdmitMaxLog2)
    throw std::runtime_error("table_pull: admit log2");
  const int64_t nm = a.n_dev ? a.n_max : a.n_host;
  const int g = (int)((nm + kAdmitChunk - 1) / kAdmitChunk);
  hipLaunchKernelGGL(k_admit_count, dim3(g > 0 ? g : 1), dim3(kBlock), 0, st, a.admit, a.keys,
                     a.n_dev, a.n_host, a.n_max, a.out_slot);
  hipLaunchKernelGGL(k_admit_insert, dim3(g > 0 ? g : 1), dim3(kBlock), 0, st, a.table, a.admit,
                     a.keys, a.n_dev, a.n_host, a.n_max, a.out_slot);
}

void launch_table_pull(const PullArgs& a0, hipStream_t st) {
  if (a0.n_max <= 0) return;
  // admission: the kernels below only look up (present keys get their slot
  // and values; an absent key's values are those of a fresh slot already),
  // then the two admission kernels count and insert the absent entries
  const bool admit = a0.insert && a0.admit.counters != nullptr;
  PullArgs a = a0;
  if (admit) a.insert = false;
  if (admit && !a.out_slot) throw std::runtime_error("table_pull: admission needs out_slot");
  const TableLayout& L = a.table.L;
  int grid = grid_for(a.n_dev ? a.n_max : a.n_host);
  if (L.lr16()) {
    if (a.zero_out && a.zero_width != 1) throw std::runtime_error("table_pull: zero_width");
    int64_t nm = a.n_dev ? a.n_max : a.n_host;
    int g = (int)((nm + kPullChunk - 1) / kPullChunk);
    hipLaunchKernelGGL(k_pull_lr16, dim3(g > 0 ? g : 1), dim3(kBlock), 0, st, a.table, a.opt.ftrl, a.keys,
                       a.n_dev, a.n_host, a.n_max, a.insert, a.out_slot, a.out_vals, a.out_map,
                       reinterpret_cast<float2*>(a.out_nz), a.zero_out);
  } else if (a.out_slot && a.pstride >= 2 && L.P <= kWave) {
    if (a.fm_vals && L.P < 2) throw std::runtime_error("fm_vals: bad layout");
    const int64_t nm = a.n_dev ? a.n_max : a.n_host;
    const int g1 = (int)((nm + kBlock * kProbeItems - 1) / (kBlock * kProbeItems));
    hipLaunchKernelGGL(k_pull_probe, dim3(g1 > 0 ? g1 : 1), dim3(kBlock), 0, st, a.table, a.keys,
                       a.n_dev, a.n_host, a.n_max, a.insert, a.out_slot);
    if (a.out_vals || a.out_w || a.zero_out) {
      // one key per lane group where possible: the grid-stride iterations of
      // a group are dependent random-access chains (latency bound)
      hipLaunchKernelGGL(k_pull_values, dim3(packed_grid(nm, L.P)), dim3(kBlock), 0, st, a);
    }
  } else {
    if (a.fm_vals || a.out_w) throw std::runtime_error("table_pull: fm_vals/out_w need the group path");
    hipLaunchKernelGGL(k_pull_generic, dim3(grid), dim3(kBlock), 0, st, a);
  }
  if (admit) launch_admit(a0, st);
  XF_HIP_CHECK(hipGetLastError());
}

}  // namespace hip
}  // namespace xflow
