// xflow-amd: the worker-side key preparation of the HBM-resident sparse
// parameter store (gfx950).  Replaces the reference's sort/unique
// (lr_worker.cc:146-166):
//
//   dedup        persistent, epoch-stamped open-addressing scratch table: each
//                occurrence finds (or CAS-claims, for keys new to the table)
//                its key's slot and stamps it; the unique list is compacted
//                from the stamps without global atomics.  No sort at all.
//
// Also the unique-index positions of the fused single-rank step (k_remap_pos)
// and the per-owner counts of the owner-partitioned dedup (k_partition_counts).
#include "table_common.h"

namespace xflow {
namespace hip {

// ---------------------------------------------------------------------------
// dedup
// ---------------------------------------------------------------------------
// The worker dedup table is persistent across steps (see ScratchView): hot
// keys keep their slot, so after warm-up almost every occurrence is a plain
// hit.  CTR keys are extremely skewed (top-1000 keys ~60% of occurrences); a
// table cleared every step made each hot key a same-address CAS storm.
//
// Device-side rebuilds.  With ctl (adaptive capacity, the HIP engine) the
// compaction decides them: k_compact_scan switches the active capacity for
// the next batch (ctl[0]) while keeping this batch's in ctl[3], and
// k_compact_write frees the new capacity's slots right after reading its own
// (each thread owns 16 slots) -- no extra launches per step.  Without ctl the
// table is rebuilt by the two kernels below once `claims` exceeds rebuild_at.
//
// Carry-over (ScratchView::carry): a rebuild at an unchanged capacity keeps
// the slots stamped with this epoch -- the batch's own keys, the ones most
// likely to come back -- and frees the rest; see k_compact_scan and the note
// on holes above k_dedup_insert.
__device__ __forceinline__ u64 active_cap(const ScratchView& sv) {
  return sv.ctl ? (u64)sv.ctl[0] : sv.cap;
}

// capacity this batch was deduplicated with (valid after k_compact_scan)
__device__ __forceinline__ u64 batch_cap(const ScratchView& sv) {
  return sv.ctl ? (u64)sv.ctl[3] : sv.cap;
}

// this batch spilled past the active capacity (ScratchView::ctl[4])
__device__ __forceinline__ bool batch_spilled(const ScratchView& sv) {
  return sv.ctl && sv.ctl[4] == (unsigned long long)sv.epoch;
}

__global__ void k_scratch_maybe_clear(u64* __restrict__ skeys, u64 cap,
                                      const unsigned long long* __restrict__ claims,
                                      u64 rebuild_at, const unsigned long long* __restrict__ ctl) {
  u64 n = cap;
  if (ctl) {
    n = ctl[2];
    if (n == 0) return;
  } else if (*claims <= rebuild_at) {
    return;
  }
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 s = (u64)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += stride)
    skeys[s] = kEmptyKey;
}

__global__ void k_scratch_claims_reset(unsigned long long* claims, u64 rebuild_at,
                                       unsigned long long* ctl) {
  if (ctl) {
    if (ctl[2]) {
      ctl[0] = ctl[2];
      ctl[2] = 0ull;
      *claims = 0ull;
    }
  } else if (*claims > rebuild_at) {
    *claims = 0ull;
  }
}

// ScratchView::grow: rebuild at the grown capacity before the insert
// (k_scratch_maybe_clear and k_scratch_claims_reset apply ctl[2]).
__global__ void k_scratch_grow(unsigned long long* __restrict__ ctl, u64 cap_alloc, float grow) {
  const double need = (double)kScratchHeadroom * (double)ctl[1] * (double)grow;
  u64 want = kScratchMinCap;
  while ((double)want < need && want < cap_alloc) want <<= 1;
  if (want > cap_alloc) want = cap_alloc;
  ctl[2] = want > ctl[0] ? want : 0ull;
}

// Step 1 -- insert / stamp, two levels.
//   (a) workgroup level: the block's kDedupChunk occurrences (1024: measured
//       137 us per 10.2 M-key batch vs 154 at 2048, 158 at 512, 196 at 4096)
//       are deduplicated in an LDS hash table (2x oversized, 64-bit ds CAS);
//       the first occurrence of each key becomes its leader.
//   (b) global level: only leaders probe the persistent table -- all of their
//       first-probe loads in flight before any is resolved -- CAS new keys,
//       write the epoch stamp and publish the slot in LDS; every occurrence
//       then reads its slot from LDS.
// Hot keys (an int-field value can occur in half the rows) otherwise send one
// read and one stamp store per occurrence to the same L2 channel; with (a)
// they cost one per workgroup.
//
// kLead (DedupOut::lead, the leader handoff to k_lr_lead): the tile's
// grouping is handed on instead of thrown away.  A leader's LDS entry also
// carries its in-tile occurrence index (bits 32..41), a leader still writes
// pos = its slot and a follower writes pos = kLeadBit | its leader's index.
// Which occurrence of a key wins the LDS CAS is a race: consumers may rely on
// the grouping only, never on who leads.  Slots stay below kLeadBit
// (launch_dedup checks the allocation).
//
// Holes (carry-over rebuilds).  A carry-over rebuild frees some slots of a
// probe chain and keeps others, so a kept key K can sit behind a hole of its
// own chain.  The loop below needs no change for that.  Within a batch slots
// only go from empty to occupied, so "the first slot of K's chain that holds
// K or is empty" is the same slot for every leader of K: the first leader to
// reach the hole claims it with one CAS (or loses the CAS to another leader
// of K and reads K back), every other leader probes from the same home and
// meets that slot before the old copy.  All of K's occurrences get the one
// slot and only it is stamped, so K is in the unique list once (the list
// holds stamped slots only).  The old copy behind it is never reached again,
// so never stamped again, and goes at the next rebuild; until then it only
// occupies a slot (the occupancy counter counted it when it was claimed).
// Which slot a key gets was a CAS race before and no result depends on it.
constexpr int kDedupItems = 4;
constexpr int kDedupChunk = kBlock * kDedupItems;
constexpr int kDedupLog2 = 11;  // LDS slots = 2 * kDedupChunk
static_assert((1 << kDedupLog2) == 2 * kDedupChunk, "LDS dedup table sizing");
static_assert(kDedupChunk == kLeadTile, "the handoff's tile is the dedup chunk");

template <bool kLead>
__global__ void __launch_bounds__(kBlock) k_dedup_insert(const u64* __restrict__ keys, int64_t nnz,
                                                         ScratchView sv, u32* __restrict__ pos,
                                                         u32* __restrict__ overflow) {
  constexpr u32 kL = 1u << kDedupLog2;
  __shared__ u64 t_key[kL];  // keys during the LDS level, then leaders' slots
  u64* __restrict__ skeys = sv.keys;
  const u64 cap = active_cap(sv), mask = cap - 1;
  const u32 parts = (u32)sv.parts;
  const u64 R = parts > 1 ? cap / parts : cap;  // probe range per owner
  // (ScratchView::home_bits: the top bits of the table home's hash bits)
  const int clog = 63 - __clzll((long long)cap);
  const int hshift = sv.home_bits > clog ? sv.home_bits - clog : 0;
  const int64_t base = (int64_t)blockIdx.x * kDedupChunk + threadIdx.x;
  for (u32 i = threadIdx.x; i < kL; i += kBlock) t_key[i] = kEmptyKey;
  u64 k[kDedupItems], s[kDedupItems];
  u32 h[kDedupItems];
#pragma unroll
  for (int j = 0; j < kDedupItems; ++j) {
    int64_t i = base + (int64_t)j * kBlock;
    k[j] = i < nnz ? sanitize_key(keys[i]) : 0ull;
    const u64 f = fmix64(k[j]);
    s[j] = parts > 1 ? (u64)((u32)(f >> 32) % parts) * R + (((f & 0xffffffffull) * R) >> 32)
                     : (f >> hshift) & mask;
    h[j] = (u32)(f >> (64 - kDedupLog2));
  }
  __syncthreads();
  u32 lead = 0;
#pragma unroll
  for (int j = 0; j < kDedupItems; ++j) {
    if (base + (int64_t)j * kBlock >= nnz) continue;
    u32 x = h[j];
    while (true) {  // (one CAS against an empty slot per probe step, no read first)
      const u64 prev = atomicCAS((unsigned long long*)&t_key[x], (unsigned long long)kEmptyKey,
                                 (unsigned long long)k[j]);
      if (prev == kEmptyKey) {
        lead |= 1u << j;
        break;
      }
      if (prev == k[j]) break;
      x = (x + 1) & (kL - 1);  // <= kDedupChunk keys in kL slots: terminates
    }
    h[j] = x;
  }
  // every LDS lookup is done: the leaders' table entries can now carry slots
  __syncthreads();
  // global level, leaders only: all first-probe loads in flight, then each
  // leader resolves (CAS only for keys new to the table)
  u64 cur[kDedupItems];
#pragma unroll
  for (int j = 0; j < kDedupItems; ++j) cur[j] = (lead >> j) & 1u ? skeys[s[j]] : k[j];
  unsigned int claimed = 0;
#pragma unroll
  for (int j = 0; j < kDedupItems; ++j) {
    if (!((lead >> j) & 1u)) continue;
    u64 sj = s[j], c = cur[j];
    u64 n = 0;
    while (c != k[j]) {
      if (c == kEmptyKey) {
        u64 prev = atomicCAS((unsigned long long*)&skeys[sj], (unsigned long long)kEmptyKey,
                             (unsigned long long)k[j]);
        if (prev == kEmptyKey) {
          ++claimed;
          break;
        }
        if (prev == k[j]) break;
      }
      if (++n >= R) {
        // the active table is full (a surge of distinct keys): probe on in
        // the rest of the allocation, which this batch's compaction then
        // covers (ScratchView::ctl[4])
        if (sv.ctl && parts == 1 && cap < sv.cap && n == R) {
          sv.ctl[4] = sv.epoch;
          const u64 Z = sv.cap - cap;
          sj = cap + fmix64(k[j]) % Z;
          c = skeys[sj];
          for (u64 m = 0; c != k[j]; ) {
            if (c == kEmptyKey) {
              u64 prev = atomicCAS((unsigned long long*)&skeys[sj], (unsigned long long)kEmptyKey,
                                   (unsigned long long)k[j]);
              if (prev == kEmptyKey) {
                ++claimed;
                break;
              }
              if (prev == k[j]) break;
            }
            if (++m >= Z) {
              sj = sv.cap;
              break;
            }
            if (++sj == sv.cap) sj = cap;
            c = skeys[sj];
          }
          if (sj < sv.cap) break;
        }
        // no free slot: the key's occurrences go to the trash slot (index
        // cap: never stamped, so never in the unique list; its pulled row is
        // zero and its gradients are dropped) and the step is flagged --
        // never merged into another key's slot
        *overflow = 1u;
        sj = sv.cap;
        break;
      }
      if (parts > 1) {
        ++sj;
        if (sj % R == 0) sj -= R;  // wrap inside the owner's range
      } else {
        sj = (sj + 1) & mask;
      }
      c = skeys[sj];
    }
    XF_DASSERT(sj <= sv.cap);
    if constexpr (kLead) {
      XF_DASSERT(sj < kLeadBit);
      t_key[h[j]] = sj | ((u64)(j * kBlock + (int)threadIdx.x) << 32);
    } else {
      t_key[h[j]] = sj;
    }
    if (sj < sv.cap) sv.stamps[sj] = (unsigned char)sv.epoch;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kDedupItems; ++j) {
    int64_t i = base + (int64_t)j * kBlock;
    if (i >= nnz) continue;
    const u64 e = t_key[h[j]];
    if constexpr (kLead) pos[i] = (lead >> j) & 1u ? (u32)e : kLeadBit | (u32)(e >> 32);
    else pos[i] = (u32)e;
  }
  // one no-return atomic per workgroup for the rebuild counter
  block_count_add<kBlock>(sv.claims, claimed);
}

// Step 2 -- compaction of the slots stamped with this epoch into the unique
// list, without a single global atomic: (a) each workgroup counts its 4096
// slots (coalesced stamp reads), (b) one workgroup scans the counts, (c) each
// workgroup re-reads its stamps (L3/L2 resident) and writes (key, slot) at
// its offset.  Output order = slot order: deterministic.
constexpr int kCompactItems = 16;
constexpr int kCompactChunk = kBlock * kCompactItems;
static_assert(kCompactChunk == 1 << kCompactChunkLog2, "k_red_sum ranks slots by these chunks");

// 16 consecutive byte stamps as one dwordx4 load (cap is a power of two >=
// 16, so a 16-slot group is either fully inside the table or fully outside).
__device__ __forceinline__ unsigned int compact_hits(const ScratchView& sv, u64 base, u64 cap,
                                                     unsigned int& cnt) {
  unsigned int hit = 0;
  cnt = 0;
  if (base >= cap) return 0;
  const uint4 q = *reinterpret_cast<const uint4*>(sv.stamps + base);
  const u32 w[4] = {q.x, q.y, q.z, q.w};
  const u32 e = sv.epoch & 0xFFu;
#pragma unroll
  for (int j = 0; j < 16; ++j) hit |= (unsigned int)(((w[j >> 2] >> (8 * (j & 3))) & 0xFFu) == e) << j;
  cnt = __popc(hit);
  return hit;
}

// lane t owns the 16 consecutive slots [base + 16t, base + 16t + 16): the
// stamp loads are dwordx4-able and the output stays in slot order
__global__ void __launch_bounds__(kBlock) k_compact_count(ScratchView sv,
                                                          unsigned int* __restrict__ counts) {
  const u64 base = (u64)blockIdx.x * kCompactChunk + (u64)threadIdx.x * kCompactItems;
  unsigned int cnt;
  compact_hits(sv, base, batch_spilled(sv) ? sv.cap : active_cap(sv), cnt);
  unsigned int tot;
  block_exclusive_scan<kBlock>(cnt, &tot);
  if (threadIdx.x == 0) counts[blockIdx.x] = tot;
}

// Also sizes the scratch for the next batch (ctl): active cap = the power of
// two >= kScratchHeadroom x the largest batch seen, rebuilt when it should
// grow, when it is 4x too large, or when the rebuild counter passes its
// threshold.  A rebuild takes effect here: ctl[3] keeps this batch's capacity
// for k_compact_write / k_partition_counts, ctl[0] becomes the new one,
// ctl[2] tells k_compact_write how many slots to free and ctl[5] how.
//
// Without carry-over the counter holds the keys claimed since the last
// rebuild, a rebuild frees every slot and comes once they pass half the
// table.  With it (ScratchView::carry) a rebuild at an unchanged capacity of
// a batch that did not spill keeps the batch's own slots -- `carry` below, the
// unique count, is exactly their number -- so the counter restarts there and
// means occupied slots, and the rebuild comes at kCarryRebuildEighths / 8 of
// the table: a rebuild no longer makes the next batch claim its hot keys
// again, so it can come earlier and keep the probe chains shorter.  A resize,
// a spilled batch and a batch over 1 / kScratchHeadroom of the table (a
// capacity clamped to the allocation) keep the full clear.
// (interleaved A/B on the bench step, profiles/dedup_carry_ab.txt: 3/8 -- a
// two-step cycle at insert loads 0.20 / 0.35 -- beat 1/2 and a rebuild in
// every step; 0 would mean every step)
constexpr u64 kCarryRebuildEighths = 3;
static_assert(kCarryRebuildEighths <= 4, "stale claims <= cur / 2 at a batch start");

__global__ void __launch_bounds__(kScanBlock) k_compact_scan(
    unsigned int* __restrict__ counts, int nb, unsigned long long* __restrict__ n_out,
    unsigned long long* __restrict__ claims, unsigned long long* __restrict__ ctl,
    u64 cap_alloc, unsigned long long* __restrict__ n_copy,
    unsigned long long* __restrict__ cap_out, u32 epoch, bool carry_on) {
  // only the blocks of this batch's capacity hold stamps (the rest count 0):
  // at 4x headroom that is 1/8 of the allocation's blocks
  if (ctl) {
    const u64 lim = ctl[4] == epoch ? cap_alloc : (u64)ctl[0];  // (read before thread 0 updates ctl)
    const u64 nbl = (lim + kCompactChunk - 1) / kCompactChunk;
    if (nbl < (u64)nb) nb = (int)nbl;
  }
  unsigned long long carry = 0;
  for (int c0 = 0; c0 < nb; c0 += kScanBlock) {
    int i = c0 + (int)threadIdx.x;
    unsigned int v = i < nb ? counts[i] : 0u;
    unsigned int tot;
    unsigned int ex = block_exclusive_scan<kScanBlock>(v, &tot);
    if (i < nb) counts[i] = (unsigned int)(carry + ex);  // exclusive offsets (< 2^32 slots)
    carry += tot;
  }
  if (threadIdx.x == 0) {
    *n_out = carry;
    if (n_copy) *n_copy = carry;  // e.g. the one-owner counts of a world-1 sharded step
    if (ctl) {
      const u64 mx = ctl[1] > carry ? ctl[1] : carry;
      ctl[1] = mx;
      u64 want = kScratchMinCap;
      while (want < kScratchHeadroom * mx && want < cap_alloc) want <<= 1;
      if (want > cap_alloc) want = cap_alloc;
      const u64 cur = ctl[0];
      // (stale claims <= cur / 2 at a batch start: 2x the most unique keys
      // seen fit in the active table; a larger surge spills, see ctl[4].
      // With carry-over: at most the threshold <= cur / 2 without a rebuild,
      // the kept keys <= cur / kScratchHeadroom after one)
      const bool resize = want > cur || want * 4 <= cur;
      const u64 full_at = carry_on ? cur * kCarryRebuildEighths / 8 : cur / 2;
      const bool rebuild = *claims > full_at || resize;
      const bool keep = carry_on && rebuild && !resize && ctl[4] != epoch &&
                        carry * kScratchHeadroom <= cur;
      ctl[3] = cur;
      ctl[2] = rebuild ? want : 0ull;
      ctl[5] = keep ? 1ull : 0ull;
      if (rebuild) {
        ctl[0] = want;
        *claims = keep ? carry : 0ull;
        ctl[6] += 1ull;
        ctl[7] = keep ? carry : 0ull;
      }
    }
    // (the reduction's bucket geometry: a spilled batch's slots reach cap_alloc)
    if (cap_out) *cap_out = ctl && ctl[4] != epoch ? ctl[3] : cap_alloc;
  }
}

__global__ void __launch_bounds__(kBlock) k_compact_write(ScratchView sv,
                                                          const unsigned int* __restrict__ offs,
                                                          u64* __restrict__ uk,
                                                          u32* __restrict__ up,
                                                          u32* __restrict__ inv) {
  const u64 base = (u64)blockIdx.x * kCompactChunk + (u64)threadIdx.x * kCompactItems;
  unsigned int cnt;
  unsigned int hit = compact_hits(sv, base, batch_spilled(sv) ? sv.cap : batch_cap(sv), cnt);
  unsigned int tot;
  unsigned int ex = block_exclusive_scan<kBlock>(cnt, &tot);
  unsigned long long dst = (unsigned long long)offs[blockIdx.x] + ex;
  u32 iv[kCompactItems];
  // the thread's 16 keys (one 128-byte line) loaded before any store: the
  // stores to uk may alias sv.keys for the compiler, which would otherwise
  // serialise one load round trip per hit
  u64 kv[kCompactItems];
  if (hit) {
    const ulonglong2* kp = reinterpret_cast<const ulonglong2*>(sv.keys + base);
#pragma unroll
    for (int q = 0; q < kCompactItems / 2; ++q) {
      const ulonglong2 v = kp[q];
      kv[2 * q] = v.x;
      kv[2 * q + 1] = v.y;
    }
  }
#pragma unroll
  for (int j = 0; j < kCompactItems; ++j) {
    iv[j] = 0xFFFFFFFFu;
    if (!(hit & (1u << j))) continue;
    u64 s = base + (u64)j;
    uk[dst] = kv[j];
    up[dst] = (u32)s;
    iv[j] = (u32)dst;
    ++dst;
  }
  // inv for all of the thread's slots as four dwordx4 stores (whole lines
  // instead of ~10 % scattered dword stores); non-hit slots get a sentinel
  if (inv && hit) {
    uint4* ip = reinterpret_cast<uint4*>(inv + base);
#pragma unroll
    for (int j = 0; j < kCompactItems / 4; ++j)
      ip[j] = make_uint4(iv[4 * j], iv[4 * j + 1], iv[4 * j + 2], iv[4 * j + 3]);
  }
  // rebuild decided by k_compact_scan: free this thread's slots of the new
  // capacity (its own slots, already read above).  A carry-over rebuild
  // (ctl[5]; the capacity is the batch's) keeps the slots stamped with this
  // epoch: the line goes back whole, kv[j] where hit -- nothing else touches
  // the scratch while the compaction runs
  const u64 fresh = sv.ctl ? (u64)sv.ctl[2] : 0ull;
  if (base < fresh) {
    ulonglong2* kp = reinterpret_cast<ulonglong2*>(sv.keys + base);
    if (hit && sv.ctl[5]) {
#pragma unroll
      for (int j = 0; j < kCompactItems / 2; ++j)
        kp[j] = make_ulonglong2(hit & (1u << (2 * j)) ? kv[2 * j] : kEmptyKey,
                                hit & (1u << (2 * j + 1)) ? kv[2 * j + 1] : kEmptyKey);
    } else {
#pragma unroll
      for (int j = 0; j < kCompactItems / 2; ++j) kp[j] = make_ulonglong2(kEmptyKey, kEmptyKey);
    }
  }
}

// Unique-index positions (the fused single-rank step): each occurrence's
// scratch slot becomes its index in the batch's unique list (inv, written by
// the compaction), the trash slot's occurrences get `none`.  Pulled rows,
// gradient destinations (unique * S + s) and the unique-order outputs then
// share one dense index space: the reductions span the batch's unique keys
// instead of the 4x-headroom scratch capacity, the pulled rows are 4x denser
// in the caches, and no slot -> unique map is read at the output.  Four
// occurrences per lane (dwordx4 in and out, four independent gathers: 39.7 us
// per 10.2 M occurrences; sixteen per lane measured 44.7 us).
constexpr int kRemapPer = 4;

__global__ void __launch_bounds__(kBlock) k_remap_pos(u32* __restrict__ pos, int64_t nnz,
                                                      const u32* __restrict__ inv, u32 none) {
  const int64_t i = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kRemapPer;
  auto map = [&](u32 u) { return u == 0xFFFFFFFFu ? none : u; };
  if (i + kRemapPer <= nnz) {
    uint4 p[kRemapPer / 4];
#pragma unroll
    for (int q = 0; q < kRemapPer / 4; ++q) p[q] = reinterpret_cast<const uint4*>(pos + i)[q];
    u32 u[kRemapPer];
#pragma unroll
    for (int q = 0; q < kRemapPer / 4; ++q) {
      u[4 * q] = inv[p[q].x];
      u[4 * q + 1] = inv[p[q].y];
      u[4 * q + 2] = inv[p[q].z];
      u[4 * q + 3] = inv[p[q].w];
    }
#pragma unroll
    for (int q = 0; q < kRemapPer / 4; ++q)
      reinterpret_cast<uint4*>(pos + i)[q] =
          make_uint4(map(u[4 * q]), map(u[4 * q + 1]), map(u[4 * q + 2]), map(u[4 * q + 3]));
  } else {
    for (int64_t j = i; j < nnz; ++j) pos[j] = map(inv[pos[j]]);
  }
}

void launch_remap_pos(u32* pos, int64_t nnz, const u32* inv, u32 none, hipStream_t st) {
  if (nnz <= 0) return;
  if (reinterpret_cast<uintptr_t>(pos) & 15) throw std::runtime_error("remap_pos: pos must be 16-byte aligned");
  const int64_t lanes = (nnz + kRemapPer - 1) / kRemapPer;
  hipLaunchKernelGGL(k_remap_pos, dim3((unsigned)((lanes + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     st, pos, nnz, inv, none);
  XF_HIP_CHECK(hipGetLastError());
}

// Owner-partitioned dedup: the unique list is in slot order, so owner o's
// keys start at the number of stamped slots below o*R = the compaction offset
// of the chunk holding o*R plus the hits in that chunk below it (one wave per
// boundary, 64 slots per lane).  counts[o] = start[o+1] - start[o].
constexpr int kPartBlock = 1024;

__global__ void __launch_bounds__(kPartBlock) k_partition_counts(
    ScratchView sv, const unsigned int* __restrict__ offs, const int64_t* __restrict__ n_uniq,
    int64_t* __restrict__ counts, int64_t seq) {
  __shared__ int64_t start[kMaxParts + 1];
  const u32 parts = (u32)sv.parts;
  const u64 R = batch_cap(sv) / parts;
  const int lane = threadIdx.x % kWave, w = threadIdx.x / kWave;
  for (u32 o = w; o <= parts; o += kPartBlock / kWave) {
    if (o == 0 || o == parts) {
      if (lane == 0) start[o] = o == 0 ? 0 : *n_uniq;
      continue;
    }
    const u64 b = (u64)o * R, c = b / kCompactChunk, c0 = c * kCompactChunk;
    unsigned int hits = 0;
    for (u64 q = c0 + (u64)lane * 64; q < c0 + (u64)lane * 64 + 64; ++q)
      hits += (q < b && sv.stamps[q] == (unsigned char)sv.epoch) ? 1u : 0u;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) hits += __shfl_xor(hits, d);
    if (lane == 0) start[o] = (int64_t)offs[c] + hits;
  }
  __syncthreads();
  for (u32 o = threadIdx.x; o < parts; o += kPartBlock) {
    XF_DASSERT(start[o + 1] >= start[o]);
    const int64_t c = start[o + 1] - start[o];
    counts[o] = seq >= 0 ? encode_count(c, seq) : c;
  }
}

void launch_partition_counts(const ScratchView& s, const u32* chunk_offsets,
                             const int64_t* n_uniq, int64_t* counts, int64_t seq, hipStream_t st) {
  if (s.parts < 2 || s.parts > kMaxParts) throw std::runtime_error("partition_counts: bad parts");
  hipLaunchKernelGGL(k_partition_counts, dim3(1), dim3(kPartBlock), 0, st, s, chunk_offsets,
                     n_uniq, counts, seq);
  XF_HIP_CHECK(hipGetLastError());
}

void launch_dedup(const u64* keys, int64_t nnz, ScratchView s, DedupOut o, hipStream_t st) {
  if (nnz <= 0) return;
  if (!s.ctl || s.grow > 0.0f) {
    // fixed capacity: threshold rebuild before the batch; adaptive: growth
    if (s.ctl) hipLaunchKernelGGL(k_scratch_grow, dim3(1), dim3(1), 0, st, s.ctl, s.cap, s.grow);
    hipLaunchKernelGGL(k_scratch_maybe_clear, dim3(grid_for((int64_t)s.cap)), dim3(kBlock), 0, st,
                       s.keys, s.cap, s.claims, s.rebuild_at, s.ctl);
    hipLaunchKernelGGL(k_scratch_claims_reset, dim3(1), dim3(1), 0, st, s.claims, s.rebuild_at,
                       s.ctl);
  }
  int g1 = (int)((nnz + kDedupChunk - 1) / kDedupChunk);
  if (o.lead) {
    // (whole tiles only, and slots -- the trash slot included -- below the follower bit)
    if (nnz % kDedupChunk || s.cap >= kLeadBit || s.parts != 1)
      throw std::runtime_error("dedup: the leader handoff needs whole tiles and < 2^31 slots");
    hipLaunchKernelGGL(k_dedup_insert<true>, dim3(g1), dim3(kBlock), 0, st, keys, nnz, s, o.pos,
                       o.overflow);
  } else {
    hipLaunchKernelGGL(k_dedup_insert<false>, dim3(g1), dim3(kBlock), 0, st, keys, nnz, s, o.pos,
                       o.overflow);
  }
  if (!o.block_counts) throw std::runtime_error("dedup: block_counts workspace missing");
  // sized for the allocated capacity; blocks past the active one count zero
  int g2 = (int)((s.cap + kCompactChunk - 1) / kCompactChunk);
  hipLaunchKernelGGL(k_compact_count, dim3(g2), dim3(kBlock), 0, st, s, o.block_counts);
  hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(kScanBlock), 0, st, o.block_counts, g2,
                     reinterpret_cast<unsigned long long*>(o.n_uniq), s.claims, s.ctl, s.cap,
                     reinterpret_cast<unsigned long long*>(o.n_uniq_copy), o.cap_out, s.epoch,
                     s.carry);
  hipLaunchKernelGGL(k_compact_write, dim3(g2), dim3(kBlock), 0, st, s, o.block_counts,
                     o.uniq_keys, o.uniq_pos, o.inv);
  XF_HIP_CHECK(hipGetLastError());
}

}  // namespace hip
}  // namespace xflow
