// xflow-amd: scalar bucket reduction of the LR / reference-FM gradient records
// and its CSR form (gfx950); k_red_scatter, which the vector reduction
// shares, is in model_common.h.
#include "model_common.h"

namespace xflow {
namespace hip {

// ---------------------------------------------------------------------------
// LR gradient reduction without global atomics (FwdArgs::red_*).
// Scattered float atomics execute at the memory side at ~20 G adds/s on
// gfx950 (one 4-byte add per lane, 64 rows per wave instruction), which made
// the ~3 M per-column partial sums of a Criteo-shaped batch cost ~145 us.
// Here they are partitioned by destination bucket (dest >> kRedShift) with
// plain stores and summed per bucket in a 64 KB LDS accumulator.
//   1. k_red_scan     per bucket: exclusive scan of the workgroups' counts
//   2. k_red_scatter  per producing workgroup: bucket starts (scan of the
//                     bucket totals), then its pairs to their bucket ranges
//   3. k_red_sum      per bucket: LDS sums, one plain store per non-zero dest
// The LR handoff step (FwdArgs::red_local) runs 3 alone, on the segments of
// the producers' bucket-sorted regions (k_red_sum_local).
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) k_red_scan(u32* __restrict__ hist, int groups,
                                                     u32* __restrict__ tot, RedGeom geom,
                                                     int base) {
  if ((int)blockIdx.x >= geom.active(geom.shift(base), (int)gridDim.x)) return;
  const size_t row = (size_t)blockIdx.x * groups;
  u32 carry = 0;
  for (int c0 = 0; c0 < groups; c0 += kBlock) {
    const int i = c0 + (int)threadIdx.x;
    const u32 v = i < groups ? hist[row + i] : 0u;
    u32 t;
    const u32 ex = block_exclusive_scan<kBlock>(v, &t);
    if (i < groups) hist[row + i] = carry + ex;
    carry += t;
  }
  if (threadIdx.x == 0) tot[blockIdx.x] = carry;
}

// A bucket's sums are either initialised and written densely (all kR dests)
// or per record: with the 4x-headroom dedup scratch and S slices, a bucket's
// dests are mostly untouched (S = 8 at bench shape: ~1500 records over 16384
// dests), and the dense passes cost more than the per-record phases on
// register-held records.
//
// One (bucket, sub) unit of k_red_sum: records [beg, end) of bucket b, dests
// [lo, lo + kR).  Barriers are LDS-only: a unit's global stores need not land
// before the next unit starts.
//
// kSeg (k_red_sum_local): the bucket's records are not a range of `sorted`
// but one segment per producer workgroup, in the producers' bucket-sorted
// regions (LeadSegs).  Wave w takes the workgroups [w per, w per + per), per =
// ceil(groups / waves), their lead_seg words held one per lane; a segment is
// read 64 records at a time, its lanes' loads coalesced.  The sums, the rank
// machinery and the outputs are the range form's.
template <int NV, bool kSeg = false>
__device__ __forceinline__ void red_sum_unit(u64 lo, u32 beg, u32 end,
                                             const void* __restrict__ sorted, const RedFinal& f,
                                             long long* acc, u32* pbits, u32* cbits, u32* rpre,
                                             u32* rwt, const LeadSegs& sg = LeadSegs{}) {
  using T = typename RedRec<NV>::T;
  constexpr int kShift = red_shift(NV);
  constexpr u32 kR = 1u << kShift;
  constexpr int kFx = FxBits<NV>::kFx;
  static_assert(!kSeg || NV == 1, "segments: LR records");
  if (kSeg ? !sg.any : beg == end) return;
  // Unique-order outputs without the slot -> unique map (RedFinal::rk_offs;
  // one slice, so dests are slots and pbits is free): lane w < kR / 32 turns
  // the 32 stamps of slots [lo + 32 w, + 32) into bitmap word w (bit: the slot
  // is in the batch) and takes the word's rank -- its chunk's compaction
  // offset plus the set bits of the chunk's words before it.  A chunk is two
  // waves' words: a wave scan, plus the even wave's total for the odd one
  // (added after the first barrier below).  Slots at or past the capacity the
  // compaction covered (the trash slot) have no bit.
  constexpr u32 kRw = kR / 32;
  constexpr u32 kChunkW = (1u << kCompactChunkLog2) / 32;
  static_assert(kRw <= (u32)kRedBlock && kChunkW == 2 * kWave && kRw % kChunkW == 0,
                "a unit is whole chunks, a chunk two waves of bitmap words");
  // FTRL in place of the unique-order store (RedFinal::ap_*, below)
  const bool apply = kSeg && f.ap_slots;                // (block-uniform)
  const bool rank = (f.out || apply) && f.rk_offs;      // (block-uniform)
  u32 rk_pre = 0;
  if (rank && threadIdx.x < kRw) {
    const u32 w = threadIdx.x;
    const u64 base = lo + 32ull * w;
    u32 m = 0;
    const u64 cap = (u64)*f.rk_cap;  // (a power of two >= 16: whole 16-slot groups)
    if (base < cap) {
      const uint4* sp = reinterpret_cast<const uint4*>(f.rk_stamps + base);
      const uint4 q0 = sp[0], q1 = base + 16 < cap ? sp[1] : make_uint4(0u, 0u, 0u, 0u);
      rk_pre = f.rk_offs[base >> kCompactChunkLog2];
      const u32 sw[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
      const u32 e = f.rk_epoch & 0xFFu;
#pragma unroll
      for (int j = 0; j < 32; ++j) m |= (u32)(((sw[j >> 2] >> (8 * (j & 3))) & 0xFFu) == e) << j;
    }
    pbits[w] = m;
    const u32 c = (u32)__popc(m);
    u32 incl = c;
    const int lane = (int)(w % kWave);
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const u32 t = __shfl_up(incl, o);
      if (lane >= o) incl += t;
    }
    rk_pre += incl - c;
    if (lane == kWave - 1) rwt[w / kWave] = incl;
  }
  // sparse units hold their records in registers across the three phases
  constexpr int kSp = 2 * kRedUnroll;
  // (kSeg: a wave's slots are rows of 64 records, one segment each -- sparse
  // when every wave's segments fit its kSp rows, k_red_sum_local)
  const bool dense = kSeg ? sg.dense : end - beg > (u32)(kSp * kRedBlock);  // (block-uniform)
  constexpr u32 kWaves = kRedBlock / kWave;
  const u32 lane = threadIdx.x % kWave;
  const u32 sper = kSeg ? (sg.groups + kWaves - 1) / kWaves : 0u;
  const u32 sgb = (threadIdx.x / kWave) * sper;
  const u32 sge = sgb + sper < sg.groups ? sgb + sper : sg.groups;
  const T* src = static_cast<const T*>(sorted);
  const u64 S = (u64)f.S;
  auto add = [&](const T& r, u32 l) {
    if (f.masks) atomicOr(&pbits[l >> 5], 1u << (l & 31));
    if constexpr (NV == 1) {
      atomicAdd(reinterpret_cast<unsigned long long*>(&acc[l]),
                (unsigned long long)fx_from<kFx>(__uint_as_float((u32)(r >> 32))));
    } else {
      atomicAdd(reinterpret_cast<unsigned long long*>(&acc[l * 2]),
                (unsigned long long)fx_from<kFx>(__uint_as_float(r.y)));
      atomicAdd(reinterpret_cast<unsigned long long*>(&acc[l * 2 + 1]),
                (unsigned long long)fx_from<kFx>(__uint_as_float(r.z)));
    }
  };
  T pr[kSp];
  u32 lr[kSp];  // (sparse) the record's local dest, kR: none
  if (dense) {
    for (u32 i = threadIdx.x; i < kR * NV; i += kRedBlock) acc[i] = 0ll;
    if (f.masks)
      for (u32 i = threadIdx.x; i < kR / 32; i += kRedBlock) pbits[i] = 0u;
    lds_barrier();
    if constexpr (kSeg) {
      // kRedUnroll segments' first rows in flight, then their adds, then the
      // rest of a segment longer than a row
      for (u32 c0 = sgb; c0 < sge; c0 += kWave) {
        const u32 mine = c0 + lane < sge ? sg.row[c0 + lane] : 0u;
        const u32 n = sge - c0 < (u32)kWave ? sge - c0 : (u32)kWave;
        for (u32 k0 = 0; k0 < n; k0 += kRedUnroll) {
          u32 off[kRedUnroll], cnt[kRedUnroll];
          const T* reg[kRedUnroll];
#pragma unroll
          for (int q = 0; q < kRedUnroll; ++q) {
            // (lanes at or past n hold no segment: k0 + q < kWave)
            sg.seg(__shfl(mine, (int)k0 + q), off[q], cnt[q]);
            reg[q] = reinterpret_cast<const T*>(sg.pairs) + (u64)(c0 + k0 + q) * sg.gcap + off[q];
            if (lane < cnt[q]) pr[q] = reg[q][lane];
          }
#pragma unroll
          for (int q = 0; q < kRedUnroll; ++q) {
            if (lane >= cnt[q]) continue;
            const u64 d = (u64)RedRec<NV>::dest(pr[q]), l = d - lo;
            if (l < kR) add(pr[q], (u32)l);  // (else another unit's dest)
          }
#pragma unroll
          for (int q = 0; q < kRedUnroll; ++q) {
            for (u32 i0 = kWave + lane; i0 < cnt[q]; i0 += kRedUnroll * kWave) {
              T tr[kRedUnroll];
#pragma unroll
              for (int e = 0; e < kRedUnroll; ++e)
                if (i0 + (u32)e * kWave < cnt[q]) tr[e] = reg[q][i0 + (u32)e * kWave];
#pragma unroll
              for (int e = 0; e < kRedUnroll; ++e) {
                if (i0 + (u32)e * kWave >= cnt[q]) continue;
                const u64 d = (u64)RedRec<NV>::dest(tr[e]), l = d - lo;
                if (l < kR) add(tr[e], (u32)l);
              }
            }
          }
        }
      }
    } else {
      for (u32 i0 = beg + threadIdx.x; i0 < end; i0 += kRedUnroll * kRedBlock) {
#pragma unroll
        for (int q = 0; q < kRedUnroll; ++q) {
          const u32 i = i0 + (u32)q * kRedBlock;
          if (i < end) pr[q] = src[i];
        }
#pragma unroll
        for (int q = 0; q < kRedUnroll; ++q) {
          if (i0 + (u32)q * kRedBlock >= end) continue;
          const u64 d = (u64)RedRec<NV>::dest(pr[q]), l = d - lo;
          if (l < kR) add(pr[q], (u32)l);  // (else another unit's dest)
        }
      }
    }
  } else {
    if constexpr (kSeg) {
      // slot q: the wave's q-th row of 64 records, walking its segments in
      // order (sparse: at most kWave segments, at most kSp rows in all)
      const u32 mine = sgb + lane < sge ? sg.row[sgb + lane] : 0u;
      u32 k = 0, i0 = 0, off, cnt;
      sg.seg(__shfl(mine, 0), off, cnt);
#pragma unroll
      for (int q = 0; q < kSp; ++q) {
        while (i0 >= cnt && k + 1 < (u32)kWave) {  // (wave-uniform)
          ++k;
          i0 = 0;
          sg.seg(__shfl(mine, (int)k), off, cnt);
        }
        lr[q] = kR;
        if (i0 + lane < cnt) {
          pr[q] = (reinterpret_cast<const T*>(sg.pairs) + (u64)(sgb + k) * sg.gcap + off)[i0 + lane];
          const u64 d = (u64)RedRec<NV>::dest(pr[q]), l = d - lo;
          if (l < kR) lr[q] = (u32)l;
        }
        i0 += kWave;
      }
    } else {
#pragma unroll
      for (int q = 0; q < kSp; ++q) {
        const u32 i = beg + threadIdx.x + (u32)q * kRedBlock;
        lr[q] = kR;
        if (i < end) {
          pr[q] = src[i];
          const u64 d = (u64)RedRec<NV>::dest(pr[q]), l = d - lo;
          if (l < kR) lr[q] = (u32)l;
        }
      }
    }
    // zero what the records touch (same-value plain stores), and for the
    // masks every bitmap word their slots' dests cover
#pragma unroll
    for (int q = 0; q < kSp; ++q) {
      const u32 l = lr[q];
      if (l >= kR) continue;
#pragma unroll
      for (int v = 0; v < NV; ++v) acc[(u64)l * NV + v] = 0ll;
      cbits[l >> 5] = 0u;
      if (f.masks) {
        const u64 d0 = ((lo + l) / S) * S;
        const u64 a0 = d0 > lo ? d0 - lo : 0, a1 = d0 + S - 1 - lo;
        pbits[a0 >> 5] = 0u;
        if (a1 < kR) pbits[a1 >> 5] = 0u;
      }
    }
    lds_barrier();
#pragma unroll
    for (int q = 0; q < kSp; ++q)
      if (lr[q] < kR) add(pr[q], lr[q]);
  }
  // (the waves' totals were stored before the barrier above)
  if (rank && threadIdx.x < kRw) {
    const u32 wv = threadIdx.x / kWave;
    rpre[threadIdx.x] = rk_pre + ((wv & 1u) ? rwt[wv - 1] : 0u);
  }
  lds_barrier();
  // unique index of the unit's slot lo + l from the bitmap and the word ranks;
  // none (0xFFFFFFFF) for a slot the batch did not stamp
  auto rank_of = [&](u32 l) -> u32 {
    const u32 word = pbits[l >> 5], bit = 1u << (l & 31);
    if (!(word & bit)) {
      // (a sum on a slot of the compacted range that is not in the batch)
      XF_DASSERT(lo + l >= (u64)*f.rk_cap);
      return 0xFFFFFFFFu;
    }
    return rpre[l >> 5] + (u32)__popc(word & (bit - 1u));
  };
  // slice bits of a slot: one plain store per slot inside [lo, lo + kR), an
  // atomic OR for a slot that straddles its edge (S not dividing kR)
  auto put_mask = [&](u64 slot, u32 bits) {
    u64 m = slot;
    if (f.out) {  // (NV == 1, S > 1) unique order
      m = uix(f.inv, slot);
      if (m == 0xFFFFFFFFu) return;
    }
    if (slot * S >= lo && slot * S + S <= lo + kR) f.masks[m] = bits;
    else atomicOr(&f.masks[m], bits);
  };
  // the sum of dest lo + l (skipped when zero: grad is zero outside this
  // step's keys -- except a present slice of the unique-order S > 1 output,
  // which the apply reads by its slice bit)
  auto emit = [&](u32 l, bool present) {
    const u64 dest = lo + l;
    if constexpr (NV == 1) {
      const long long a = acc[l];
      if (a == 0 && !(present && f.out && S > 1)) return;
      if (f.out) {
        // normalised like the gather would (lr_worker.cc:116-118, in double);
        // S > 1: [unique][slice], per-slice rows
        const u64 slot = dest / S, sl = dest - slot * S;
        const u32 o = rank ? rank_of(l) : uix(f.inv, slot);
        if (o != 0xFFFFFFFFu)  // (not the trash slot)
          f.out[(u64)o * S + sl] = (float)(fx_to_double<kFx>(a) / (double)f.rows[sl]);
      } else {
        f.grad[dest] = (float)fx_to_double<kFx>(a);
      }
    } else {
      // (a present slice of the S > 1 unique-order output is written even
      // when zero: the apply reads it by its slice bit)
      if (acc[2 * l] == 0 && acc[2 * l + 1] == 0 && !(present && f.out && S > 1)) return;
      const float B = (float)fx_to_double<kFx>(acc[2 * l]);
      const float C = (float)fx_to_double<kFx>(acc[2 * l + 1]);
      if (f.compact) {  // expanded by the apply (k_apply_group)
        if (f.out) {    // unique (send) order; S > 1: [unique][slice]
          const u64 slot = dest / S, sl = dest - slot * S;
          const u32 o0 = rank ? rank_of(l) : uix(f.inv, slot);
          if (o0 == 0xFFFFFFFFu) return;
          const u64 o = (u64)o0 * S + sl;
          if (f.rows) {  // normalised before the expansion (the send buffer, the fused step)
            const double rows = (double)f.rows[sl];  // (one rounding, as k_red_csr)
            reinterpret_cast<float2*>(f.out)[o] =
                make_float2((float)(fx_to_double<kFx>(acc[2 * l]) / rows),
                            (float)(fx_to_double<kFx>(acc[2 * l + 1]) / rows));
          } else {  // normalised by the apply
            reinterpret_cast<float2*>(f.out)[o] = make_float2(B, C);
          }
        } else {
          *reinterpret_cast<float2*>(f.grad + dest * f.ps) = make_float2(B, C);
        }
        return;
      }
      // rows are padded to 16 B: dwordx4 loads of v and stores of the row
      const float4* v4 = reinterpret_cast<const float4*>(f.wpull + (dest / S) * f.ps);
      float4* g4 = reinterpret_cast<float4*>(f.grad + dest * f.ps);
      for (int q = 0; q < f.ps / 4; ++q) {
        const float4 v = v4[q];
        float o[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = 4 * q + e;  // component: 0 = w, 1..D = v, above = pad
          o[e] = c == 0 ? (float)f.D * B : (c <= f.D ? C - o[e] * B : 0.0f);
        }
        g4[q] = make_float4(o[0], o[1], o[2], o[3]);
      }
    }
  };
  if constexpr (kSeg) {
    if (apply) {
      // The unit's stamped slots are the keys [r0, r0 + cnt) of the unique
      // list, in slot order (rank_of), and thread t applies the keys r0 + t,
      // + kRedBlock, ...: the slot and (n, z) reads are dense and the lanes of
      // the FTRL arithmetic all live, where one lane per slot of the
      // 4x-headroom scratch would leave four of five idle.  The way from a key
      // back to its sum goes through the accumulators' own words: dest l's
      // normalised sum -- a zero sum too: k_apply_lr16 pushes g = 0 -- replaces
      // the low word of acc[l], written by the thread that read it; after a
      // barrier (every sum has been read) l goes to the high word of
      // acc[rank - r0].  Every stamped slot below the capacity leads a tile of
      // k_lr_lead, so it has a record in this unit and is handled exactly
      // once -- in the sparse form by the record that claims its bit, as
      // emit's.
      constexpr u32 kNone = 0xFFFFFFFFu;
      const u32 r0 = rpre[0];  // (lo below the capacity, else cnt == 0)
      u32 cnt = 0;
#pragma unroll
      for (u32 i = 0; i < kRw / kWave; ++i) cnt += rwt[i];
      u32* aw = reinterpret_cast<u32*>(acc);
      // as emit: normalised like the gather would (lr_worker.cc:116-118, in double)
      auto put_sum = [&](u32 l) {
        aw[2 * l] = __float_as_uint((float)(fx_to_double<kFx>(acc[l]) / (double)f.rows[0]));
      };
      u32 mine = 0;  // (sparse) the records that claimed their dest
      if (dense) {
        for (u32 l = threadIdx.x; l < kR; l += kRedBlock)
          if (rank_of(l) != kNone) put_sum(l);
      } else {
#pragma unroll
        for (int q = 0; q < kSp; ++q) {
          const u32 l = lr[q];
          if (l >= kR) continue;
          const u32 bit = 1u << (l & 31);
          if (atomicOr(&cbits[l >> 5], bit) & bit) continue;
          if (rank_of(l) == kNone) continue;
          mine |= 1u << q;
          put_sum(l);
        }
      }
      lds_barrier();
      if (dense) {
        for (u32 l = threadIdx.x; l < kR; l += kRedBlock) {
          const u32 o = rank_of(l);
          if (o != kNone) aw[2 * (o - r0) + 1] = l;
        }
      } else {
#pragma unroll
        for (int q = 0; q < kSp; ++q)
          if (mine & (1u << q)) aw[2 * (rank_of(lr[q]) - r0) + 1] = lr[q];
      }
      lds_barrier();
      // kAp keys' inputs in flight together (indices past the unit's keys are
      // clamped, not predicated: no branch around a load), then their pushes
      // and stores.  A unit of more than kAp kRedBlock keys -- a scratch more
      // than a quarter full -- takes another round, whose loads queue behind
      // the first round's stores (vmcnt counts both).
      constexpr int kAp = 4;
      const FtrlParams fp = f.ap_fp;
      for (u32 j0 = threadIdx.x; j0 < cnt; j0 += kAp * kRedBlock) {
        u32 slot[kAp];
        float2 nz[kAp];
        float g[kAp];
#pragma unroll
        for (int q = 0; q < kAp; ++q) {
          const u32 j = j0 + (u32)q * kRedBlock;
          const u32 jc = j < cnt ? j : cnt - 1u;
          slot[q] = f.ap_slots[r0 + jc];
          nz[q] = f.ap_nz[r0 + jc];
          g[q] = __uint_as_float(aw[2 * (aw[2 * jc + 1] & (kR - 1u))]);  // (masked: an index inside the unit, whatever the word)
        }
#pragma unroll
        for (int q = 0; q < kAp; ++q) {
          // (kNoSlot: not admitted, or the table had no room)
          if (j0 + (u32)q * kRedBlock >= cnt || slot[q] == kNoSlot) continue;
          const float w = ftrl_weight(nz[q].y, nz[q].x, fp);
          ftrl_push(nz[q].x, nz[q].y, w, g[q], fp);
          *reinterpret_cast<float2*>(f.ap_words + (u64)slot[q] * 4 + 2) = nz[q];
        }
      }
      return;
    }
  }
  if (dense) {
    for (u32 l = threadIdx.x; l < kR; l += kRedBlock)
      emit(l, f.masks && ((pbits[l >> 5] >> (l & 31)) & 1u));
    if (f.masks) {
      const u64 s0 = lo / S, s1 = (lo + kR + S - 1) / S;
      for (u64 slot = s0 + threadIdx.x; slot < s1; slot += kRedBlock) {
        const u32 bits = slot_bits<kR>(pbits, slot, S, lo);
        if (bits) put_mask(slot, bits);
      }
    }
  } else {
    // one writer per dest (the record that claims its bit), and per slot the
    // writer of its lowest present dest
#pragma unroll
    for (int q = 0; q < kSp; ++q) {
      const u32 l = lr[q];
      if (l >= kR) continue;
      const u32 bit = 1u << (l & 31);
      if (atomicOr(&cbits[l >> 5], bit) & bit) continue;
      emit(l, true);
      if (f.masks) {
        const u64 slot = (lo + l) / S;
        const u32 bits = slot_bits<kR>(pbits, slot, S, lo);
        if (slot * S + (u64)__ffs(bits) - 1 == lo + l) put_mask(slot, bits);
      }
    }
  }
}

// A persistent grid (one workgroup per CU: the accumulator fills the LDS)
// walks this step's (bucket, sub) units -- a bucket of 2^shift dests is
// summed in 2^(shift - kShift) units of kR dests (one in the common case) --
// so the sparse units of a many-slice step do not each pay a workgroup
// launch; the next unit's record range is loaded during the current one.
template <int NV>
__global__ void __launch_bounds__(kRedBlock) k_red_sum(const void* __restrict__ sorted,
                                                       const u32* __restrict__ start, RedFinal f,
                                                       RedGeom geom, int nb) {
  constexpr int kShift = red_shift(NV);
  constexpr u32 kR = 1u << kShift;
  // fixed-point accumulators: the bucket's sums do not depend on record order
  __shared__ long long acc[kR * NV];
  __shared__ u32 pbits[kR / 32];  // (f.masks) dests some record reached
  __shared__ u32 cbits[kR / 32];  // (sparse) dests whose sum is being stored
  __shared__ u32 rpre[kR / 32];   // (f.rk_offs) unique index of the first stamped slot of a bitmap word
  __shared__ u32 rwt[kR / 32 / kWave];
  const int shift = geom.shift(kShift);
  const u32 act = (u32)geom.active(shift, nb);
  const u32 units = act << (shift - kShift);
  u32 id = blockIdx.x, nbeg = 0, nend = 0;
  if (id < units) {
    nbeg = start[id % act];
    nend = start[id % act + 1];
  }
  for (; id < units; id += gridDim.x) {
    const u32 beg = nbeg, end = nend, b = id % act, sub = id / act;
    const u32 nid = id + gridDim.x;
    if (nid < units) {
      nbeg = start[nid % act];
      nend = start[nid % act + 1];
    }
    const u64 lo = ((u64)b << shift) + ((u64)sub << kShift);
    red_sum_unit<NV>(lo, beg, end, sorted, f, acc, pbits, cbits, rpre, rwt);
    lds_barrier();  // the next unit reinitialises what this one read
  }
}

// k_red_sum<1> on the producers' bucket-sorted regions (FwdArgs::red_local):
// no k_red_scan, no k_red_scatter, no red_sorted.  Per unit the workgroup
// reads its bucket's row of lead_seg words once to decide the form: every
// wave counts the 64-record rows of its segments; the unit is sparse when no
// wave has more than the 2 kRedUnroll rows its lanes have record slots for
// (and at most kWave segments), else dense.  Nothing here depends on another
// workgroup of this launch.
// snap: the step's capacity snapshot, when this launch stands in for the
// apply's (RedFinal::ap_*): the pulls and the forward have completed.
struct RedSnap {
  HostSnap* dst = nullptr;
  const u32* mon = nullptr;
  unsigned long long seq = 0;
};
__global__ void __launch_bounds__(kRedBlock) k_red_sum_local(LeadSegs sg, RedFinal f, RedGeom geom,
                                                             int nb, RedSnap snap) {
  if (snap.dst) store_snapshot(snap.dst, snap.mon, snap.seq);
  constexpr int kShift = red_shift(1);
  constexpr u32 kR = 1u << kShift;
  constexpr u32 kWaves = kRedBlock / kWave;
  constexpr u32 kSp = 2 * kRedUnroll;
  __shared__ long long acc[kR];
  __shared__ u32 pbits[kR / 32];
  __shared__ u32 cbits[kR / 32];
  __shared__ u32 rpre[kR / 32];
  __shared__ u32 rwt[kR / 32 / kWave];
  __shared__ u32 s_rows[kWaves];  // 64-record rows of each wave's segments
  const int shift = geom.shift(kShift);
  const u32 act = (u32)geom.active(shift, nb);
  const u32 units = act << (shift - kShift);
  const u32 lane = threadIdx.x % kWave, w = threadIdx.x / kWave;
  const u32 per = (sg.groups + kWaves - 1) / kWaves;
  const u32 gb = w * per, ge = gb + per < sg.groups ? gb + per : sg.groups;
  for (u32 id = blockIdx.x; id < units; id += gridDim.x) {
    const u32 b = id % act, sub = id / act;
    sg.row = sg.hist + (size_t)b * sg.groups;
    u32 rows = 0;
    for (u32 c0 = gb; c0 < ge; c0 += kWave) {
      u32 off, cnt;
      sg.seg(c0 + lane < ge ? sg.row[c0 + lane] : 0u, off, cnt);
      rows += (cnt + kWave - 1) / kWave;
    }
    rows = wave_sum_u32(rows);
    if (lane == 0) s_rows[w] = rows;
    lds_barrier();
    u32 tot = 0, most = 0;
#pragma unroll
    for (u32 i = 0; i < kWaves; ++i) {
      tot += s_rows[i];
      most = most > s_rows[i] ? most : s_rows[i];
    }
    sg.any = tot != 0u;
    sg.dense = most > kSp || per > (u32)kWave;
    const u64 lo = ((u64)b << shift) + ((u64)sub << kShift);
    red_sum_unit<1, true>(lo, 0u, 0u, nullptr, f, acc, pbits, cbits, rpre, rwt, sg);
    lds_barrier();  // the next unit reinitialises what this one read
  }
}

// ---------------------------------------------------------------------------
// CSR reduction (FwdArgs::red_csr): every slice of the step in one pass.
// Dests are key * 2^slog2 + slice, so a bucket's dests are whole keys and
// the bucket's distinct dests in dest order ARE its keys' entries in (key,
// slice) order.  Per bucket (one workgroup), per window of 2^16 dests:
//   1. a presence bitmap of the window's dests (one bit per dest: 8 KB) and
//      its prefix popcounts -> the rank of every present dest;
//   2. per key of the window: cnt = its present slices, off = rank of the
//      first (entries start at the bucket's first record index: a bucket
//      has at most as many distinct dests as records);
//   3. the sums: an LDS hash table keyed by dest when the window holds at
//      most kCsrHash / 2 records (the common case: a bucket's records are a
//      sparse sample of its dests), else direct-indexed sub-windows of
//      kCsrHash dests; fixed-point int64 (order-free, deterministic), each
//      distinct dest written once at its rank.
// A bucket of at most kCsrReg * kCsrBlock records keeps them in registers
// across the passes.
// ---------------------------------------------------------------------------
constexpr int kCsrBlock = 512;
constexpr int kCsrWinLog2 = 16;
constexpr int kCsrWords = 1 << (kCsrWinLog2 - 5);
constexpr int kCsrHash = 4096;
constexpr int kCsrReg = 4;

template <int NV>
__global__ void __launch_bounds__(kCsrBlock) k_red_csr(const void* __restrict__ sorted,
                                                       const u32* __restrict__ start, CsrOut c,
                                                       RedGeom geom, int nb) {
  using T = typename RedRec<NV>::T;
  constexpr int kFx = FxBits<NV>::kFx;
  constexpr int kWaves = kCsrBlock / kWave;
  __shared__ u32 bits[kCsrWords];
  __shared__ u32 wscan[kCsrWords];
  __shared__ u32 tag[kCsrHash];
  __shared__ long long acc[kCsrHash * NV];
  __shared__ u32 s_part[kWaves];
  const int shift = geom.shift(red_shift(NV));
  const int b = (int)blockIdx.x;
  if (b >= geom.active(shift, nb)) return;
  const u32 beg = start[b], end = start[b + 1];
  if (beg == end) return;  // (no records: no key of the batch has a dest here)
  const u64 nuq = *geom.nuq;
  const T* src = static_cast<const T*>(sorted);
  const u64 blo = (u64)b << shift, bhi = blo + (1ull << shift);
  const int wl2 = shift < kCsrWinLog2 ? shift : kCsrWinLog2;
  const u32 wn = 1u << wl2;
  const int sl = c.slog2;
  const u32 smask = (1u << sl) - 1u;
  const u32 nrec = end - beg;
  const int tid = (int)threadIdx.x;
  const bool reg = nrec <= (u32)(kCsrReg * kCsrBlock) && shift <= kCsrWinLog2;
  T pr[kCsrReg];
  u32 pd[kCsrReg];  // (reg) the record's dest - blo, ~0: none
#pragma unroll
  for (int q = 0; q < kCsrReg; ++q) {
    pd[q] = ~0u;
    const u32 i = beg + (u32)tid + (u32)q * kCsrBlock;
    if (reg && i < end) {
      pr[q] = src[i];
      pd[q] = (u32)((u64)RedRec<NV>::dest(pr[q]) - blo);
    }
  }
  auto rank = [&](u32 d) -> u32 {
    return wscan[d >> 5] + (u32)__popc(bits[d >> 5] & ((1u << (d & 31)) - 1u));
  };
  auto emit = [&](u32 o, u32 d, const long long* a) {
    const u32 slice = d & smask;
    const double rows = c.rows ? (double)c.rows[slice] : 1.0;
    if constexpr (NV == 1) {
      const float v = (float)(fx_to_double<kFx>(a[0]) / rows);
      static_cast<u64*>(c.ent)[o] = (u64)slice | ((u64)__float_as_uint(v) << 32);
    } else {
      const float B = (float)(fx_to_double<kFx>(a[0]) / rows);
      const float C = (float)(fx_to_double<kFx>(a[1]) / rows);
      static_cast<uint3*>(c.ent)[o] = make_uint3(slice, __float_as_uint(B), __float_as_uint(C));
    }
  };
  auto add = [&](u32 h, const T& r) {
    if constexpr (NV == 1) {
      atomicAdd(reinterpret_cast<unsigned long long*>(&acc[h]),
                (unsigned long long)fx_from<kFx>(__uint_as_float((u32)(r >> 32))));
    } else {
      atomicAdd(reinterpret_cast<unsigned long long*>(&acc[2 * h]),
                (unsigned long long)fx_from<kFx>(__uint_as_float(r.y)));
      atomicAdd(reinterpret_cast<unsigned long long*>(&acc[2 * h + 1]),
                (unsigned long long)fx_from<kFx>(__uint_as_float(r.z)));
    }
  };
  u32 out = beg;
  for (u64 wlo = blo; wlo < bhi; wlo += wn) {
    const u32 woff = (u32)(wlo - blo);
    // 1. presence bitmap of the window
    for (u32 i = (u32)tid; i < (wn >> 5); i += kCsrBlock) bits[i] = 0u;
    lds_barrier();
    u32 mine = 0;
    if (reg) {
#pragma unroll
      for (int q = 0; q < kCsrReg; ++q) {
        const u32 d = pd[q] - woff;
        if (pd[q] != ~0u && d < wn) {
          atomicOr(&bits[d >> 5], 1u << (d & 31));
          ++mine;
        }
      }
    } else {
      for (u32 i = beg + (u32)tid; i < end; i += kCsrBlock) {
        const u64 d = (u64)RedRec<NV>::dest(src[i]) - wlo;
        if (d < wn) {
          atomicOr(&bits[d >> 5], 1u << (d & 31));
          ++mine;
        }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if (tid % kWave == 0) s_part[tid / kWave] = mine;
    lds_barrier();
    u32 nwin = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) nwin += s_part[w];
    if (nwin == 0) continue;  // (block-uniform)
    // prefix popcounts: each lane scans wn / 32 / kCsrBlock consecutive words
    constexpr int kPer = kCsrWords / kCsrBlock;
    const u32 nwords = wn >> 5;
    u32 loc[kPer], tl = 0;
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
      const u32 w = (u32)tid * kPer + (u32)q;
      loc[q] = w < nwords ? (u32)__popc(bits[w]) : 0u;
      tl += loc[q];
    }
    u32 total;
    u32 ex = block_exclusive_scan<kCsrBlock>(tl, &total);
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
      const u32 w = (u32)tid * kPer + (u32)q;
      if (w < nwords) wscan[w] = ex;
      ex += loc[q];
    }
    lds_barrier();
    // 2. per key: entry count and first entry
    {
      const u64 k0 = wlo >> sl;
      const u32 nk = wn >> sl;
      for (u32 kk = (u32)tid; kk < nk; kk += kCsrBlock) {
        const u64 k = k0 + kk;
        if (k >= nuq) break;
        const u32 o = kk << sl;
        u32 cnt = 0, first = ~0u;
        if (sl < 5) {  // (the key's 2^sl presence bits inside one word)
          const u32 m = (bits[o >> 5] >> (o & 31)) & ((1u << (1u << sl)) - 1u);
          cnt = (u32)__popc(m);
          if (m) first = o + (u32)__ffs(m) - 1u;
        } else {
          for (u32 w = 0; w < (1u << (sl - 5)); ++w) {
            const u32 x = bits[(o >> 5) + w];
            cnt += (u32)__popc(x);
            if (x && first == ~0u) first = o + 32u * w + (u32)__ffs(x) - 1u;
          }
        }
        c.cnt[k] = cnt;
        c.off[k] = out + (cnt ? rank(first) : 0u);
      }
    }
    // 3. sums, each distinct dest written once at its rank
    if (nwin <= (u32)(kCsrHash / 2)) {
      for (u32 i = (u32)tid; i < (u32)kCsrHash; i += kCsrBlock) {
        tag[i] = ~0u;
#pragma unroll
        for (int v = 0; v < NV; ++v) acc[i * NV + v] = 0ll;
      }
      lds_barrier();
      auto insert = [&](u32 d, const T& r) {
        u32 h = (d * 0x9E3779B1u) >> (32 - ilog2c(kCsrHash));
        while (true) {  // (one CAS against an empty slot per probe step)
          const u32 old = atomicCAS(&tag[h], ~0u, d);
          if (old == ~0u || old == d) break;
          h = (h + 1) & (kCsrHash - 1);
        }
        add(h, r);
      };
      if (reg) {
#pragma unroll
        for (int q = 0; q < kCsrReg; ++q) {
          const u32 d = pd[q] - woff;
          if (pd[q] != ~0u && d < wn) insert(d, pr[q]);
        }
      } else {
        for (u32 i = beg + (u32)tid; i < end; i += kCsrBlock) {
          const T r = src[i];
          const u64 d = (u64)RedRec<NV>::dest(r) - wlo;
          if (d < wn) insert((u32)d, r);
        }
      }
      lds_barrier();
      for (u32 i = (u32)tid; i < (u32)kCsrHash; i += kCsrBlock) {
        const u32 d = tag[i];
        if (d != ~0u) emit(out + rank(d), d, &acc[i * NV]);
      }
      lds_barrier();
    } else {
      for (u32 sub = 0; sub < wn; sub += kCsrHash) {
        for (u32 i = (u32)tid; i < (u32)(kCsrHash * NV); i += kCsrBlock) acc[i] = 0ll;
        lds_barrier();
        // (never the register form: it holds at most kCsrReg * kCsrBlock =
        // kCsrHash / 2 records, and this branch has more in one window)
        for (u32 i = beg + (u32)tid; i < end; i += kCsrBlock) {
          const T r = src[i];
          const u64 d = (u64)RedRec<NV>::dest(r) - wlo - sub;
          if (d < (u64)kCsrHash) add((u32)d, r);
        }
        lds_barrier();
        for (u32 l = (u32)tid; l < (u32)kCsrHash; l += kCsrBlock) {
          const u32 d = sub + l;
          if ((bits[d >> 5] >> (d & 31)) & 1u) emit(out + rank(d), d, &acc[l * NV]);
        }
        lds_barrier();
      }
    }
    out += total;
  }
}

// the outputs of k_red_sum / k_red_sum_local
template <int NV>
static RedFinal red_final(const FwdArgs& a) {
  if (a.red_out && (NV == 2 ? !a.fm_compact : false))
    throw std::runtime_error("red_out: compact rows (reference FM)");
  if (a.red_out && a.S != 1 && !a.red_masks)
    throw std::runtime_error("red_out with several slices needs the slice bits (red_masks)");
  RedFinal f{a.grad, a.wpull, a.S, a.model.pstride(), a.model.v_dim,
             a.red_out, a.red_inv, a.red_rows, NV == 2 && a.fm_compact,
             a.S > 1 ? a.red_masks : nullptr};
  if (a.red_apply_slots) {
    // (the sums are pushed where they would be stored: k_red_sum_local's ranks)
    if (NV != 1 || !a.red_local || a.red_out || !a.red_rank_offs || !a.red_rows ||
        !a.red_apply_words || !a.red_apply_nz)
      throw std::runtime_error("red_apply: the ranked bucket-sorted LR step only (plan_step)");
    f.ap_words = a.red_apply_words;
    f.ap_slots = a.red_apply_slots;
    f.ap_nz = reinterpret_cast<const float2*>(a.red_apply_nz);
    f.ap_fp = a.red_apply_ftrl;
  }
  if (a.red_rank_offs && (a.red_out || a.red_apply_slots)) {
    // (dests are slots, the slice bits' bitmap is free for the stamps)
    if (a.S != 1 || a.red_nuq || !a.red_rank_stamps || !a.red_bcap)
      throw std::runtime_error("red_rank: one slice, slot positions, the batch's stamps and capacity");
    f.rk_offs = a.red_rank_offs;
    f.rk_stamps = a.red_rank_stamps;
    f.rk_cap = a.red_bcap;
    f.rk_epoch = a.red_rank_epoch;
    f.inv = nullptr;
  }
  return f;
}

template <int NV>
void launch_reduction(const FwdArgs& a, int groups, int rows_per_group, hipStream_t st) {
  if (a.red_local) {
    // the producer (k_lr_lead<true>) left each bucket's records as one segment
    // per workgroup region: the sums read them in place
    const BatchView& b = a.batch;
    if (NV != 1 || !a.lead || a.S != 1 || a.red_masks || a.red_nuq || a.red_csr.cnt || b.row_ptr ||
        rows_per_group != kLeadTile || b.nnz_per_row < 1 || b.nnz_per_row > kLeadMaxFields ||
        (int64_t)groups * kLeadTile != b.rows)
      throw std::runtime_error("red_local: the LR leader handoff step only (plan_step)");
    LeadSegs sg;
    sg.pairs = a.red_pairs;
    sg.hist = a.red_hist;
    sg.groups = (u32)groups;
    sg.gcap = (u32)(kLeadTile * b.nnz_per_row);
    const u32 grid = std::min<u32>((u32)(a.red_nb * a.red_nsub), (u32)device_cus());
    RedSnap snap;
    if (a.red_apply_slots) snap = {a.snap, a.snap_mon, a.snap_seq};
    hipLaunchKernelGGL(k_red_sum_local, dim3(grid), dim3(kRedBlock), 0, st, sg, red_final<1>(a),
                       red_geom(a), a.red_nb, snap);
    return;
  }
  u32* start = a.red_tot + a.red_nb + 1;
  hipLaunchKernelGGL(k_red_scan, dim3(a.red_nb), dim3(kBlock), 0, st, a.red_hist, groups,
                     a.red_tot, red_geom(a), red_shift(NV));
  hipLaunchKernelGGL(k_red_scatter<NV>, dim3(groups), dim3(kRedBlock), 0, st, a.batch,
                     rows_per_group, static_cast<const void*>(a.red_pairs), a.red_count,
                     a.red_hist, a.red_tot, start, a.red_nb, static_cast<void*>(a.red_sorted),
                     red_geom(a));
  if (a.red_csr.cnt) {
    if (!a.red_nuq || a.red_out || a.S != (1 << a.red_csr.slog2) ||
        a.red_csr.slog2 > red_shift(NV) || (NV == 2 && !a.fm_compact))
      throw std::runtime_error("CSR reduction: unique positions, S = 2^slog2 <= 2^shift, no other outputs");
    hipLaunchKernelGGL(k_red_csr<NV>, dim3(a.red_nb), dim3(kCsrBlock), 0, st,
                       static_cast<const void*>(a.red_sorted), start, a.red_csr, red_geom(a), a.red_nb);
    return;
  }
  const RedFinal f = red_final<NV>(a);
  const u32 grid = std::min<u32>((u32)(a.red_nb * a.red_nsub), (u32)device_cus());
  hipLaunchKernelGGL(k_red_sum<NV>, dim3(grid), dim3(kRedBlock), 0, st,
                     static_cast<const void*>(a.red_sorted), start, f, red_geom(a), a.red_nb);
}
template void launch_reduction<1>(const FwdArgs&, int, int, hipStream_t);
template void launch_reduction<2>(const FwdArgs&, int, int, hipStream_t);

}  // namespace hip
}  // namespace xflow
